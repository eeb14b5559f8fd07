"""CPU-side checks of the moving camera (include/rusty_marcher_amd.h, "moving camera").

1. The five entry points are exported and bound by ctypes, the Rust shim and the C++ mirror with the header's shapes,
   rm_camera_motion is 48 bytes, rm_build_info says " moving-camera" and the ABI is still 5, a NULL context is refused with
   nothing written, and the Python wrappers raise before the library is called.
2. rm_camera_sequence: the offsets against a numpy restatement and against rm_motion_sequence's bytes for the same velocity,
   the bases against the library's own rm_camera_basis_turn row by row (no libm in the test), rates of zero keep the basis byte
   for byte, row 0 is the camera as it stands, and every refusal writes nothing.
3. tests/camera_motion_reference.py -- the yardstick of the GPU tests -- is moving_reference.samples byte for byte for a camera
   that stands still under an oriented view, and is not vacuous: every test motion changes the committed number of pixels, each
   more than 5 % of the frame."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import camera_motion_reference as CM
import lens_reference as LR
import motion_reference as MR
import moving_reference as MV
import progressive_reference as PR
import radiance_reference as RR
import soft_reference as SR
import test_rust_binding as RB
import workloads

FUNCTIONS = ["rm_camera_sequence", "rm_accumulate_camera_device", "rm_accumulate_converging_camera_device", "rm_render_progressive_camera",
             "rm_render_converging_camera"]
D, U8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)


def basis(pkg):
    """An oriented basis the library accepts, made by the library."""
    return pkg.backend.basis_look_at((3., 1., 2.), (0., 0., -10.))


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_camera_abi"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return CM.Yardstick(pkg, O, orc)


# ---------------------------------------------------------------- the ABI
def test_camera_symbols_are_exported_and_bound(pkg, entry):
    L = pkg.lib()
    header = open(os.path.join(entry.ROOT, "include", "rusty_marcher_amd.h")).read()
    for name in FUNCTIONS:
        assert hasattr(L, name), "library does not export %s" % name
        assert name in pkg._lib.SIGNATURES
        assert re.search(r"^rm_status %s\(" % name, header, flags=re.M), name
    for name in ("accumulate_camera_device", "accumulate_converging_camera_device", "render_progressive_camera", "render_converging_camera",
                 "camera_sequence"):
        assert callable(getattr(pkg.backend.Context, name))
    assert callable(pkg.backend.camera_sequence)
    for name in ("render_progressive_camera", "render_camera_blur", "render_converging_camera", "render_converged_camera"):
        assert callable(getattr(pkg.Renderer, name))


def test_struct_sizes_and_build_info(pkg):
    L, B = pkg.lib(), pkg._lib
    assert C.sizeof(B.rm_camera_motion) == 48 and C.sizeof(B.rm_camera_basis) == 72
    assert B.rm_camera_motion.yaw.offset == 24 and B.rm_camera_motion.roll.offset == 40
    info = L.rm_build_info().decode()
    assert "moving-camera" in info.split(" ") and " moving-shapes" in info and " converge-moving" in info
    assert L.rm_abi_version() == 5


def test_camera_functions_have_the_header_shapes_in_the_rust_shim_and_the_cpp_mirror(entry):
    c, r = RB.header_functions(), RB.rust_functions()
    for name in FUNCTIONS:
        assert name in c and name in r, name
        assert c[name] == r[name], "%s: header %s, gpu.rs %s" % (name, c[name], r[name])
    # the siblings' lists with the camera's rows (a pointer) behind the table, and the motion (a pointer) behind the shutter
    moving = c["rm_accumulate_moving_device"][1]
    assert c["rm_accumulate_camera_device"] == ("i32", moving[:4] + ["ptr"] + moving[4:])
    moving = c["rm_accumulate_converging_moving_device"][1]
    assert c["rm_accumulate_converging_camera_device"] == ("i32", moving[:6] + ["ptr"] + moving[6:])
    for tick, sibling in (("rm_render_progressive_camera", "rm_render_progressive_moving"), ("rm_render_converging_camera", "rm_render_converging_moving")):
        s = c[sibling][1]
        k = s.index("f64") + 1
        assert c[tick] == ("i32", s[:k] + ["ptr"] + s[k:])
    assert c["rm_camera_sequence"] == ("i32", ["u32", "u32", "ptr", "ptr", "f64", "ptr"])
    assert dict(RB.header_structs())["rm_camera_motion"] == dict(RB.rust_structs())["RmCameraMotion"]
    text = open(RB.RUST).read()
    assert re.search(r"pub fn render_progressive_camera\(\s*&mut self", text) and re.search(r"pub fn render_converging_camera\(\s*&mut self", text)
    hpp = open(os.path.join(entry.PKG_DIR, "host", "rusty_marcher.hpp")).read()
    assert "rm_render_progressive_camera(ctx_" in hpp and "rm_render_converging_camera(ctx_" in hpp


def test_cpp_mirror_compiles_with_the_camera_renders(entry, tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "rusty_marcher.hpp"\nusing namespace rusty_marcher;\n'
                   'rm_converge_report tick(renderer::Renderer &r, framebuffer::FrameBuffer &fb, const scene::Scene &sc) {'
                   ' const rm_camera_motion m{{1., 0., 0.5}, 0.1, 0., 0.};'
                   ' std::vector<Vec3f> v(sc.shapes.size(), Vec3f{0., 1., 0.});'
                   ' r.render_progressive_camera(fb, sc, m, 1., 8u); r.render_progressive_camera(fb, sc, m, 0.5, 8u, v, {1.5, 0.}, 0.4, 5., true);'
                   ' return r.render_converging_camera(fb, sc, m, 1., rm_converge{0.1, 16u, 256u}, 8u, v); }\n'
                   'int main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(entry.ROOT, "include"),
                           "-I", os.path.join(entry.PKG_DIR, "host"), str(src)])


def test_camera_entry_points_refuse_null_context(pkg):
    L, B = pkg.lib(), pkg._lib
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 3)
    lens, conv = B.rm_lens(LR.APERTURE, LR.FOCUS, 4, 0), B.rm_converge(0.1, 16, 64)
    motion = B.rm_camera_motion(B.rm_vec3(1., 0., 0.), 0.1, 0., 0.)
    frame, bytes8, total = np.full((64, 64, 3), 7.25), np.full((64, 64, 3), 7, np.uint8), C.c_uint32(77)
    report = B.rm_converge_report(5, 6, 7, 8, 0)
    E = B.RM_ERR_INVALID_ARG
    assert L.rm_accumulate_camera_device(None, C.byref(p), C.byref(lens), None, None, None, 2, None, 3, 0, None, None, None, None) == E
    assert b"rm_accumulate_camera_device: NULL ctx" in L.rm_last_error(None)
    assert L.rm_accumulate_converging_camera_device(None, C.byref(p), C.byref(lens), C.byref(conv), None, 64, None, None, 2, None, 3, 1, None, None) == E
    assert b"rm_accumulate_converging_camera_device: NULL ctx" in L.rm_last_error(None)
    assert L.rm_render_progressive_camera(None, C.byref(p), C.byref(lens), None, 0, None, 0, 1., C.byref(motion), 0, frame.ctypes.data_as(D),
                                          bytes8.ctypes.data_as(U8), C.byref(total), None) == E
    assert b"rm_render_progressive_camera: NULL ctx" in L.rm_last_error(None)
    assert L.rm_render_converging_camera(None, C.byref(p), C.byref(lens), C.byref(conv), None, 0, None, 0, 1., C.byref(motion), 0,
                                         frame.ctypes.data_as(D), bytes8.ctypes.data_as(U8), C.byref(report), None) == E
    assert b"rm_render_converging_camera: NULL ctx" in L.rm_last_error(None)
    assert np.all(frame == 7.25) and np.all(bytes8 == 7) and total.value == 77 and (report.samples_cast, report.listed) == (5, 6)


class _NoLibrary:
    """A Context whose library must not be reached: the wrappers refuse before they call it."""
    device, ptr = 0, None

    class L:
        def __getattr__(self, name):
            raise AssertionError("the library was called: %s" % name)
    L = L()


def test_python_wrappers_check_before_the_library_sees_anything(pkg):
    import torch
    K, ctx = pkg.backend, _NoLibrary()
    p = K.make_params(workloads.FOV, 64., 64., 3)
    nan, inf = float("nan"), float("inf")
    demo = pkg.Scene.create_default()
    n = len(demo.shapes)
    r, fb = pkg.create_renderer(workloads.FOV, 64., 64.), pkg.create_frame_buffer(64, 64)
    for velocity, turn in (((nan, 0., 0.), (0., 0., 0.)), ((0., inf, 0.), (0., 0., 0.)), ((1., 2.), (0., 0., 0.)), ((1., 0., 0.), (0., nan, 0.)),
                           ((1., 0., 0.), (0., 0.)), (1.5, (0., 0., 0.)), (None, (0., 0., 0.)), ((1., 0., 0.), "abc")):
        with pytest.raises(ValueError):
            K.Context.render_progressive_camera(ctx, p, velocity, 1., 0.4, 5., 4, turn)
        with pytest.raises(ValueError):
            K.Context.render_converging_camera(ctx, p, velocity, 1., 0.4, 5., 4, 0.1, 16, 64, turn)
        with pytest.raises(ValueError):
            r.render_progressive_camera(fb, demo, velocity, 1., 4, turn)
        with pytest.raises(ValueError):
            r.render_camera_blur(fb, demo, velocity, 1., 4, turn)
        with pytest.raises(ValueError):
            r.render_converging_camera(fb, demo, velocity, 1., 0.1, 4, turn)
        with pytest.raises(ValueError):
            K.camera_sequence(0, 4, velocity, 1., turn)
    good = (1., 0., 0.5)
    for shutter in (-0.1, nan, inf, "1", None, True):
        with pytest.raises(ValueError, match="shutter"):
            K.Context.render_progressive_camera(ctx, p, good, shutter, 0.4, 5., 4)
        with pytest.raises(ValueError, match="shutter"):
            r.render_progressive_camera(fb, demo, good, shutter, 4)
        with pytest.raises(ValueError, match="shutter"):
            K.camera_sequence(0, 4, good, shutter)
    for bad in ([], [None] * (n - 1), [None] * (n + 1)):
        with pytest.raises(ValueError, match="one velocity a shape"):
            r.render_progressive_camera(fb, demo, good, 1., 4, velocities=bad)
        with pytest.raises(ValueError, match="one velocity a shape"):
            r.render_converging_camera(fb, demo, good, 1., 0.1, 4, velocities=bad)
    with pytest.raises(ValueError, match="one radius a light"):
        r.render_progressive_camera(fb, demo, good, 1., 4, light_radii=(1.5,))
    for aperture, focus, ns in ((-0.1, 5., 4), (0.4, 0., 4), (0.4, 5., 0), (0.4, 5., 65), (0.4, 5., 2.5)):
        with pytest.raises(ValueError):
            K.Context.render_progressive_camera(ctx, p, good, 1., aperture, focus, ns)
        with pytest.raises(ValueError):
            r.render_progressive_camera(fb, demo, good, 1., ns, aperture=aperture, focus=focus)
    for ns in (0, -1, 65537, 2.5, True):
        with pytest.raises(ValueError):
            r.render_camera_blur(fb, demo, good, 1., ns)
    for first, count in ((-1, 4), (0, -1), (65536, 1), (0.5, 1)):
        with pytest.raises(ValueError):
            K.camera_sequence(first, count, good, 1.)
    t = torch.zeros((64, 64, 3), dtype=torch.float64)
    table, lights = PR.lens_sequence(0, 4), np.zeros((4, 2, 3))
    for s in (np.zeros((64, 64, 3)), t.float(), t, None):               # (a sum that is no tensor of the context's device)
        with pytest.raises(ValueError):
            K.Context.accumulate_camera_device(ctx, p, s, 0.4, 5., table, np.zeros((4, 12)), lights, None, 0)
    for rows in (np.zeros((4, 11)), np.zeros((3, 12)), np.full((4, 12), nan), np.zeros(48), torch.zeros((4, 12), dtype=torch.float32)):
        with pytest.raises(ValueError, match="camera_rows"):
            K._camera_rows_tensor(rows, 4, torch.device("cpu"))
    assert K._camera_rows_tensor(np.zeros((4, 12)), 4, torch.device("cpu")).shape == (4, 12)


# ---------------------------------------------------------------- the sequence
def _sequence(pkg, first, count, motion, b, shutter, out=None):
    L, B = pkg.lib(), pkg._lib
    rows = np.full((max(count, 1), 12), 7.25) if out is None else out
    m = B.rm_camera_motion(B.vec3(motion[:3]), *motion[3:]) if motion is not None else None
    st = L.rm_camera_sequence(first, count, C.byref(m) if m is not None else None, C.byref(b) if b is not None else None, shutter,
                              rows.ctypes.data_as(D) if rows is not False else None)
    return st, rows


def test_the_offsets_are_the_restatement_and_the_shapes_sequence_byte_for_byte(pkg):
    b = basis(pkg)
    v = (2.5, -1.25, 0.3)
    for first, count, shutter in ((0, 16, 1.), (5, 40, 0.37), (65530, 6, 2.)):
        st, rows = _sequence(pkg, first, count, v + (0.3, -0.2, 0.1), b, shutter)
        assert st == 0
        ref = MR.motion_sequence(first, count, [v], shutter)[:, 0]     # numpy: velocity.c * (shutter * phi_17(s))
        assert rows[:, :3].tobytes() == ref.tobytes()
        off = np.zeros((count, 1, 3))
        assert pkg.lib().rm_motion_sequence(first, count, C.byref(pkg._lib.vec3(v)), 1, shutter, off.ctypes.data_as(D)) == 0
        assert rows[:, :3].tobytes() == off[:, 0].tobytes()             # the camera and the shapes of a sample share an instant
        assert rows[:, :3].tobytes() == CM.camera_rows(first, count, v, (0., 0., 0.), shutter=shutter)[:, :3].tobytes()


def test_the_bases_are_the_librarys_own_turn_row_by_row(pkg):
    L, B = pkg.lib(), pkg._lib
    b = basis(pkg)
    yaw, pitch, roll, shutter = 0.3, -0.2, 0.1, 0.75
    st, rows = _sequence(pkg, 3, 24, (1., 0., 0., yaw, pitch, roll), b, shutter)
    assert st == 0
    t = MR.motion_sequence(3, 24, [(1., 0., 0.)], shutter)[:, 0, 0]
    for k in range(24):
        out = B.rm_camera_basis()
        assert L.rm_camera_basis_turn(C.byref(b), yaw * t[k], pitch * t[k], roll * t[k], C.byref(out)) == 0
        assert rows[k, 3:].tobytes() == bytes(out), k
        assert L.rm_camera_basis_check(C.byref(out)) == 0
    assert len({rows[k, 3:].tobytes() for k in range(24)}) == 24           # every row another basis
    # ... and the yardstick's own path is that to rounding
    mine = CM.camera_rows(3, 24, (1., 0., 0.), (yaw, pitch, roll), RR.basis_tuple(b), shutter)
    assert np.abs(mine - rows).max() < 1e-14


def test_zero_rates_keep_the_basis_and_row_0_is_the_camera_as_it_stands(pkg):
    b = basis(pkg)
    for rates in ((0., 0., 0.), (-0., 0., -0.)):
        st, rows = _sequence(pkg, 0, 32, (4., 1., -2.) + rates, b, 1.)
        assert st == 0
        assert all(rows[k, 3:].tobytes() == bytes(b) for k in range(32))   # no re-orthonormalisation
    st, rows = _sequence(pkg, 0, 4, (4., 1., -2., 0.3, 0.2, 0.1), b, 1.)
    assert st == 0 and not rows[0, :3].any() and (rows[1:, :3] != 0.).all()
    assert np.abs(rows[0, 3:] - np.frombuffer(bytes(b), dtype=np.float64)).max() < 1e-15
    st, rows = _sequence(pkg, 7, 4, (4., 1., -2., 0.3, 0.2, 0.1), b, 0.)   # a shutter that never opens
    assert st == 0 and not rows[:, :3].any()


def test_every_refusal_of_the_sequence_writes_nothing(pkg):
    L, B = pkg.lib(), pkg._lib
    b = basis(pkg)
    nan, inf = float("nan"), float("inf")
    good = (1., 0., 0., 0.1, 0., 0.)
    skew = B.rm_camera_basis(B.vec3((1., 0., 0.)), B.vec3((0., 1., 0.)), B.vec3((0., 0.1, -1.)))
    cases = [(65533, 4, good, b, 1., "first + count"), (0, 4, None, b, 1., "NULL motion"), (0, 4, (nan, 0., 0., 0., 0., 0.), b, 1., "not finite"),
             (0, 4, (1., 0., 0., 0., inf, 0.), b, 1., "not finite"), (0, 4, good, b, -1., "shutter"), (0, 4, good, b, nan, "shutter"),
             (0, 4, good, None, 1., "NULL basis"), (0, 4, good, skew, 1., "rm_camera_sequence: ")]
    for first, count, motion, bb, shutter, text in cases:
        st, rows = _sequence(pkg, first, count, motion, bb, shutter)
        assert st == B.RM_ERR_INVALID_ARG and (rows == 7.25).all(), text
        assert text.encode() in L.rm_last_error(None) and b"rm_camera_sequence" in L.rm_last_error(None), L.rm_last_error(None)
    st, _ = _sequence(pkg, 0, 4, good, b, 1., out=False)
    assert st == B.RM_ERR_INVALID_ARG and b"NULL rows" in L.rm_last_error(None)
    st, rows = _sequence(pkg, 9, 0, None, None, nan)                       # count == 0 asks for nothing
    assert st == 0 and (rows == 7.25).all()


def test_the_python_sequence_is_the_librarys(pkg):
    b = basis(pkg)
    rows = pkg.backend.camera_sequence(2, 9, (1., 2., 3.), 0.5, (0.1, 0.2, 0.3), b)
    st, ref = _sequence(pkg, 2, 9, (1., 2., 3., 0.1, 0.2, 0.3), b, 0.5)
    assert st == 0 and rows.shape == (9, 12) and rows.tobytes() == ref.tobytes()
    fixed = pkg.backend.camera_sequence(0, 3, (1., 2., 3.), 0.5)
    assert (fixed[:, 3:] == np.array([1., 0., 0., 0., 1., 0., 0., 0., -1.])).all()


# ---------------------------------------------------------------- the yardstick
def test_a_standing_camera_is_the_moving_shapes_yardstick_byte_for_byte(pkg, O, orc, Y):
    """An oriented view, every row that view's basis and an offset of +0. or -0.: the samples moving_reference casts from that
    view -- with shapes moving and without."""
    b = RR.basis_tuple(basis(pkg))
    table = PR.lens_sequence(0, 8)
    for name, aperture in (("demo", 0.), ("demo", LR.APERTURE), ("cornell", LR.APERTURE), ("pool", 0.)):
        oscene, eye, kinds = Y.scene(name)[1], Y.eye(name), Y.kinds(name)
        lights = SR.light_sequence(0, 8, (1.5,) * Y.n_lights(name))
        shapes = MR.motion_sequence(0, 8, MV.velocities(kinds, MV.SPEED[name]), MV.SHUTTER)
        for zero in (0., -0.):
            cam = CM.standing_rows(8, b, (zero,) * 3)
            for g in (None, shapes):
                a = CM.samples(O, orc, oscene, eye, 32, 32, 3, aperture, LR.FOCUS, table, cam, lights, g)
                ref = MV.samples(O, orc, oscene, eye, b, 32, 32, 3, aperture, LR.FOCUS, table, lights, np.zeros_like(shapes) if g is None else g)
                assert a.tobytes() == ref.tobytes() and a.any(), name


def test_constant_rows_are_the_view_from_the_moved_camera(pkg, O, orc, Y):
    b = RR.basis_tuple(basis(pkg))
    table, lights = PR.lens_sequence(0, 8), np.zeros((8, Y.n_lights("demo"), 3))
    off = np.array([0.37, -1.1, 2.3])
    eye = np.asarray(Y.eye("demo"), dtype=np.float64)
    a = CM.samples(O, orc, Y.scene("demo")[1], eye, 32, 32, 3, LR.APERTURE, LR.FOCUS, table, CM.standing_rows(8, b, off), lights)
    ref = MV.samples(O, orc, Y.scene("demo")[1], tuple(eye + off), b, 32, 32, 3, LR.APERTURE, LR.FOCUS, table, lights,
                     np.zeros((8, Y.n_shapes("demo"), 3)))
    assert a.tobytes() == ref.tobytes()


@pytest.mark.parametrize("case", sorted(CM.MOTIONS))
def test_the_yardstick_is_not_vacuous(Y, case):
    """Each test motion changes more than 5 % of the pixels of its 32 x 32 frame by more than 0.05: the committed count."""
    n = Y.blurred(case)
    print("    %s: %d pixels differ from the standing camera's frame" % (case, n))
    assert n == CM.BLURRED[case] and n > 0.05 * 1024
