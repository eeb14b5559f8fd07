"""CPU-side checks of the moving spheres (include/rusty_marcher_amd.h, "moving spheres").

1. The three entry points are exported and bound by ctypes, the Rust shim and the C++ mirror with the header's shapes,
   rm_build_info says " motion" and the ABI is still 5, a NULL context is refused with nothing written, and the Python wrappers
   raise before the library is called.
2. rm_motion_sequence is tests/motion_reference.py's numpy restatement bit for bit, and its refusals are returned with their
   text and write nothing.
3. tests/motion_reference.py -- the yardstick of the GPU tests -- is soft_reference.samples when every shape offset is zero,
   moves the sphere centres it says it moves and nothing else, and is not vacuous: the motion frames the GPU tests compare differ
   from the still frames of the same tables in the committed numbers of pixels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lens_reference as LR
import motion_reference as MR
import progressive_reference as PR
import radiance_reference as RR
import soft_reference as SR
import test_rust_binding as RB
import variant_matrix as VM
import workloads

FUNCTIONS = ["rm_motion_sequence", "rm_accumulate_motion_device", "rm_render_progressive_motion"]
D, U8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
VELOCITIES = np.array([[2., -1., 0.5], [0., 0., 0.], [-0.125, 3., -7.]])
SHUTTER = 0.75


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_motion_abi"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return MR.Yardstick(pkg, O, orc)


@pytest.fixture(scope="module")
def matrix(pkg, O, orc):
    return VM.Matrix(pkg, O, orc)


def V3P(pkg, a):
    return a.ctypes.data_as(C.POINTER(pkg._lib.rm_vec3))


# ---------------------------------------------------------------- the ABI
def test_motion_symbols_are_exported_and_bound(pkg, entry):
    L = pkg.lib()
    header = open(os.path.join(entry.ROOT, "include", "rusty_marcher_amd.h")).read()
    lib_py = open(os.path.join(entry.PKG_DIR, "_lib.py")).read()
    for name in FUNCTIONS:
        assert hasattr(L, name), "library does not export %s" % name
        assert name in pkg._lib.SIGNATURES and '"%s"' % name in lib_py
        assert re.search(r"^rm_status %s\(" % name, header, flags=re.M), name
    assert "moving spheres" in header
    for name in ("motion_sequence", "accumulate_motion_device", "render_progressive_motion"):
        assert callable(getattr(pkg.backend.Context, name))
    assert callable(pkg.Renderer.render_progressive_motion) and callable(pkg.Renderer.render_motion_blur)


def test_motion_functions_have_the_header_shapes_in_the_rust_shim_and_the_cpp_mirror(entry):
    c, r = RB.header_functions(), RB.rust_functions()
    for name in FUNCTIONS:
        assert name in c and name in r, name
        assert c[name] == r[name], "%s: header %s, gpu.rs %s" % (name, c[name], r[name])
    assert c["rm_motion_sequence"] == ("i32", ["u32", "u32", "ptr", "u32", "f64", "ptr"])
    assert c["rm_accumulate_motion_device"] == ("i32", ["ptr"] * 5 + ["u32", "ptr", "u32", "u32"] + ["ptr"] * 4)
    assert c["rm_render_progressive_motion"] == ("i32", ["ptr"] * 4 + ["u32", "ptr", "u32", "f64", "i32"] + ["ptr"] * 4)
    text = open(RB.RUST).read()
    assert re.search(r"pub fn render_progressive_motion\(\s*&mut self", text) and "rm_render_progressive_motion(self.ctx" in text
    assert re.search(r"pub fn accumulate_motion\(\s*&mut self", text) and "rm_accumulate_motion_device(self.ctx" in text
    assert "rm_motion_sequence(first, count" in text
    hpp = open(os.path.join(entry.PKG_DIR, "host", "rusty_marcher.hpp")).read()
    assert re.search(r"render_progressive_motion\(framebuffer::FrameBuffer", hpp) and "rm_render_progressive_motion(ctx_" in hpp


def test_cpp_mirror_compiles_with_the_motion_render(entry, tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "rusty_marcher.hpp"\nusing namespace rusty_marcher;\n'
                   'std::string tick(renderer::Renderer &r, framebuffer::FrameBuffer &fb, const scene::Scene &sc) {'
                   ' std::vector<Vec3f> v(sc.shapes.size(), Vec3f{0., 0., 0.}); v[0] = Vec3f{1., 0., 0.5};'
                   ' r.render_progressive_motion(fb, sc, v, 1., 8u); return r.render_progressive_motion(fb, sc, v, 0.5, 8u, {1.5, 0.}, 0.4, 5., true); }\n'
                   'int main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(entry.ROOT, "include"),
                           "-I", os.path.join(entry.PKG_DIR, "host"), str(src)])


def test_build_info_announces_motion(pkg):
    L = pkg.lib()
    assert " motion" in L.rm_build_info().decode() and " soft" in L.rm_build_info().decode()
    assert L.rm_abi_version() == 5


def test_motion_entry_points_refuse_null_context(pkg):
    L, B = pkg.lib(), pkg._lib
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 3)
    lens = B.rm_lens(LR.APERTURE, LR.FOCUS, 4, 0)
    v = np.ascontiguousarray(VELOCITIES)
    frame, bytes8, total = np.full((64, 64, 3), 7.25), np.full((64, 64, 3), 7, np.uint8), C.c_uint32(77)
    assert L.rm_accumulate_motion_device(None, C.byref(p), C.byref(lens), None, None, 2, None, 3, 0, None, None, None, None) == B.RM_ERR_INVALID_ARG
    assert b"NULL ctx" in L.rm_last_error(None)
    assert L.rm_render_progressive_motion(None, C.byref(p), C.byref(lens), None, 0, V3P(pkg, v), 3, 1., 0, frame.ctypes.data_as(D),
                                          bytes8.ctypes.data_as(U8), C.byref(total), None) == B.RM_ERR_INVALID_ARG
    assert b"NULL ctx" in L.rm_last_error(None)
    assert np.all(frame == 7.25) and np.all(bytes8 == 7) and total.value == 77       # nothing written


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
    assert n >= 3 and len(demo.lights) == 2
    good = [pkg.Vec3f(1., 0., 0.5)] + [None] * (n - 1)
    r, fb = pkg.create_renderer(workloads.FOV, 64., 64.), pkg.create_frame_buffer(64, 64)
    # bad velocities: not finite, not vectors, not a sequence
    for bad in ([(nan, 0., 0.)] + [None] * (n - 1), [(0., inf, 0.)] + [None] * (n - 1), [(1., 2.)] + [None] * (n - 1), ["abc"] + [None] * (n - 1),
                1.5, None, "12"):
        with pytest.raises(ValueError):
            K.Context.render_progressive_motion(ctx, p, bad, 1., 0.4, 5., 4)
        with pytest.raises(ValueError):
            K.Context.motion_sequence(ctx, 0, 4, bad, 1.)
        with pytest.raises(ValueError):
            r.render_progressive_motion(fb, demo, bad, 1., 4)
        with pytest.raises(ValueError):
            r.render_motion_blur(fb, demo, bad, 1., 4)
    # a velocity list of the wrong length for the scene: the renderer knows the scene
    for bad in ([], good[:-1], good + [None]):
        with pytest.raises(ValueError, match="one velocity a shape"):
            r.render_progressive_motion(fb, demo, bad, 1., 4)
        with pytest.raises(ValueError, match="one velocity a shape"):
            r.render_motion_blur(fb, demo, bad, 1., 4)
    # the shutter
    for shutter in (-0.1, nan, inf, -inf, "1", None, True):
        with pytest.raises(ValueError, match="shutter"):
            K.Context.render_progressive_motion(ctx, p, good, shutter, 0.4, 5., 4)
        with pytest.raises(ValueError, match="shutter"):
            K.Context.motion_sequence(ctx, 0, 4, good, shutter)
        with pytest.raises(ValueError, match="shutter"):
            r.render_progressive_motion(fb, demo, good, shutter, 4)
    # radii, where given, as the soft wrappers check them
    for radii in ((-0.1, 1.), (nan, 1.), "12", 1.5):
        with pytest.raises(ValueError):
            K.Context.render_progressive_motion(ctx, p, good, 1., 0.4, 5., 4, radii=radii)
        with pytest.raises(ValueError):
            r.render_progressive_motion(fb, demo, good, 1., 4, light_radii=radii)
    with pytest.raises(ValueError, match="one radius a light"):
        r.render_progressive_motion(fb, demo, good, 1., 4, light_radii=(1.5,))
    # the lens, as the progressive wrappers check it
    for aperture, focus, ns in ((-0.1, 5., 4), (nan, 5., 4), (0.4, 0., 4), (0.4, inf, 4), (0.4, 5., 0), (0.4, 5., 65), (0.4, 5., 2.5), (0.4, 5., True)):
        with pytest.raises(ValueError):
            K.Context.render_progressive_motion(ctx, p, good, 1., aperture, focus, ns)
        with pytest.raises(ValueError):
            r.render_progressive_motion(fb, demo, good, 1., ns, aperture=aperture, focus=focus)
    for ns in (0, -1, 65537, 2.5, True):
        with pytest.raises(ValueError):
            r.render_motion_blur(fb, demo, good, 1., ns)
    # bad host buffers: too small; float32; a list; float64 bytes; too small; strided
    for host_rgb, host_rgb8 in ((np.zeros((32, 64, 3)), None), (np.zeros((64, 64, 3), np.float32), None), ([0.] * 12288, None),
                                (None, np.zeros((64, 64, 3))), (None, np.zeros((64, 32, 3), np.uint8)),
                                (np.zeros((64, 64, 6))[:, :, ::2], None)):
        with pytest.raises(ValueError):
            K.Context.render_progressive_motion(ctx, p, good, 1., 0.4, 5., 4, host_rgb=host_rgb, host_rgb8=host_rgb8)
    for first, count in ((-1, 4), (0, -1), (65536, 1), (65473, 64), (0, 65537), (1.5, 1), (0, True)):
        with pytest.raises(ValueError):
            K.Context.motion_sequence(ctx, first, count, good, 1.)
    # the device call: the sum as accumulate_lens_device wants it -- numpy; float32; on the CPU; wrong shape; missing
    t = torch.zeros((64, 64, 3), dtype=torch.float64)
    table, lights, shapes = PR.lens_sequence(0, 4), np.zeros((4, 2, 3)), np.zeros((4, n, 3))
    for s in (np.zeros((64, 64, 3)), t.float(), t, torch.zeros((64, 32, 3), dtype=torch.float64), None):
        with pytest.raises(ValueError):
            K.Context.accumulate_motion_device(ctx, p, s, 0.4, 5., table, lights, shapes, 0)


# ---------------------------------------------------------------- rm_motion_sequence
def library_sequence(pkg, first, count, velocities=VELOCITIES, shutter=SHUTTER):
    v = np.ascontiguousarray(velocities, dtype=np.float64)
    off = np.full((count + 1, len(v), 3), -7.)
    assert pkg.lib().rm_motion_sequence(first, count, V3P(pkg, v), len(v), shutter, off.ctypes.data_as(D)) == 0
    assert np.all(off[count] == -7.)                                  # nothing behind the rows asked for
    return off[:count]


class _NoContext:
    """A Context without an rm_ctx: for the calls that need none."""
    device, ptr = 0, None

    def __init__(self, L):
        self.L = L


def test_motion_sequence_is_the_numpy_restatement_bit_for_bit(pkg):
    for first, count in ((0, 4096), (65472, 64), (1000, 7)):
        got, ref = library_sequence(pkg, first, count), MR.motion_sequence(first, count, VELOCITIES, SHUTTER)
        assert got.shape == (count, 3, 3)
        assert got.tobytes() == ref.tobytes(), "first = %d: rows %s differ" % (first, first + np.flatnonzero((got != ref).any(axis=(1, 2))))
    assert pkg.backend.Context.motion_sequence(_NoContext(pkg.lib()), 1000, 7, VELOCITIES, SHUTTER).tobytes() == \
        MR.motion_sequence(1000, 7, VELOCITIES, SHUTTER).tobytes()
    # a slice is the rows of the whole, wherever it begins
    whole = library_sequence(pkg, 0, 4096)
    assert library_sequence(pkg, 1000, 7).tobytes() == whole[1000:1007].tobytes()
    # row 0 is the scene as uploaded, a velocity of zero gives zeros whatever the row, and every row lies within the shutter
    assert np.all(whole[0] == 0.) and np.all(whole[:, 1] == 0.)
    t = whole[:, 0, 0] / VELOCITIES[0, 0]
    assert t.min() == 0. and 0.74 < t.max() < SHUTTER and len(np.unique(t)) == 4096
    assert np.allclose(whole[:, 2], t[:, None] * VELOCITIES[2][None, :], rtol=1e-15, atol=0.)
    # a shutter of zero is a still frame
    assert np.all(library_sequence(pkg, 0, 64, shutter=0.) == 0.)
    # the integers stay exact, as in rm_lens_sequence: q is a power of 17 just above 65535
    assert PR.digit_reversed(65535, 17)[1] == 17 ** 4 < 2 ** 53


def test_motion_sequence_refusals(pkg):
    L, B = pkg.lib(), pkg._lib
    v = np.array([[2., 0.5, 0.], [0., 1., -1.]])
    off = np.full((65, 2, 3), -7.)
    vp, op = V3P(pkg, v), off.ctypes.data_as(D)
    for first, count in ((65536, 1), (65473, 64), (0, 65537), (2 ** 32 - 1, 2), (2 ** 32 - 1, 2 ** 32 - 1)):
        assert L.rm_motion_sequence(first, count, vp, 2, 1., op) == B.RM_ERR_INVALID_ARG
        assert b"first + count" in L.rm_last_error(None)
    for bad in (float("nan"), float("inf"), -float("inf")):
        for c in range(3):
            w = v.copy()
            w[1, c] = bad
            assert L.rm_motion_sequence(0, 4, V3P(pkg, w), 2, 1., op) == B.RM_ERR_INVALID_ARG
            assert b"velocities[1]" in L.rm_last_error(None)
        assert L.rm_motion_sequence(0, 4, vp, 2, bad, op) == B.RM_ERR_INVALID_ARG and b"shutter" in L.rm_last_error(None)
    assert L.rm_motion_sequence(0, 4, vp, 2, -1e-9, op) == B.RM_ERR_INVALID_ARG and b"shutter" in L.rm_last_error(None)
    assert L.rm_motion_sequence(0, 4, None, 2, 1., op) == B.RM_ERR_INVALID_ARG and b"NULL velocities" in L.rm_last_error(None)
    assert L.rm_motion_sequence(0, 4, vp, 2, 1., None) == B.RM_ERR_INVALID_ARG and b"NULL offsets" in L.rm_last_error(None)
    assert np.all(off == -7.)                                         # nothing written
    # nothing to write: RM_OK, whatever the pointers
    assert L.rm_motion_sequence(12, 0, None, 2, 1., None) == 0 and L.rm_motion_sequence(65536, 0, vp, 2, 1., op) == 0
    assert L.rm_motion_sequence(0, 4, None, 0, 1., None) == 0 and L.rm_motion_sequence(0, 4, vp, 0, 1., op) == 0
    assert np.all(off == -7.)
    assert L.rm_motion_sequence(65535, 1, vp, 2, 1., op) == 0 and np.all(off[1:] == -7.) and not (off[0] == -7.).any()


# ---------------------------------------------------------------- the yardstick
def test_zero_shape_offsets_are_the_soft_yardstick_byte_for_byte(O, orc, Y):
    table = PR.lens_sequence(0, 8)
    for name, aperture in (("demo", 0.), ("demo", LR.APERTURE), ("cornell", LR.APERTURE)):
        oscene, eye = Y.scene(name)[1], Y.eye(name)
        lights = SR.light_sequence(0, 8, (1.5,) * Y.n_lights(name))
        soft = SR.samples(O, orc, oscene, eye, None, 32, 32, 3, aperture, LR.FOCUS, table, lights)
        for zero in (0., -0.):
            motion = MR.samples(O, orc, oscene, eye, None, 32, 32, 3, aperture, LR.FOCUS, table, lights, np.full((8, Y.n_shapes(name), 3), zero))
            assert motion.tobytes() == soft.tobytes(), name
        assert soft.any()
    assert MR.ORC_SPHERE not in Y.kinds("cornell")                    # no sphere: it serves the zero-offset identity only


def test_moved_scene_moves_the_sphere_centres_and_nothing_else(O, orc, Y):
    oscene = Y.scene("penumbra")[1]                                   # a polygon, then a sphere; three lights
    src = oscene.c
    assert Y.kinds("penumbra") == [1, MR.ORC_SPHERE]
    before = C.string_at(src.shapes, C.sizeof(O.Shape) * 2)
    soff = np.array([[5., 5., 5.], [3.5, 0.25, -1.]])                 # (the polygon's row is never read)
    loff = np.array([[-3., 0., 0.], [0.25, -0.5, 1.], [0., 0., 0.]])
    moved = MR.MovedScene(O, oscene, loff, soff)
    assert moved.c.n_lights == src.n_lights == 3 and moved.c.n_shapes == src.n_shapes == 2
    assert C.addressof(moved.c.shapes.contents) != C.addressof(src.shapes.contents)      # a copy of its own
    assert C.string_at(src.shapes, C.sizeof(O.Shape) * 2) == before                      # the source is left alone
    # the polygon: every byte the source's
    assert C.string_at(C.addressof(moved.c.shapes[0]), C.sizeof(O.Shape)) == before[:C.sizeof(O.Shape)]
    # the sphere: the centre moved by one addition a component, every other byte the source's
    a, b = src.shapes[1], moved.c.shapes[1]
    assert a.center.tup() == SR.PENUMBRA_SPHERE[0]
    assert b.center.tup() == tuple(np.array(SR.PENUMBRA_SPHERE[0]) + soff[1])
    back = O.Shape.from_buffer_copy(C.string_at(C.addressof(b), C.sizeof(O.Shape)))
    back.center = O.Vec3(*a.center.tup())
    assert bytes(back) == before[C.sizeof(O.Shape):]
    for l, (pos, _, inten) in enumerate(SR.PENUMBRA_LIGHTS):
        assert moved.c.lights[l].position.tup() == tuple(np.array(pos) + loff[l]) and moved.c.lights[l].intensity == inten
    # A ray down the axis of the view meets the sphere where it stands and misses it once it has moved 3.5 to the right; a ray
    # towards the moved centre meets it there alone.
    L = O.lib()

    def hits_sphere(scene_c, d):
        hit = O.Intersection()
        got = L.orc_find_closest_intersect(O.v3(0., 0., 0.), L.orc_normalized(O.v3(d)), scene_c.shapes, scene_c.n_shapes, C.byref(hit), None)
        return bool(got) and bool(hit.reflectance.is_glass_like)
    assert hits_sphere(src, (0., -2., -9.)) and not hits_sphere(moved.c, (0., -2., -9.))
    assert hits_sphere(moved.c, (3.5, -1.75, -10.)) and not hits_sphere(src, (3.5, -1.75, -10.))
    # ... and the normal of that hit points away from the moved centre
    hit = O.Intersection()
    assert L.orc_find_closest_intersect(O.v3(0., 0., 0.), L.orc_normalized(O.v3(3.5, -1.75, -10.)), moved.c.shapes, 2, C.byref(hit), None)
    n = np.array(hit.point.tup()) - np.array(b.center.tup())
    assert np.allclose(np.array(hit.normal.tup()), n / np.linalg.norm(n), atol=1e-12)


def motion_and_still(Y, name, depth, rows, aperture, focus):
    table = PR.lens_sequence(0, rows)
    lights = np.zeros((rows, Y.n_lights(name), 3))
    shapes = MR.motion_sequence(0, rows, MR.velocities(Y.kinds(name)), MR.SHUTTER)
    _, motion = Y.motion(name, 32, 32, depth, aperture, focus, table, lights, shapes, (rows,))
    _, still = Y.soft(name, 32, 32, depth, aperture, focus, table, lights, (rows,))
    return int((np.abs(motion - still) > 0.05).any(axis=2).sum())


@pytest.mark.parametrize("name", sorted(MR.BLURRED))
def test_motion_frames_are_another_picture_than_still_ones(Y, name):
    """Non-vacuity of the yardstick alone, at the settings the GPU tests use: a pinhole, point lights, shutter 1."""
    depth, rows, pixels = MR.BLURRED[name]
    differ = motion_and_still(Y, name, depth, rows, 0., LR.FOCUS)
    print("%s 32x32, depth %d, %d rows: %d pixels differ from the still frame by more than 0.05" % (name, depth, rows, differ))
    assert differ == pixels and pixels > VM.SHARE * 32 * 32


def test_64_rows_of_the_demo_blur_as_16_do(Y):
    differ = motion_and_still(Y, "demo", 3, 64, 0., LR.FOCUS)
    print("demo 32x32, depth 3, 64 rows: %d pixels differ" % differ)
    assert differ == 433


@pytest.mark.parametrize("cell", VM.CELLS, ids=VM.cell_id)
def test_motion_frames_of_the_matrix_cells_are_another_picture(Y, matrix, cell):
    bvh, generic, depth = cell
    name = VM.register(Y, matrix.name(bvh, generic), matrix.pair(bvh, generic))
    differ = motion_and_still(Y, name, depth, MR.CELL_ROWS, VM.APERTURE, VM.FOCUS)
    print("%s: %d pixels differ from the still frame by more than 0.05" % (VM.cell_id(cell), differ))
    assert differ == MR.BLURRED_CELLS[VM.cell_id(cell)] and differ > VM.SHARE * VM.W * VM.H
    assert 81 <= differ <= 222
