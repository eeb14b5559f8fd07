"""CPU-side checks of the area lights (include/rusty_marcher_amd.h, "area lights").

1. The three entry points are exported and bound by ctypes, the Rust shim and the C++ mirror with the header's shapes,
   rm_build_info says " soft" and the ABI is still 5, a NULL context is refused with nothing written, and the Python wrappers
   raise before the library is called.
2. rm_light_sequence is tests/soft_reference.py's numpy restatement bit for bit, every one of its 65,536 rows lies on its
   light's sphere, and its refusals are returned with their text.
3. tests/soft_reference.py -- the yardstick of the GPU tests -- is progressive_reference.samples when every offset is zero,
   moves the lights it says it moves, and is not vacuous: the soft frames the GPU tests compare differ from the hard-shadow
   frames of the same tables in the committed numbers of pixels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lens_reference as LR
import progressive_reference as PR
import radiance_reference as RR
import soft_reference as SR
import test_rust_binding as RB
import workloads

FUNCTIONS = ["rm_light_sequence", "rm_accumulate_soft_device", "rm_render_progressive_soft"]
D, U8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
RADII = (2., 0.5, 0.)


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_soft_abi"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return SR.Yardstick(pkg, O, orc)


# ---------------------------------------------------------------- the ABI
def test_soft_symbols_are_exported_and_bound(pkg, entry):
    L = pkg.lib()
    header = open(os.path.join(entry.ROOT, "include", "rusty_marcher_amd.h")).read()
    lib_py = open(os.path.join(entry.PKG_DIR, "_lib.py")).read()
    for name in FUNCTIONS:
        assert hasattr(L, name), "library does not export %s" % name
        assert name in pkg._lib.SIGNATURES and '"%s"' % name in lib_py
        assert re.search(r"^rm_status %s\(" % name, header, flags=re.M), name
    assert "area lights" in header
    for name in ("light_sequence", "accumulate_soft_device", "render_progressive_soft"):
        assert callable(getattr(pkg.backend.Context, name))
    assert callable(pkg.Renderer.render_progressive_soft) and callable(pkg.Renderer.render_soft_shadows)


def test_soft_functions_have_the_header_shapes_in_the_rust_shim_and_the_cpp_mirror(entry):
    c, r = RB.header_functions(), RB.rust_functions()
    for name in FUNCTIONS:
        assert name in c and name in r, name
        assert c[name] == r[name], "%s: header %s, gpu.rs %s" % (name, c[name], r[name])
    assert c["rm_light_sequence"] == ("i32", ["u32", "u32", "ptr", "u32", "ptr"])
    assert c["rm_accumulate_soft_device"] == ("i32", ["ptr"] * 5 + ["u32", "u32"] + ["ptr"] * 4)
    assert c["rm_render_progressive_soft"] == ("i32", ["ptr"] * 4 + ["u32", "i32"] + ["ptr"] * 4)
    text = open(RB.RUST).read()
    assert re.search(r"pub fn render_progressive_soft\(\s*&mut self", text) and "rm_render_progressive_soft(self.ctx" in text
    assert re.search(r"pub fn accumulate_soft\(\s*&mut self", text) and "rm_accumulate_soft_device(self.ctx" in text
    assert "rm_light_sequence(first, count" in text
    hpp = open(os.path.join(entry.PKG_DIR, "host", "rusty_marcher.hpp")).read()
    assert re.search(r"render_progressive_soft\(framebuffer::FrameBuffer", hpp) and "rm_render_progressive_soft(ctx_" in hpp


def test_cpp_mirror_compiles_with_the_soft_render(entry, tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "rusty_marcher.hpp"\nusing namespace rusty_marcher;\n'
                   'std::string tick(renderer::Renderer &r, framebuffer::FrameBuffer &fb, const scene::Scene &sc) {'
                   ' r.render_progressive_soft(fb, sc, {1.5, 1.5}, 0.4, 5., 8u); return r.render_progressive_soft(fb, sc, {1.5, 0.}, 0., 5., 8u, true); }\n'
                   'int main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(entry.ROOT, "include"),
                           "-I", os.path.join(entry.PKG_DIR, "host"), str(src)])


def test_build_info_announces_soft(pkg):
    L = pkg.lib()
    assert " soft" in L.rm_build_info().decode() and " progressive" in L.rm_build_info().decode()
    assert L.rm_abi_version() == 5


def test_soft_entry_points_refuse_null_context(pkg):
    L, B = pkg.lib(), pkg._lib
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 3)
    lens = B.rm_lens(LR.APERTURE, LR.FOCUS, 4, 0)
    radii = np.array([1.5, 1.5])
    frame, bytes8, total = np.full((64, 64, 3), 7.25), np.full((64, 64, 3), 7, np.uint8), C.c_uint32(77)
    assert L.rm_accumulate_soft_device(None, C.byref(p), C.byref(lens), None, None, 2, 0, None, None, None, None) == B.RM_ERR_INVALID_ARG
    assert b"NULL ctx" in L.rm_last_error(None)
    assert L.rm_render_progressive_soft(None, C.byref(p), C.byref(lens), radii.ctypes.data_as(D), 2, 0, frame.ctypes.data_as(D),
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
    assert len(demo.lights) == 2
    r, fb = pkg.create_renderer(workloads.FOV, 64., 64.), pkg.create_frame_buffer(64, 64)
    # bad radii: negative, not finite, not numbers, not a sequence, a matrix
    for radii in ((-0.1, 1.), (nan, 1.), (1., inf), (1., -inf), ("a", "b"), 1.5, None, "12", ((1., 1.), (1., 1.))):
        with pytest.raises(ValueError):
            K.Context.render_progressive_soft(ctx, p, radii, 0.4, 5., 4)
        with pytest.raises(ValueError):
            K.Context.light_sequence(ctx, 0, 4, radii)
        with pytest.raises(ValueError):
            r.render_progressive_soft(fb, demo, radii, 0.4, 5., 4)
        with pytest.raises(ValueError):
            r.render_soft_shadows(fb, demo, radii, 4)
    # a radii list of the wrong length for the scene: the renderer knows the scene
    for radii in ((), (1.5,), (1.5, 1.5, 1.5)):
        with pytest.raises(ValueError, match="one radius a light"):
            r.render_progressive_soft(fb, demo, radii, 0.4, 5., 4)
        with pytest.raises(ValueError, match="one radius a light"):
            r.render_soft_shadows(fb, demo, radii, 4)
    # the lens, as the progressive wrappers check it
    for aperture, focus, n in ((-0.1, 5., 4), (nan, 5., 4), (0.4, 0., 4), (0.4, inf, 4), (0.4, 5., 0), (0.4, 5., 65), (0.4, 5., 2.5), (0.4, 5., True)):
        with pytest.raises(ValueError):
            K.Context.render_progressive_soft(ctx, p, (1.5, 1.5), aperture, focus, n)
        with pytest.raises(ValueError):
            r.render_progressive_soft(fb, demo, (1.5, 1.5), aperture, focus, n)
    # bad host buffers: too small; float32; a list; float64 bytes; too small; strided
    for host_rgb, host_rgb8 in ((np.zeros((32, 64, 3)), None), (np.zeros((64, 64, 3), np.float32), None), ([0.] * 12288, None),
                                (None, np.zeros((64, 64, 3))), (None, np.zeros((64, 32, 3), np.uint8)),
                                (np.zeros((64, 64, 6))[:, :, ::2], None)):
        with pytest.raises(ValueError):
            K.Context.render_progressive_soft(ctx, p, (1.5, 1.5), 0.4, 5., 4, host_rgb=host_rgb, host_rgb8=host_rgb8)
    for first, count in ((-1, 4), (0, -1), (65536, 1), (65473, 64), (0, 65537), (1.5, 1), (0, True)):
        with pytest.raises(ValueError):
            K.Context.light_sequence(ctx, first, count, (1.5, 1.5))
    # the device call: the sum as accumulate_lens_device wants it -- numpy; float32; on the CPU; wrong shape; missing
    t = torch.zeros((64, 64, 3), dtype=torch.float64)
    table, offsets = PR.lens_sequence(0, 4), SR.light_sequence(0, 4, (1.5, 1.5))
    for s in (np.zeros((64, 64, 3)), t.float(), t, torch.zeros((64, 32, 3), dtype=torch.float64), None):
        with pytest.raises(ValueError):
            K.Context.accumulate_soft_device(ctx, p, s, 0.4, 5., table, offsets, 0)


# ---------------------------------------------------------------- rm_light_sequence
def library_sequence(pkg, first, count, radii=RADII):
    r = np.ascontiguousarray(radii, dtype=np.float64)
    off = np.full((count + 1, len(r), 3), -7.)
    assert pkg.lib().rm_light_sequence(first, count, r.ctypes.data_as(D), len(r), off.ctypes.data_as(D)) == 0
    assert np.all(off[count] == -7.)                                  # nothing behind the rows asked for
    return off[:count]


class _NoContext:
    """A Context without an rm_ctx: for the calls that need none."""
    device, ptr = 0, None

    def __init__(self, L):
        self.L = L


def test_light_sequence_is_the_numpy_restatement_bit_for_bit(pkg):
    for first, count in ((0, 4096), (65472, 64), (1000, 7)):
        got, ref = library_sequence(pkg, first, count), SR.light_sequence(first, count, RADII)
        assert got.shape == (count, 3, 3)
        assert got.tobytes() == ref.tobytes(), "first = %d: rows %s differ" % (first, first + np.flatnonzero((got != ref).any(axis=(1, 2))))
    assert pkg.backend.Context.light_sequence(_NoContext(pkg.lib()), 1000, 7, RADII).tobytes() == SR.light_sequence(1000, 7, RADII).tobytes()
    # a slice is the rows of the whole, wherever it begins
    whole = library_sequence(pkg, 0, 4096)
    assert library_sequence(pkg, 1000, 7).tobytes() == whole[1000:1007].tobytes()
    # a radius of 0 gives zeros (of either sign), whatever the row
    assert np.all(whole[:, 2] == 0.)
    # row 0 of light 0: phi = 0, a = b = -1, the rim of the disc, the south pole of the sphere
    x, y, z = whole[0, 0]
    assert x == 0. and y == 0. and np.signbit(x) and np.signbit(y) and abs(z + 2.) <= 1e-15
    # lights of one row are shifted against one another: another point for each
    assert not np.allclose(whole[:, 0] / 2., whole[:, 1] / 0.5)
    # the integers stay exact, as in rm_lens_sequence: every q is a power of its base just above 65535
    assert max(PR.digit_reversed(65535, b)[1] for b in (11, 13)) <= 13 ** 5 < 2 ** 53


def test_every_row_of_the_light_sequence_lies_on_its_sphere(pkg):
    off = library_sequence(pkg, 0, 65536)
    for l, r in enumerate(RADII):
        dev = np.abs(np.sqrt((off[:, l] ** 2).sum(axis=1)) - r)
        print("radius %g: | |off| - r | <= %.3e over 65,536 rows" % (r, dev.max()))
        assert dev.max() <= 1e-12 * r
    # ... and the points spread over the whole sphere: every octant is met by the first 64 rows
    octants = {tuple(np.signbit(o)) for o in off[:64, 0] if np.all(o != 0.)}
    assert len(octants) == 8


def test_light_sequence_refusals(pkg):
    L, B = pkg.lib(), pkg._lib
    radii = np.array([2., 0.5])
    off = np.full((65, 2, 3), -7.)
    rp, op = radii.ctypes.data_as(D), off.ctypes.data_as(D)
    for first, count in ((65536, 1), (65473, 64), (0, 65537), (2 ** 32 - 1, 2), (2 ** 32 - 1, 2 ** 32 - 1)):
        assert L.rm_light_sequence(first, count, rp, 2, op) == B.RM_ERR_INVALID_ARG
        assert b"first + count" in L.rm_last_error(None)
    for bad in (-1e-9, float("nan"), float("inf"), -float("inf")):
        r = np.array([2., bad])
        assert L.rm_light_sequence(0, 4, r.ctypes.data_as(D), 2, op) == B.RM_ERR_INVALID_ARG
        assert b"radii[1]" in L.rm_last_error(None)
    assert L.rm_light_sequence(0, 4, None, 2, op) == B.RM_ERR_INVALID_ARG and b"NULL radii" in L.rm_last_error(None)
    assert L.rm_light_sequence(0, 4, rp, 2, None) == B.RM_ERR_INVALID_ARG and b"NULL offsets" in L.rm_last_error(None)
    assert np.all(off == -7.)                                         # nothing written
    # nothing to write: RM_OK, whatever the pointers
    assert L.rm_light_sequence(12, 0, None, 2, None) == 0 and L.rm_light_sequence(65536, 0, rp, 2, op) == 0
    assert L.rm_light_sequence(0, 4, None, 0, None) == 0 and L.rm_light_sequence(0, 4, rp, 0, op) == 0
    assert np.all(off == -7.)
    assert L.rm_light_sequence(65535, 1, rp, 2, op) == 0 and np.all(off[1:] == -7.) and not (off[0] == -7.).any()


# ---------------------------------------------------------------- the yardstick
def test_zero_offsets_are_the_progressive_yardstick_byte_for_byte(O, orc, Y):
    table = PR.lens_sequence(0, 8)
    for name, aperture in (("demo", 0.), ("demo", LR.APERTURE), ("cornell", LR.APERTURE)):
        oscene, eye = Y.scene(name)[1], Y.eye(name)
        hard = PR.samples(orc, oscene, eye, None, 32, 32, 3, aperture, LR.FOCUS, table)
        for zero in (0., -0.):
            soft = SR.samples(O, orc, oscene, eye, None, 32, 32, 3, aperture, LR.FOCUS, table, np.full((8, Y.n_lights(name), 3), zero))
            assert soft.tobytes() == hard.tobytes(), name
        assert hard.any()


def test_moved_scene_moves_the_lights_and_nothing_else(O, orc, Y):
    oscene = Y.scene("penumbra")[1]
    src = oscene.c
    off = np.array([[-3., 0., 0.], [0.25, -0.5, 1.], [0., 0., 0.]])
    moved = SR.moved_scene(O, oscene, off)
    assert moved.c.n_lights == src.n_lights == 3 and moved.c.n_shapes == src.n_shapes == 2
    assert C.addressof(moved.c.shapes.contents) == C.addressof(src.shapes.contents)      # the shapes are the original's
    for l, (pos, _, inten) in enumerate(SR.PENUMBRA_LIGHTS):
        a, b = src.lights[l], moved.c.lights[l]
        assert a.position.tup() == pos                                                   # the source is left alone
        assert b.position.tup() == tuple(np.array(pos) + off[l])
        assert b.color.tup() == a.color.tup() and b.intensity == a.intensity == inten
    # One shadow decision flips.  The floor point below lies beside the hard shadow of the light overhead (the sphere's shadow
    # has a radius of about 2.7 there): lit where the light stands, shadowed with the light moved 3 to the left.
    floor_y = -6. + (-3. - -9.) * 3. / 31.                                               # the floor's height at z = -9
    point = np.array([3.1, floor_y + 0.01, -9.])
    L = O.lib()

    def shadowed(scene_c):
        p = scene_c.lights[0].position
        d = L.orc_normalized(O.v3(p.x - point[0], p.y - point[1], p.z - point[2]))
        return bool(L.orc_intersect_shape_set(O.v3(point), d, scene_c.shapes, scene_c.n_shapes))

    assert not shadowed(src) and shadowed(moved.c)
    # ... and the radiance of the ray from the eye to that point says the same
    d = np.array([point - np.array([0., 0.01, 0.])])
    lit = orc.cast(oscene, np.zeros((1, 3)), d, 3, normalize=True)[0]
    dark = orc.cast(moved, np.zeros((1, 3)), d, 3, normalize=True)[0]
    print("floor point beside the shadow: radiance %s where the light stands, %s with it moved" % (lit, dark))
    assert (lit - dark > 0.1).all()


@pytest.mark.parametrize("name", ["demo", "synthetic256", "penumbra"])
def test_soft_frames_are_another_picture_than_hard_ones(Y, name):
    """Non-vacuity of the yardstick alone, at the settings the GPU tests use: radii 1.5 for every light, aperture 0."""
    depth, rows, pixels = SR.SOFTENED[name]
    table = PR.lens_sequence(0, rows)
    offsets = SR.light_sequence(0, rows, (1.5,) * Y.n_lights(name))
    _, soft = Y.soft(name, 32, 32, depth, 0., LR.FOCUS, table, offsets, (rows,))
    _, hard = Y.progressive(name, 32, 32, depth, 0., LR.FOCUS, table, (rows,))
    differ = int((np.abs(soft - hard) > 0.05).any(axis=2).sum())
    print("%s 32x32, depth %d, %d rows, radii 1.5: %d pixels differ from the hard frame by more than 0.05" % (name, depth, rows, differ))
    assert differ == pixels and pixels >= 16


def test_cornell_shows_no_penumbra_and_serves_the_zero_offset_identity_only(Y):
    """Its lights, at the eye and at (20, 20, 20), throw no penumbra into that view at radii 1.5 or 3 -- so the GPU tests use
    it for the zero-offset identity alone."""
    table = PR.lens_sequence(0, 16)
    _, hard = Y.progressive("cornell", 32, 32, 3, 0., LR.FOCUS, table, (16,))
    for r in (1.5, 3.):
        _, soft = Y.soft("cornell", 32, 32, 3, 0., LR.FOCUS, table, SR.light_sequence(0, 16, (r, r)), (16,))
        assert int((np.abs(soft - hard) > 0.05).any(axis=2).sum()) < 16
