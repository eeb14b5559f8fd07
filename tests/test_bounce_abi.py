"""CPU-side checks of the diffuse bounce (include/rusty_marcher_amd.h, "diffuse bounce").

1. The five entry points are exported and bound by ctypes, the Rust shim and the C++ mirror with the header's shapes,
   rm_build_info says " bounce" and the ABI is still 5, a NULL context is refused with nothing written, and the Python wrappers
   raise before the library is called.
2. rm_bounce_sequence is tests/bounce_reference.py's numpy restatement byte for byte, and its refusals are returned with their
   text.  The new host arithmetic (rm_sampling.cpp) runs stand-alone under the sanitizers.
3. tests/bounce_reference.py -- the yardstick of the GPU tests -- is soft_reference's frame exactly with strength 0, its
   weighted directions are cosine-distributed, and it is not vacuous: the bounce frames the GPU tests compare differ from the
   frames without a bounce in the committed numbers of pixels, and the Cornell box bleeds.
4. What the GPU tests' inputs exercise of steps 2 and 3 (bounce_reference.counters): the fixed-view inputs meet no surface from
   behind; every view of BR.VIEWS holds the committed counters, which meet its conditions, and no ray on a boundary; the edge
   rows put a bouncing sample on every edge of the square, most of them where the radicand is below zero."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bounce_reference as BR
import lens_reference as LR
import progressive_reference as PR
import radiance_reference as RR
import soft_reference as SR
import test_rust_binding as RB
import workloads

FUNCTIONS = ["rm_bounce_sequence", "rm_accumulate_bounce_device", "rm_accumulate_converging_bounce_device", "rm_render_progressive_bounce",
             "rm_render_converging_bounce"]
D, U8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_bounce_abi"))


@pytest.fixture(scope="module")
def Y(pkg, O, entry, orc, tmp_path_factory):
    return BR.Yardstick(pkg, O, orc, BR.compile_helper(O, entry, tmp_path_factory.mktemp("orb_bounce_abi")))


# ---------------------------------------------------------------- the ABI
def test_bounce_symbols_are_exported_and_bound(pkg, entry):
    L = pkg.lib()
    header = open(os.path.join(entry.ROOT, "include", "rusty_marcher_amd.h")).read()
    lib_py = open(os.path.join(entry.PKG_DIR, "_lib.py")).read()
    for name in FUNCTIONS:
        assert hasattr(L, name), "library does not export %s" % name
        assert name in pkg._lib.SIGNATURES and '"%s"' % name in lib_py
        assert re.search(r"^rm_status %s\(" % name, header, flags=re.M), name
    assert "diffuse bounce" in header
    assert callable(pkg.backend.bounce_sequence)
    for name in ("accumulate_bounce_device", "accumulate_converging_bounce_device", "render_progressive_bounce", "render_converging_bounce"):
        assert callable(getattr(pkg.backend.Context, name))
    for name in ("render_progressive_bounce", "render_global_illumination", "render_converging_bounce", "render_converged_bounce"):
        assert callable(getattr(pkg.Renderer, name))


def test_bounce_functions_have_the_header_shapes_in_the_rust_shim_and_the_cpp_mirror(entry):
    c, r = RB.header_functions(), RB.rust_functions()
    for name in FUNCTIONS:
        assert name in c and name in r, name
        assert c[name] == r[name], "%s: header %s, gpu.rs %s" % (name, c[name], r[name])
    assert c["rm_bounce_sequence"] == ("i32", ["u32", "u32", "ptr"])
    assert c["rm_accumulate_bounce_device"] == ("i32", ["ptr"] * 5 + ["u32", "ptr", "f64", "u32"] + ["ptr"] * 4)
    assert c["rm_accumulate_converging_bounce_device"] == ("i32", ["ptr"] * 5 + ["u32", "ptr", "u32", "ptr", "f64", "i32", "ptr", "ptr"])
    assert c["rm_render_progressive_bounce"] == ("i32", ["ptr"] * 4 + ["u32", "f64", "i32"] + ["ptr"] * 4)
    assert c["rm_render_converging_bounce"] == ("i32", ["ptr"] * 5 + ["u32", "f64", "i32"] + ["ptr"] * 4)
    text = open(RB.RUST).read()
    assert re.search(r"pub fn render_progressive_bounce\(\s*&mut self", text) and "rm_render_progressive_bounce(self.ctx" in text
    assert re.search(r"pub fn render_converging_bounce\(\s*&mut self", text) and "rm_render_converging_bounce(self.ctx" in text
    assert "rm_bounce_sequence(first, count" in text
    hpp = open(os.path.join(entry.PKG_DIR, "host", "rusty_marcher.hpp")).read()
    assert re.search(r"render_progressive_bounce\(framebuffer::FrameBuffer", hpp) and "rm_render_progressive_bounce(ctx_" in hpp
    assert re.search(r"render_converging_bounce\(framebuffer::FrameBuffer", hpp) and "rm_render_converging_bounce(ctx_" in hpp


def test_cpp_mirror_compiles_with_the_bounce_renders(entry, tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "rusty_marcher.hpp"\nusing namespace rusty_marcher;\n'
                   'rm_converge_report tick(renderer::Renderer &r, framebuffer::FrameBuffer &fb, const scene::Scene &sc) {'
                   ' r.render_progressive_bounce(fb, sc, 8u); r.render_progressive_bounce(fb, sc, 8u, 0.5, {1.5, 1.5}, 0.4, 5., true);'
                   ' const rm_converge c{0.01, 16u, 1024u};'
                   ' r.render_converging_bounce(fb, sc, c, 8u); return r.render_converging_bounce(fb, sc, c, 8u, 0.5, {1.5, 0.}, 0.4, 5., true); }\n'
                   'int main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(entry.ROOT, "include"),
                           "-I", os.path.join(entry.PKG_DIR, "host"), str(src)])


def test_build_info_announces_bounce(pkg):
    L = pkg.lib()
    assert " bounce" in L.rm_build_info().decode() and " soft" in L.rm_build_info().decode()
    assert L.rm_abi_version() == 5


def test_bounce_entry_points_refuse_null_context(pkg):
    L, B = pkg.lib(), pkg._lib
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 3)
    lens = B.rm_lens(LR.APERTURE, LR.FOCUS, 4, 0)
    conv = B.rm_converge(0.01, 16, 1024)
    frame, bytes8, total = np.full((64, 64, 3), 7.25), np.full((64, 64, 3), 7, np.uint8), C.c_uint32(77)
    report = B.rm_converge_report()
    assert L.rm_accumulate_bounce_device(None, C.byref(p), C.byref(lens), None, None, 2, None, 1., 0, None, None, None, None) == B.RM_ERR_INVALID_ARG
    assert b"NULL ctx" in L.rm_last_error(None)
    assert L.rm_accumulate_converging_bounce_device(None, C.byref(p), C.byref(lens), C.byref(conv), None, 1024, None, 0, None, 1., 1, None,
                                                    None) == B.RM_ERR_INVALID_ARG
    assert b"NULL ctx" in L.rm_last_error(None)
    assert L.rm_render_progressive_bounce(None, C.byref(p), C.byref(lens), None, 0, 1., 0, frame.ctypes.data_as(D), bytes8.ctypes.data_as(U8),
                                          C.byref(total), None) == B.RM_ERR_INVALID_ARG
    assert b"NULL ctx" in L.rm_last_error(None)
    assert L.rm_render_converging_bounce(None, C.byref(p), C.byref(lens), C.byref(conv), None, 0, 1., 0, frame.ctypes.data_as(D),
                                         bytes8.ctypes.data_as(U8), C.byref(report), None) == B.RM_ERR_INVALID_ARG
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
    r, fb = pkg.create_renderer(workloads.FOV, 64., 64.), pkg.create_frame_buffer(64, 64)
    # the strength: negative, not finite, not a number
    for strength in (-1e-9, -1., nan, inf, -inf, "a", None):
        with pytest.raises((ValueError, TypeError)):
            K.Context.render_progressive_bounce(ctx, p, 0., 1., 4, strength)
        with pytest.raises((ValueError, TypeError)):
            K.Context.render_converging_bounce(ctx, p, 0., 1., 4, 0.01, 16, 1024, strength)
        with pytest.raises((ValueError, TypeError)):
            r.render_progressive_bounce(fb, demo, 4, strength)
        with pytest.raises((ValueError, TypeError)):
            r.render_global_illumination(fb, demo, 4, strength)
        with pytest.raises((ValueError, TypeError)):
            r.render_converging_bounce(fb, demo, 0.01, 4, strength)
        with pytest.raises((ValueError, TypeError)):
            r.render_converged_bounce(fb, demo, 0.01, 4, strength)
    # radii of the wrong length for the scene, the lens, the sample numbers
    with pytest.raises(ValueError, match="one radius a light"):
        r.render_progressive_bounce(fb, demo, 4, 1., light_radii=(1.5,))
    for aperture, focus, n in ((-0.1, 5., 4), (0.4, 0., 4), (0.4, 5., 0), (0.4, 5., 65), (0.4, 5., True)):
        with pytest.raises(ValueError):
            K.Context.render_progressive_bounce(ctx, p, aperture, focus, n)
        with pytest.raises(ValueError):
            r.render_converging_bounce(fb, demo, 0.01, n, aperture=aperture, focus=focus)
    for n in (0, 65537, 2.5, True):
        with pytest.raises(ValueError):
            r.render_global_illumination(fb, demo, n)
    for first, count in ((-1, 4), (0, -1), (65536, 1), (65473, 64), (0, 65537), (1.5, 1), (0, True)):
        with pytest.raises(ValueError):
            K.bounce_sequence(first, count)
    # the device call: the sum as accumulate_soft_device wants it, then the bounce table -- a matrix of another shape, NaN
    t = torch.zeros((64, 64, 3), dtype=torch.float64)
    table, offsets, bounce = PR.lens_sequence(0, 4), SR.light_sequence(0, 4, (1.5, 1.5)), BR.bounce_sequence(0, 4)
    for s in (np.zeros((64, 64, 3)), t.float(), t, torch.zeros((64, 32, 3), dtype=torch.float64), None):
        with pytest.raises(ValueError):
            K.Context.accumulate_bounce_device(ctx, p, s, 0.4, 5., table, offsets, bounce, 1., 0)
    for bad in (bounce[:3], np.zeros((4, 3)), np.full((4, 2), nan), torch.zeros((4, 2), dtype=torch.float32)):
        with pytest.raises(ValueError):
            K._bounce_tensor(bad, 4, torch.device("cpu"))


# ---------------------------------------------------------------- rm_bounce_sequence
def library_sequence(pkg, first, count):
    t = np.full((count + 1, 2), -7.)
    assert pkg.lib().rm_bounce_sequence(first, count, t.ctypes.data_as(D)) == 0
    assert np.all(t[count] == -7.)                                    # nothing behind the rows asked for
    return t[:count]


def test_bounce_sequence_is_the_numpy_restatement_byte_for_byte(pkg):
    for first, count in ((0, 200), (1000, 7), (65472, 64)):
        got, ref = library_sequence(pkg, first, count), BR.bounce_sequence(first, count)
        assert got.shape == (count, 2)
        assert got.tobytes() == ref.tobytes(), "first = %d: rows %s differ" % (first, first + np.flatnonzero((got != ref).any(axis=1)))
    assert pkg.backend.bounce_sequence(1000, 7).tobytes() == BR.bounce_sequence(1000, 7).tobytes()
    whole = library_sequence(pkg, 0, 4096)
    assert library_sequence(pkg, 1000, 7).tobytes() == whole[1000:1007].tobytes()     # a slice is the rows of the whole
    assert whole[0].tolist() == [0., 0.] and whole[1].tolist() == [1. / 19., 1. / 23.]
    assert (whole >= 0.).all() and (whole < 1.).all()
    # the bases are the sequence's own: 2, 3, 5, 7 are the lens table's, 11 and 13 the lights', 17 the shutter's
    assert len({tuple(r) for r in whole}) == 4096
    # the integers stay exact: every q is a power of its base just above 65535
    assert max(PR.digit_reversed(65535, b)[1] for b in (19, 23)) <= 23 ** 4 < 2 ** 53


def test_bounce_sequence_refusals(pkg):
    L, B = pkg.lib(), pkg._lib
    t = np.full((65, 2), -7.)
    tp = t.ctypes.data_as(D)
    for first, count in ((65536, 1), (65473, 64), (0, 65537), (2 ** 32 - 1, 2), (2 ** 32 - 1, 2 ** 32 - 1)):
        assert L.rm_bounce_sequence(first, count, tp) == B.RM_ERR_INVALID_ARG
        assert b"first + count" in L.rm_last_error(None)
    assert L.rm_bounce_sequence(0, 4, None) == B.RM_ERR_INVALID_ARG and b"NULL table" in L.rm_last_error(None)
    assert np.all(t == -7.)                                           # nothing written
    assert L.rm_bounce_sequence(12, 0, None) == 0 and L.rm_bounce_sequence(65536, 0, tp) == 0
    assert np.all(t == -7.)
    assert L.rm_bounce_sequence(65535, 1, tp) == 0 and np.all(t[1:] == -7.) and not (t[0] == -7.).any()


def test_new_host_arithmetic_under_asan_ubsan(entry, tmp_path):
    """rm_bounce_sequence, the strength's check, the identity and the staging rule, stand-alone: nothing loaded into Python
    runs under a sanitizer."""
    exe = tmp_path / "bounce_sampling"
    subprocess.check_call([
        "g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
        "-I", os.path.join(entry.ROOT, "include"), "-I", os.path.join(entry.PKG_DIR, "csrc"),
        os.path.join(entry.PKG_DIR, "csrc", "rm_sampling.cpp"), os.path.join(entry.ROOT, "tests", "native", "bounce_sampling_main.cpp"),
        "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([str(exe)], capture_output=True, env=env)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert b"bounce sampling ok" in out.stdout


# ---------------------------------------------------------------- the yardstick
def test_the_hash_is_lowbias32():
    """Known answers worked out by hand from the header's five lines (Python integers, mod 2^32)."""
    def by_hand(h):
        h ^= h >> 16
        h = h * 0x7feb352d % 2 ** 32
        h ^= h >> 15
        h = h * 0x846ca68b % 2 ** 32
        h ^= h >> 16
        return h
    pix = np.array([0, 1, 2, 31, 32, 1023, 65535, 65536, 1920 * 1056 - 1, 2 ** 31 - 1], dtype=np.uint32)
    assert BR.lowbias32(pix).tolist() == [by_hand(int(v)) for v in pix]
    assert by_hand(0) == 0 and len(set(BR.lowbias32(np.arange(4096)).tolist())) == 4096
    # neighbouring pixels do not share a shift
    x, y = BR.shifted(0.25, 0.75, np.arange(1024, dtype=np.uint32))
    assert len({(a, b) for a, b in zip(x.tolist(), y.tolist())}) == 1024 and (x >= 0.).all() and (x < 1.).all() and (y >= 0.).all() and (y < 1.).all()
    x0, y0 = BR.shifted(0.25, 0.75, np.arange(1024, dtype=np.uint32), shift=False)
    assert np.all(x0 == 0.25) and np.all(y0 == 0.75)


def test_the_weighted_directions_are_cosine_distributed():
    """4,096 rows of the sequence, without a shift and under the shifts of eight pixels: the mean of k is 1 (the weights are a
    density), of k w 2/3 and of k u u 1/4 (the moments of the cosine lobe).  The tolerance is the quasi-Monte-Carlo error of these
    bases at this count, measured here: 1.0e-4, 4.0e-5 and 1.6e-4 without a shift, at most 4.7e-4, 1.06e-3 and 9.9e-4 under the
    eight shifts -- 2e-3 is twice the worst of them; a map that is off (the weight left out: the mean of w is then 0.70) misses
    it by an order of magnitude."""
    t = BR.bounce_sequence(0, 4096)
    worst = np.zeros(3)
    for pix in (None, 0, 1, 31, 32, 1023, 2047, 65535, 1920 * 1056 - 1):
        x, y = (t[:, 0], t[:, 1]) if pix is None else BR.shifted(t[:, 0], t[:, 1], np.full(4096, pix, dtype=np.uint32))
        u, v, w, k = BR.disc(x, y)
        assert (k >= 0.).all() and (k <= BR.FOUR_OVER_PI).all() and (u * u + v * v <= 1. + 4e-16).all()   # (the rim rounds to 1 + an ulp: step 2's fmax)
        err = np.abs([k.mean() - 1., (k * w).mean() - 2. / 3., (k * u * u).mean() - 0.25])
        worst = np.maximum(worst, err)
        assert abs(w.mean() - 2. / 3.) > 0.02                         # the map alone is not the cosine lobe: the weight is needed
    print("QMC error over 4,096 rows: mean k %.2e, k w %.2e, k u u %.2e" % tuple(worst))
    assert (worst < 2e-3).all()


def test_the_frame_of_step_3_is_orthonormal_and_faces_the_ray():
    rng = np.random.default_rng(20262101)
    N = rng.normal(size=(512, 3))
    N /= np.linalg.norm(N, axis=1)[:, None]
    N[:6] = [(0., 0., 1.), (0., 0., -1.), (1., 0., 0.), (0., -1., 0.), (0., 1e-9, -1.), (1e-9, 0., 1.)]
    N[:6] /= np.linalg.norm(N[:6], axis=1)[:, None]
    dirs = rng.normal(size=(512, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    P = rng.uniform(-5., 5., (512, 3))
    x, y = rng.uniform(0., 1., 512), rng.uniform(0., 1., 512)
    u, v, w, _ = BR.disc(x, y)
    origin, omega = BR.bounce_ray(P, N, dirs, u, v, w)
    Nf = np.where(((dirs * N).sum(axis=1) < 0.)[:, None], N, -N)
    assert ((dirs * Nf).sum(axis=1) <= 0.).all()
    assert np.abs(np.linalg.norm(omega, axis=1) - 1.).max() < 1e-12   # T, B, Nf orthonormal and u^2 + v^2 + w^2 = 1
    assert np.abs((omega * Nf).sum(axis=1) - w).max() < 1e-12          # the cosine to the facing normal is w
    assert ((omega * Nf).sum(axis=1) >= -1e-12).all()
    assert np.abs(origin - (P + Nf * 1e-3)).max() == 0.


def test_strength_zero_is_the_soft_yardstick_exactly(O, orc, Y):
    table, bounce = PR.lens_sequence(0, 8), BR.bounce_sequence(0, 8)
    for name, aperture in (("demo", 0.), ("demo", LR.APERTURE), ("cornell", LR.APERTURE), ("penumbra", 0.)):
        offsets = SR.light_sequence(0, 8, (1.5,) * Y.n_lights(name))
        oscene, eye = Y.scene(name)[1], Y.eye(name)
        soft = SR.samples(O, orc, oscene, eye, None, 32, 32, 3, aperture, LR.FOCUS, table, offsets)
        zero = BR.samples(O, Y.orb, oscene, eye, None, 32, 32, 3, aperture, LR.FOCUS, table, offsets, bounce, 0.)
        assert zero.tobytes() == soft.tobytes(), name
        assert soft.any()
        one = BR.samples(O, Y.orb, oscene, eye, None, 32, 32, 3, aperture, LR.FOCUS, table, offsets, bounce, 1.)
        assert (one >= soft).all() and (one > soft).any()              # light is only added
    # ... and without a depth there is nothing to bounce from
    flat = BR.samples(O, Y.orb, Y.scene("demo")[1], Y.eye("demo"), None, 32, 32, 0, 0., LR.FOCUS, table, None, bounce, 1.)
    assert np.all(flat == np.array(RR.BACKGROUND))


@pytest.mark.parametrize("name", sorted(BR.BOUNCED))
def test_bounce_frames_are_another_picture(Y, name):
    """Non-vacuity of the yardstick alone, at the settings the GPU tests use: strength 1, aperture 0, point lights."""
    depth, rows, pixels = BR.BOUNCED[name]
    table, bounce = PR.lens_sequence(0, rows), BR.bounce_sequence(0, rows)
    _, lit = Y.bounce(name, 32, 32, depth, 0., LR.FOCUS, table, None, bounce, 1., (rows,))
    _, plain = Y.progressive(name, 32, 32, depth, 0., LR.FOCUS, table, (rows,))
    differ = int((np.abs(lit - plain) > 0.05).any(axis=2).sum())
    print("%s 32x32, depth %d, %d rows, strength 1: %d pixels differ from the frame without a bounce by more than 0.05" % (name, depth, rows, differ))
    assert differ == pixels and pixels > 0
    # ... and the per-pixel shift matters: the frame without it is a third picture
    _, unshifted = Y.bounce(name, 32, 32, depth, 0., LR.FOCUS, table, None, bounce, 1., (rows,), shift=False)
    assert np.abs(unshifted - lit).max() > 0.01


def test_the_cornell_box_bleeds(Y):
    """A pixel whose channel ratios differ from the no-bounce frame's: the bounce brings in another surface's colour, it does
    not merely brighten."""
    depth, rows, _ = BR.BOUNCED["cornell"]
    table, bounce = PR.lens_sequence(0, rows), BR.bounce_sequence(0, rows)
    _, lit = Y.bounce("cornell", 32, 32, depth, 0., LR.FOCUS, table, None, bounce, 1., (rows,))
    _, plain = Y.progressive("cornell", 32, 32, depth, 0., LR.FOCUS, table, (rows,))
    seen = plain.sum(axis=2) > 0.2
    ratio = lambda f: f / np.where(seen, f.sum(axis=2), 1.)[..., None]
    shift = np.where(seen, np.abs(ratio(lit) - ratio(plain)).max(axis=2), 0.)
    y, x = np.unravel_index(shift.argmax(), shift.shape)
    print("cornell pixel (%d, %d): channel ratios %s without, %s with the bounce" % (x, y, ratio(plain)[y, x], ratio(lit)[y, x]))
    assert shift.max() > 0.01


def test_the_parity_inputs_hold_no_ray_on_a_hit_miss_boundary(O, Y):
    """The first rows the GPU parity tests use (tests/test_gpu_bounce.py: rows from FIRST on): no sample changes when its bounce
    direction is moved one ulp, so a deviation there is the arithmetic's and not a decision's."""
    import test_gpu_bounce as GB
    for name, depth in sorted(GB.SCENES.items()):
        table, bounce = PR.lens_sequence(GB.FIRST, 5), BR.bounce_sequence(GB.FIRST, 5)
        n = BR.boundary_rays(O, Y.orb, Y.scene(name)[1], Y.eye(name), None, 32, 32, depth, 0., LR.FOCUS, table, None, bounce, 1.)
        assert n == 0, "%s: %d samples sit on a boundary" % (name, n)


@pytest.mark.parametrize("name", sorted(BR.REQUIRED))
def test_the_views_hold_no_ray_on_a_hit_miss_boundary(pkg, O, Y, name):
    """... nor do the views from every side, under either of their tables, through the pinhole and through the lens."""
    import test_gpu_bounce as GB
    scene, depth, view, focus, _ = GB.host_view(pkg, Y, name)
    eye, basis = (Y.eye(scene), None) if view is None else view
    table = PR.lens_sequence(GB.FIRST, 5)
    for what, bounce in BR.view_tables(name, GB.FIRST, 5):
        for aperture in (0., LR.APERTURE):
            n = BR.boundary_rays(O, Y.orb, Y.scene(scene)[1], eye, basis, 32, 32, depth, aperture, focus, table, None, bounce, 1.)
            assert n == 0, "%s, %s table, aperture %g: %d samples sit on a boundary" % (name, what, aperture, n)
    if name in BR.CONVERGING_VIEWS:                                    # the converging case's rows: the library's first 15
        for aperture in (0., LR.APERTURE):
            n = BR.boundary_rays(O, Y.orb, Y.scene(scene)[1], eye, basis, 32, 32, depth, aperture, focus, PR.lens_sequence(0, 15), None,
                                 BR.bounce_sequence(0, 15), 1.)
            assert n == 0, "%s, rows 0 .. 14, aperture %g: %d samples sit on a boundary" % (name, aperture, n)


# ---------------------------------------------------------------- what the inputs exercise of steps 2 and 3
def pinned(c):
    return tuple(c[key] for key in BR.PINNED)


def test_the_fixed_view_inputs_meet_no_surface_from_behind(Y):
    """The five inputs the parity tests had before the views (5 rows from FIRST, aperture 0): not one sample takes Nf = -N, the
    Cornell box shows one orientation, and the sg = -1 half of the basis runs on a few dozen samples far from its pole."""
    import test_gpu_bounce as GB
    table, bounce = PR.lens_sequence(GB.FIRST, 5), BR.bounce_sequence(GB.FIRST, 5)
    for name, want in sorted(BR.FIXED_COVERAGE.items()):
        c = Y.counters(name, 32, 32, dict(GB.SCENES, floor=3)[name], 0., LR.FOCUS, table, None, bounce, 1.)
        print("%s, fixed view: %s" % (name, c))
        assert pinned(c) == want and c["back"] == 0 and c["front"] == c["bouncing"], name
        assert c["negative"] == 0 and c["edge"] == 0 and c["min_z"] > -0.46
    assert Y.counters("demo", 32, 32, 3, 0., LR.FOCUS, table, None, bounce, 0.)["bouncing"] == 0    # (no strength: nothing bounces)


@pytest.mark.parametrize("name", sorted(BR.REQUIRED))
def test_a_view_exercises_what_it_is_there_for(pkg, Y, name):
    """The counters of every view's parity inputs, by the oracle alone under the library's host look-at: the committed numbers,
    which meet the view's conditions; light comes back; and the frame is another picture than the fixed view's."""
    import test_gpu_bounce as GB
    scene, depth, view, focus, _ = GB.host_view(pkg, Y, name)
    table = PR.lens_sequence(GB.FIRST, 5)
    for what, bounce in BR.view_tables(name, GB.FIRST, 5):
        c = Y.counters(scene, 32, 32, depth, 0., focus, table, None, bounce, 1., view)
        print("%s, %s table: %s" % (name, what, c))
        assert pinned(c) == BR.COVERAGE[name]
        BR.assert_covers(name, c)
        assert c["front"] + c["back"] == c["bouncing"] and c["negative"] == 0
        lit = Y.bounce(scene, 32, 32, depth, 0., focus, table, None, bounce, 1., (5,), view)[1]
        plain = Y.bounce(scene, 32, 32, depth, 0., focus, table, None, bounce, 0., (5,), view)[1]
        assert (np.abs(lit - plain) > 0.05).any(axis=2).sum() > 20
        if view is not None:
            assert np.abs(lit - Y.bounce(scene, 32, 32, depth, 0., focus, table, None, bounce, 1., (5,))[1]).max() > 0.05


def test_every_pixels_shift_can_be_cancelled():
    """BR.edge_coordinate: x == 0 is within reach of every pixel of a 32 x 32 frame by a table entry of [0, 1), 1 - 2^-53 of
    those whose shift is below a half (from there on the sum rounds to 1 and wraps to 0)."""
    h = BR.lowbias32(np.arange(1024, dtype=np.uint32))
    for shift16 in sorted(set((h & np.uint32(0xffff)).tolist() + (h >> np.uint32(16)).tolist() + [0, 1, 32768, 32769, 65535])):
        near, far = BR.edge_coordinate(shift16, False), BR.edge_coordinate(shift16, True)
        assert near is not None and 0. <= near < 1. and near == (1. - shift16 / 65536.) % 1.
        assert (far is not None) == (shift16 < 32768), shift16
        assert far is None or (0. <= far < 1. and far == np.nextafter(near if near > 0. else 1., 0.))
    # the clamp is needed there: without it the yardstick's own w is NaN
    x, y = np.zeros(4096), np.random.default_rng(5).uniform(0., 1., 4096)
    r = BR.disc_unclamped(x, y)[2]
    assert 0.05 < (r < 0.).mean() < 0.3 and r.min() > -1e-15 and not np.isnan(BR.disc(x, y)[2]).any()
    with np.errstate(invalid="ignore"):
        assert np.isnan(np.sqrt(r)).any()


@pytest.mark.parametrize("name", BR.EDGE_VIEWS)
def test_the_edge_rows_put_a_bouncing_sample_on_every_edge(pkg, O, Y, name):
    """The edge cases' tables (tests/test_gpu_bounce.py): every row's target bounces and sits where the row's kind says, the
    counters meet the case's conditions, and no sample is on a hit / miss boundary."""
    import test_gpu_bounce as GB
    scene, depth, view, focus, _ = GB.host_view(pkg, Y, name)
    eye, basis = (Y.eye(scene), None) if view is None else view
    n = len(BR.EDGE_KINDS)
    table = PR.lens_sequence(GB.FIRST, n)
    bouncing = Y.bouncing_pixels(scene, 32, 32, 0., focus, table, view)
    bounce, targets = BR.edge_table(np.random.default_rng(BR.EDGE_SEED), bouncing, BR.EDGE_KINDS)
    assert bounce.shape == (n, 2) and n <= 64 and (bounce >= 0.).all() and (bounce < 1.).all()
    at = {"x_lo": (0, 0.), "x_hi": (0, BR.ONE_BELOW), "y_lo": (1, 0.), "y_hi": (1, BR.ONE_BELOW)}
    for s, (kind, p) in enumerate(zip(BR.EDGE_KINDS, targets)):
        xy = BR.shifted(bounce[s, 0], bounce[s, 1], np.array([p], dtype=np.uint32))
        assert bouncing[p, s] and all(xy[at[e][0]][0] == at[e][1] for e in kind.split("+")), (s, kind, p)
        assert "+" in kind or BR.disc_unclamped(*xy)[2][0] < 0.
    c = Y.counters(scene, 32, 32, depth, 0., focus, table, None, bounce, 1., view)
    print("%s, %d edge rows: %s" % (name, n, c))
    BR.assert_edges(c)
    assert (c["edge"], c["corner"], c["negative"]) == (24, 8, 20) and [c[e] for e in BR.EDGES] == [8, 8, 8, 8]
    assert BR.boundary_rays(O, Y.orb, Y.scene(scene)[1], eye, basis, 32, 32, depth, 0., focus, table, None, bounce, 1.) == 0
