"""CPU-side checks of the converging frames (include/rusty_marcher_amd.h, "converging frames").

1. The three entry points are exported and bound by ctypes, the Rust shim and the C++ mirror with the header's shapes, the
   structs have the header's sizes, rm_build_info says " converge" and the ABI is still 5, the workspace is
   rm_refine_workspace's, a NULL context is refused with nothing written, and the Python wrappers raise before the library is
   called.
2. tests/converge_reference.py -- the yardstick of the GPU tests -- has the properties the header states: tolerance < 0 lists
   everything, a pixel of identical samples settles at min_samples, the neighbour rule and the cap hold, and a pixel's sum at
   its count is the plain run's left fold.
3. The cases the GPU tests use are not vacuous and no decision in them is close: the committed numbers of passes, samples and
   distinct counts, counted with the oracle alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import converge_reference as CR
import lens_reference as LR
import progressive_reference as PR
import radiance_reference as RR
import soft_reference as SR
import test_rust_binding as RB
import workloads

FUNCTIONS = ["rm_converge_workspace", "rm_accumulate_converging_device", "rm_render_converging"]
D, U8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_converge_abi"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return CR.Yardstick(pkg, O, orc)


# ---------------------------------------------------------------- the ABI
def test_converge_symbols_are_exported_and_bound(pkg, entry):
    L = pkg.lib()
    header = open(os.path.join(entry.ROOT, "include", "rusty_marcher_amd.h")).read()
    lib_py = open(os.path.join(entry.PKG_DIR, "_lib.py")).read()
    for name in FUNCTIONS:
        assert hasattr(L, name), "library does not export %s" % name
        assert name in pkg._lib.SIGNATURES and '"%s"' % name in lib_py
        assert re.search(r"^rm_status %s\(" % name, header, flags=re.M), name
    assert "converging frames" in header
    for name in ("converge_workspace", "accumulate_converging_device", "render_converging"):
        assert callable(getattr(pkg.backend.Context, name))
    assert callable(pkg.Renderer.render_converging) and callable(pkg.Renderer.render_converged)


def test_converge_functions_have_the_header_shapes_in_the_rust_shim_and_the_cpp_mirror(entry):
    c, r = RB.header_functions(), RB.rust_functions()
    for name in FUNCTIONS:
        assert name in c and name in r, name
        assert c[name] == r[name], "%s: header %s, gpu.rs %s" % (name, c[name], r[name])
    assert c["rm_converge_workspace"] == ("i32", ["ptr", "ptr"])
    assert c["rm_accumulate_converging_device"] == ("i32", ["ptr"] * 5 + ["u32", "ptr", "u32", "i32", "ptr", "ptr"])
    assert c["rm_render_converging"] == ("i32", ["ptr"] * 5 + ["u32", "i32"] + ["ptr"] * 4)
    text = open(RB.RUST).read()
    assert re.search(r"pub fn render_converging\(\s*&mut self", text) and "rm_render_converging(self.ctx" in text
    assert re.search(r"pub fn accumulate_converging\(\s*&mut self", text) and "rm_accumulate_converging_device(self.ctx" in text
    assert "rm_converge_workspace(&p" in text
    for struct, fields in (("RmConverge", ("tolerance: f64", "min_samples: u32", "max_samples: u32")),
                           ("RmConvergeFrame", ("sum:", "stats:", "count:", "workspace:", "mean:", "rgb8:", "mask:")),
                           ("RmConvergeReport", ("samples_cast: u64", "listed: u32", "passes: u32", "max_count: u32", "_pad: u32"))):
        body = re.search(r"pub struct %s \{(.*?)\}" % struct, text, flags=re.S).group(1)
        at = [body.index(f) for f in fields]                          # every field, in the header's order
        assert at == sorted(at), struct
    hpp = open(os.path.join(entry.PKG_DIR, "host", "rusty_marcher.hpp")).read()
    assert re.search(r"render_converging\(framebuffer::FrameBuffer", hpp) and "rm_render_converging(ctx_" in hpp


def test_structs_have_the_header_sizes(pkg, entry, tmp_path):
    B = pkg._lib
    assert (C.sizeof(B.rm_converge), C.sizeof(B.rm_converge_frame), C.sizeof(B.rm_converge_report)) == (16, 56, 24)
    assert B.rm_converge.max_samples.offset == 12 and B.rm_converge_report.listed.offset == 8
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include "rusty_marcher_amd.h"\n'
                   '_Static_assert(sizeof(rm_converge) == 16 && offsetof(rm_converge, min_samples) == 8, "rm_converge");\n'
                   '_Static_assert(sizeof(rm_converge_frame) == 56 && offsetof(rm_converge_frame, mean) == 32, "rm_converge_frame");\n'
                   '_Static_assert(sizeof(rm_converge_report) == 24 && offsetof(rm_converge_report, max_count) == 16, "rm_converge_report");\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(entry.ROOT, "include"), str(src)])


def test_cpp_mirror_compiles_with_the_converging_render(entry, tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "rusty_marcher.hpp"\nusing namespace rusty_marcher;\n'
                   'unsigned tick(renderer::Renderer &r, framebuffer::FrameBuffer &fb, const scene::Scene &sc) {'
                   ' const rm_converge c{0.01, 16u, 1024u};'
                   ' r.render_converging(fb, sc, c, 8u); r.render_converging(fb, sc, c, 8u, {1.5, 1.5}, 0.4, 5., true);'
                   ' return r.last_report.listed + r.last_samples; }\n'
                   'int main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(entry.ROOT, "include"),
                           "-I", os.path.join(entry.PKG_DIR, "host"), str(src)])


def test_build_info_announces_converge(pkg):
    L = pkg.lib()
    info = L.rm_build_info().decode()
    assert info.endswith(" converge") and " soft" in info and " progressive" in info
    assert L.rm_abi_version() == 5


def test_workspace_is_the_refine_workspace(pkg):
    L, B = pkg.lib(), pkg._lib
    for h, w in ((32, 32), (40, 32), (1056, 1920), (31, 64)):
        p = pkg.backend.make_params(workloads.FOV, float(h), float(w), 3)
        a, b = C.c_size_t(7), C.c_size_t(9)
        assert L.rm_converge_workspace(C.byref(p), C.byref(a)) == 0 and L.rm_refine_workspace(C.byref(p), C.byref(b)) == 0
        assert a.value == b.value == (4 * (1 + (h - h % 32) * w) + 255) // 256 * 256
    odd = pkg.backend.make_params(workloads.FOV, 64., 100., 3)
    a = C.c_size_t(7)
    assert L.rm_converge_workspace(C.byref(odd), C.byref(a)) == B.RM_ERR_DIMENSIONS and a.value == 7
    assert L.rm_converge_workspace(None, C.byref(a)) == B.RM_ERR_INVALID_ARG and L.rm_converge_workspace(C.byref(odd), None) == B.RM_ERR_INVALID_ARG


def test_converge_entry_points_refuse_null_context(pkg):
    L, B = pkg.lib(), pkg._lib
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 3)
    lens, conv = B.rm_lens(LR.APERTURE, LR.FOCUS, 4, 0), B.rm_converge(0.01, 16, 64)
    frame, bytes8 = np.full((64, 64, 3), 7.25), np.full((64, 64, 3), 7, np.uint8)
    report = B.rm_converge_report(77, 77, 77, 77, 0)
    buffers = B.rm_converge_frame()
    assert L.rm_accumulate_converging_device(None, C.byref(p), C.byref(lens), C.byref(conv), None, 64, None, 0, 1, C.byref(buffers),
                                             None) == B.RM_ERR_INVALID_ARG
    assert b"NULL ctx" in L.rm_last_error(None)
    assert L.rm_render_converging(None, C.byref(p), C.byref(lens), C.byref(conv), None, 0, 0, frame.ctypes.data_as(D), bytes8.ctypes.data_as(U8),
                                  C.byref(report), None) == B.RM_ERR_INVALID_ARG
    assert b"NULL ctx" in L.rm_last_error(None)
    assert np.all(frame == 7.25) and np.all(bytes8 == 7)               # nothing written
    assert (report.samples_cast, report.listed, report.passes, report.max_count) == (77, 77, 77, 77)


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
    # rm_converge: a NaN tolerance; sample numbers that are no integers, negative, or out of order with n_samples and the cap
    for tol, lo, hi in ((nan, 16, 64), (0.01, -1, 64), (0.01, 1.5, 64), (0.01, True, 64), (0.01, 16, 7), (0.01, 16, 65537), (0.01, 16, 64.5),
                        (0.01, 16, None), (0.01, 2 ** 32, 64)):
        with pytest.raises((ValueError, TypeError)):
            K.Context.render_converging(ctx, p, 0.4, 5., 8, tol, lo, hi)
        with pytest.raises((ValueError, TypeError)):
            r.render_converging(fb, demo, tol, 8, lo, hi)
        with pytest.raises((ValueError, TypeError)):
            r.render_converged(fb, demo, tol, 8, lo, hi)
    K._converge(-1., 0, 8, 8), K._converge(inf, 16, 65536, 64)          # what is allowed: any tolerance but NaN, the whole range
    # the lens and the radii, as the progressive wrappers check them
    for aperture, focus, n in ((-0.1, 5., 4), (nan, 5., 4), (0.4, 0., 4), (0.4, inf, 4), (0.4, 5., 0), (0.4, 5., 65), (0.4, 5., 2.5), (0.4, 5., True)):
        with pytest.raises(ValueError):
            K.Context.render_converging(ctx, p, aperture, focus, n, 0.01, 16, 1024)
        with pytest.raises(ValueError):
            r.render_converging(fb, demo, 0.01, n, aperture=aperture, focus=focus)
    for radii in ((-0.1, 1.), (nan, 1.), (1., inf), ("a", "b"), 1.5, "12", ((1., 1.), (1., 1.))):
        with pytest.raises(ValueError):
            K.Context.render_converging(ctx, p, 0.4, 5., 8, 0.01, 16, 1024, radii=radii)
        with pytest.raises(ValueError):
            r.render_converging(fb, demo, 0.01, 8, light_radii=radii)
    for radii in ((), (1.5,), (1.5, 1.5, 1.5)):
        with pytest.raises(ValueError, match="one radius a light"):
            r.render_converging(fb, demo, 0.01, 8, light_radii=radii)
    # bad host buffers: too small; float32; a list; float64 bytes; strided
    for host_rgb, host_rgb8 in ((np.zeros((32, 64, 3)), None), (np.zeros((64, 64, 3), np.float32), None), ([0.] * 12288, None),
                                (None, np.zeros((64, 64, 3))), (np.zeros((64, 64, 6))[:, :, ::2], None)):
        with pytest.raises(ValueError):
            K.Context.render_converging(ctx, p, 0.4, 5., 8, 0.01, 16, 1024, host_rgb=host_rgb, host_rgb8=host_rgb8)
    # the device call: every buffer -- numpy; another dtype; on the CPU; another shape; missing -- before anything else
    table = PR.lens_sequence(0, 64)
    good = dict(sum=torch.zeros((64, 64, 3), dtype=torch.float64), stats=torch.zeros((64, 64, 2), dtype=torch.float64),
                count=torch.zeros((64, 64), dtype=torch.int32))
    for name in good:
        t = good[name]
        for bad in (t.numpy(), t.to(torch.float32), t, t[:32].contiguous(), None):
            args = dict(good)
            args[name] = bad
            with pytest.raises(ValueError):
                K.Context.accumulate_converging_device(ctx, p, args["sum"], args["stats"], args["count"], 0.4, 5., 8, table, 0.01, 16, 64, True)


# ---------------------------------------------------------------- the reference's properties
def synthetic(rng, pixels, rows, flat=()):
    """Samples [pixel][row][3] of noise; the pixels `flat` hold one value in every row."""
    s = rng.uniform(0., 1., (pixels, rows, 3))
    for p in flat:
        s[p] = s[p, 0]
    return s


def test_a_negative_tolerance_lists_everything_until_the_cap():
    rng = np.random.default_rng(20261019)
    s = synthetic(rng, 64, 40, flat=range(0, 64, 3))
    recs, _ = CR.run(s, 8, 8, 8, -1., 0, 40)
    assert [int(l.sum()) for l, _ in recs] == [64] * 5 + [0]            # five passes of 8 fit under 40; the sixth is capped
    for k, (_, st) in enumerate(recs[:5]):
        assert np.all(st.n == 8 * (k + 1))
        ref_sum, ref_mean = PR.accumulate(None, s[:, :8 * (k + 1)], 0)  # the plain run in one pass: the same left fold
        assert st.S.tobytes() == ref_sum.tobytes() and st.mean.tobytes() == ref_mean.tobytes()
        y = CR.y_of(s[:, :8 * (k + 1)])
        assert np.allclose(st.Y, y.sum(axis=1), rtol=1e-13) and np.allclose(st.Q, (y * y).sum(axis=1), rtol=1e-13)


def test_identical_samples_settle_at_min_samples_and_neighbours_keep_sampling():
    rng = np.random.default_rng(20261020)
    noisy_pixel = 3 * 8 + 4
    s = synthetic(rng, 64, 64, flat=[p for p in range(64) if p != noisy_pixel])
    s[noisy_pixel, :, 0] = np.arange(64) % 2                            # y alternates by 1: its standard error stays above 0.01
    recs, _ = CR.run(s, 8, 8, 4, 0.01, 10, 64, check=False)
    counts = [int(l.sum()) for l, _ in recs]
    # 4, 8: below min_samples, everything; 12: the flat pixels have 12 >= 10 samples and m2 = 0: settled -- all but the noisy one's
    # four neighbours, which the widening keeps; the cap ends it
    assert counts[:3] == [64, 64, 64] and set(counts[3:16]) == {5} and counts[16] == 0 and len(counts) == 17
    listed = recs[3][0].reshape(8, 8)
    assert sorted(zip(*np.nonzero(listed))) == [(2, 4), (3, 3), (3, 4), (3, 5), (4, 4)]
    final = recs[-1][1].n.reshape(8, 8)
    assert final[3, 4] == 64 and final[2, 4] == 64 and final[0, 0] == 12 and len(np.unique(final)) == 2
    # a corner has two neighbours, and row rows - 1 never looks below
    corner = np.zeros(64, bool)
    corner[63] = True
    assert sorted(np.flatnonzero(CR.dilate(corner, 8, 8))) == [55, 62, 63]
    # unlisted pixels keep every value
    before, after = recs[3][1], recs[10][1]
    quiet = ~CR.dilate(np.arange(64) == noisy_pixel, 8, 8)
    assert before.S[quiet].tobytes() == after.S[quiet].tobytes() and np.all(before.n[quiet] == 12)


def test_the_cap_holds_whatever_the_slices():
    rng = np.random.default_rng(20261021)
    s = synthetic(rng, 64, 30)
    st = CR.State(8, 8)
    for k, ns in enumerate((7, 7, 7, 7, 5, 3, 2, 1, 1)):                # 28 fit; then 7 would pass 30, but 2 fits: 30; then nothing
        listed, _ = CR.one_pass(st, s, ns, -1., 0, 30, k == 0)
        assert int(listed.sum()) == (64 if k < 4 or k == 6 else 0), k
    assert np.all(st.n == 30)
    ref_sum, ref_mean = PR.accumulate(None, s, 0)
    assert st.S.tobytes() == ref_sum.tobytes() and st.mean.tobytes() == ref_mean.tobytes()
    # a NaN in the statistics leaves the pixel unsettled; a capped pixel is not listed however noisy its neighbours
    n, Yv, Q = np.full(4, 16, np.uint32), np.array([1., np.nan, 1., 1.]), np.array([1. / 16., 1., 1. / 16., 1. / 16.])
    listed, noisy = CR.select(n, Yv, Q, 4, 1, 8, 0.5, 16, 64)
    assert list(noisy) == [False, True, False, False] and list(listed) == [True, True, True, False]
    n[0] = 60
    listed, noisy = CR.select(n, Yv, Q, 4, 1, 8, 0.5, 16, 64)
    assert list(listed) == [False, True, True, False]


def test_prefix_sums_are_the_plain_fold(Y):
    s = CR.case_samples(Y, "demo-8")
    counts = np.random.default_rng(5).integers(1, 40, s.shape[0])
    got_s, got_m = CR.prefix_sums(s, counts)
    for c in (1, 8, 39):
        ref_s, ref_m = PR.accumulate(None, s[:, :c], 0)
        at = counts == c
        assert at.any() and got_s[at].tobytes() == ref_s[at].tobytes() and got_m[at].tobytes() == ref_m[at].tobytes()


# ---------------------------------------------------------------- the cases are not vacuous, and no decision in them is close
@pytest.mark.parametrize("name", sorted(CR.CASES))
def test_cases_converge_pixel_by_pixel_with_every_decision_clear(Y, name):
    scene, depth, aperture, radii, ns, tol, lo, hi = CR.CASES[name]
    s = CR.case_samples(Y, name)
    recs, nearest = CR.run(s, 32, 32, ns, tol, lo, hi)                  # (asserts the margin of every free decision)
    counts = [int(l.sum()) for l, _ in recs]
    final = recs[-1][1].n
    print("%s: %d passes, listed %s, %d samples cast (plain: %d), %d distinct counts, largest %d; the nearest decision is %.3g x 12 n ymax TIGHT away"
          % (name, len(recs), counts, sum(counts) * ns, 1024 * int(final.max()), len(np.unique(final)), int(final.max()), nearest))
    assert nearest > 1.
    assert (len(recs), sum(counts) * ns, len(np.unique(final))) == CR.FOUND[name]
    warm = -(-max(lo, 2) // ns)                                         # passes until a pixel can settle
    assert counts[:warm] == [1024] * warm and counts[-1] == 0
    assert all(0 < c < 1024 for c in counts[warm:-1]) and len(counts) > warm + 2
    for (a, _), (b, _) in zip(recs[warm:], recs[warm + 1:]):            # a settled pixel that is not sampled stays settled
        assert not (b & ~CR.dilate(a, 32, 32)).any()
    assert len(np.unique(final)) >= 3 and final.max() <= hi and final.min() >= max(lo, ns)
    if name not in ("demo-capped", "demo-soft-64", "penumbra-1"):
        assert final.max() + ns <= hi                                   # finished before the cap
    else:
        assert final.max() == hi
    # the left fold: every pixel holds the plain run's sum and mean at its own count
    ref_s, ref_m = CR.prefix_sums(s, final)
    assert recs[-1][1].S.tobytes() == ref_s.tobytes() and recs[-1][1].mean.tobytes() == ref_m.tobytes()
