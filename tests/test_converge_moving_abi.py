"""CPU-side checks of the converging frames with moving shapes (include/rusty_marcher_amd.h, "converging frames with moving
shapes").

1. The two entry points are exported and bound by ctypes, the Rust shim and the C++ mirror with the header's shapes -- those of
   their ..._motion counterparts --, the mirror compiles, rm_build_info says " converge-moving" and the ABI is still 5, a NULL
   context is refused with nothing written, and the Python wrappers raise before the library is called.
2. The cases the GPU tests use (tests/converge_moving_reference.py) are not vacuous and no decision in them is close: the
   committed numbers of passes, samples and distinct counts, counted with the oracle alone; the motion of the polygons and meshes
   changes the final count of more than 5 % of the frame's pixels in every case; a pixel's sum at its count is the left fold of
   its rows; with only the spheres moving the yardstick finds converge_motion_reference's numbers.
3. The staging rule's three tick kinds, side by side, in a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import converge_motion_reference as CMR
import converge_moving_reference as CMV
import converge_reference as CR
import lens_reference as LR
import moving_reference as MV
import progressive_reference as PR
import radiance_reference as RR
import test_rust_binding as RB
import workloads

FUNCTIONS = ["rm_accumulate_converging_moving_device", "rm_render_converging_moving"]
D, U8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_converge_moving_abi"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return CMV.Yardstick(pkg, O, orc)


# ---------------------------------------------------------------- the ABI
def test_converge_moving_symbols_are_exported_and_bound(pkg, entry):
    L = pkg.lib()
    header = open(os.path.join(entry.ROOT, "include", "rusty_marcher_amd.h")).read()
    lib_py = open(os.path.join(entry.PKG_DIR, "_lib.py")).read()
    for name in FUNCTIONS:
        assert hasattr(L, name), "library does not export %s" % name
        assert name in pkg._lib.SIGNATURES and '"%s"' % name in lib_py
        assert re.search(r"^rm_status %s\(" % name, header, flags=re.M), name
        motion = name.replace("moving", "motion")
        restype, argtypes = pkg._lib.SIGNATURES[name]
        assert (restype, list(argtypes)) == (pkg._lib.SIGNATURES[motion][0], list(pkg._lib.SIGNATURES[motion][1])), name
        assert getattr(L, name).argtypes == getattr(L, motion).argtypes
    assert "converging frames with moving shapes" in header and "converging frames with moving spheres" in header
    for name in ("accumulate_converging_moving_device", "render_converging_moving"):
        assert callable(getattr(pkg.backend.Context, name))
    assert callable(pkg.Renderer.render_converging_moving) and callable(pkg.Renderer.render_converged_moving)


def test_converge_moving_functions_have_the_header_shapes_in_the_rust_shim_and_the_cpp_mirror(entry):
    c, r = RB.header_functions(), RB.rust_functions()
    for name in FUNCTIONS:
        assert name in c and name in r, name
        assert c[name] == r[name], "%s: header %s, gpu.rs %s" % (name, c[name], r[name])
    assert c["rm_accumulate_converging_moving_device"] == c["rm_accumulate_converging_motion_device"] == (
        "i32", ["ptr"] * 5 + ["u32", "ptr", "u32", "ptr", "u32", "i32", "ptr", "ptr"])
    assert c["rm_render_converging_moving"] == c["rm_render_converging_motion"] == ("i32", ["ptr"] * 5 + ["u32", "ptr", "u32", "f64", "i32"] + ["ptr"] * 4)
    text = open(RB.RUST).read()
    assert re.search(r"pub fn render_converging_moving\(\s*&mut self", text) and "rm_render_converging_moving(self.ctx" in text
    assert re.search(r"pub fn accumulate_converging_moving\(\s*&mut self", text) and "rm_accumulate_converging_moving_device(self.ctx" in text
    hpp = open(os.path.join(entry.PKG_DIR, "host", "rusty_marcher.hpp")).read()
    assert re.search(r"render_converging_moving\(framebuffer::FrameBuffer", hpp) and "rm_render_converging_moving(ctx_" in hpp


def test_cpp_mirror_compiles_with_the_converging_moving_render(entry, tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "rusty_marcher.hpp"\nusing namespace rusty_marcher;\n'
                   'unsigned tick(renderer::Renderer &r, framebuffer::FrameBuffer &fb, const scene::Scene &sc) {'
                   ' const rm_converge c{0.01, 16u, 1024u};'
                   ' std::vector<Vec3f> v(sc.shapes.size(), Vec3f{0., 1., 0.}); v[0] = Vec3f{1., 0., 0.5};'
                   ' r.render_converging_moving(fb, sc, v, 1., c, 8u); r.render_converging_moving(fb, sc, v, 0.5, c, 8u, {1.5, 1.5}, 0.4, 5., true);'
                   ' r.render_converging_motion(fb, sc, v, 1., c, 8u);'
                   ' return r.last_report.listed + r.last_samples; }\n'
                   'int main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(entry.ROOT, "include"),
                           "-I", os.path.join(entry.PKG_DIR, "host"), str(src)])


def test_build_info_announces_converge_moving(pkg):
    L = pkg.lib()
    info = L.rm_build_info().decode()
    words = info.split(" ")
    assert " converge-moving" in info
    assert "converge-moving" in words and "converge-motion" in words and "moving-shapes" in words and words[-1] == "converge"
    assert L.rm_abi_version() == 5


def test_converge_moving_entry_points_refuse_null_context(pkg):
    L, B = pkg.lib(), pkg._lib
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 3)
    lens, conv = B.rm_lens(LR.APERTURE, LR.FOCUS, 4, 0), B.rm_converge(0.01, 16, 64)
    frame, bytes8 = np.full((64, 64, 3), 7.25), np.full((64, 64, 3), 7, np.uint8)
    report = B.rm_converge_report(77, 77, 77, 77, 0)
    buffers = B.rm_converge_frame()
    v = np.ones((3, 3))
    assert L.rm_accumulate_converging_moving_device(None, C.byref(p), C.byref(lens), C.byref(conv), None, 64, None, 2, None, 3, 1,
                                                    C.byref(buffers), None) == B.RM_ERR_INVALID_ARG
    assert b"NULL ctx" in L.rm_last_error(None) and b"rm_accumulate_converging_moving_device" in L.rm_last_error(None)
    assert L.rm_render_converging_moving(None, C.byref(p), C.byref(lens), C.byref(conv), None, 0, v.ctypes.data_as(C.POINTER(B.rm_vec3)), 3, 1., 0,
                                         frame.ctypes.data_as(D), bytes8.ctypes.data_as(U8), C.byref(report), None) == B.RM_ERR_INVALID_ARG
    assert b"NULL ctx" in L.rm_last_error(None) and b"rm_render_converging_moving" in L.rm_last_error(None)
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
    n = len(demo.shapes)
    assert n >= 3 and len(demo.lights) == 2
    good = [pkg.Vec3f(1., 0., 0.5)] + [pkg.Vec3f(0., 1., 0.)] * (n - 1)   # every shape moves
    r, fb = pkg.create_renderer(workloads.FOV, 64., 64.), pkg.create_frame_buffer(64, 64)

    def low(v=good, shutter=1., aperture=0.4, focus=5., ns=8, tol=0.01, lo=16, hi=64, **kw):
        return K.Context.render_converging_moving(ctx, p, v, shutter, aperture, focus, ns, tol, lo, hi, **kw)

    def high(v=good, shutter=1., tol=0.01, ns=8, lo=16, hi=64, **kw):
        return r.render_converging_moving(fb, demo, v, shutter, tol, ns, lo, hi, **kw)

    def shot(v=good, shutter=1., tol=0.01, ns=8, lo=16, hi=64, **kw):
        return r.render_converged_moving(fb, demo, v, shutter, tol, ns, lo, hi, **kw)

    # rm_converge: a NaN tolerance; sample numbers that are no integers, negative, or out of order with n_samples and the cap
    for tol, lo, hi in ((nan, 16, 64), (0.01, -1, 64), (0.01, 1.5, 64), (0.01, True, 64), (0.01, 16, 7), (0.01, 16, 65537), (0.01, 16, 64.5),
                        (0.01, 16, None), (0.01, 2 ** 32, 64)):
        for call in (low, high, shot):
            with pytest.raises((ValueError, TypeError)):
                call(tol=tol, lo=lo, hi=hi)
    # bad velocities: not finite, not vectors, not a sequence
    for bad in ([(nan, 0., 0.)] + [None] * (n - 1), [(0., inf, 0.)] + [None] * (n - 1), [None] * (n - 1) + [(0., 0., -inf)],
                [(1., 2.)] + [None] * (n - 1), ["abc"] + [None] * (n - 1), 1.5, None, "12"):
        for call in (low, high, shot):
            with pytest.raises(ValueError):
                call(v=bad)
    # a velocity list of the wrong length for the scene: the renderer knows the scene
    for bad in ([], good[:-1], good + [None]):
        for call in (high, shot):
            with pytest.raises(ValueError, match="one velocity a shape"):
                call(v=bad)
    # the shutter
    for shutter in (-0.1, nan, inf, -inf, "1", None, True):
        for call in (low, high, shot):
            with pytest.raises(ValueError, match="shutter"):
                call(shutter=shutter)
    # radii, where given, as the soft wrappers check them
    for radii in ((-0.1, 1.), (nan, 1.), "12", 1.5):
        with pytest.raises(ValueError):
            low(radii=radii)
        with pytest.raises(ValueError):
            high(light_radii=radii)
    with pytest.raises(ValueError, match="one radius a light"):
        high(light_radii=(1.5,))
    # the lens, as the progressive wrappers check it
    for aperture, focus, ns in ((-0.1, 5., 4), (nan, 5., 4), (0.4, 0., 4), (0.4, inf, 4), (0.4, 5., 0), (0.4, 5., 65), (0.4, 5., 2.5), (0.4, 5., True)):
        with pytest.raises(ValueError):
            low(aperture=aperture, focus=focus, ns=ns)
        with pytest.raises(ValueError):
            high(ns=ns, aperture=aperture, focus=focus)
    # bad host buffers: too small; float32; a list; float64 bytes; strided
    for host_rgb, host_rgb8 in ((np.zeros((32, 64, 3)), None), (np.zeros((64, 64, 3), np.float32), None), ([0.] * 12288, None),
                                (None, np.zeros((64, 64, 3))), (np.zeros((64, 64, 6))[:, :, ::2], None)):
        with pytest.raises(ValueError):
            low(host_rgb=host_rgb, host_rgb8=host_rgb8)
    # the device call: every buffer -- numpy; another dtype; on the CPU; another shape; missing -- before anything else
    table, lights, shapes = PR.lens_sequence(0, 64), np.zeros((64, 2, 3)), np.zeros((64, n, 3))
    ok = dict(sum=torch.zeros((64, 64, 3), dtype=torch.float64), stats=torch.zeros((64, 64, 2), dtype=torch.float64),
              count=torch.zeros((64, 64), dtype=torch.int32))
    for name in ok:
        t = ok[name]
        for bad in (t.numpy(), t.to(torch.float32), t, t[:32].contiguous(), None):
            args = dict(ok)
            args[name] = bad
            with pytest.raises(ValueError):
                K.Context.accumulate_converging_moving_device(ctx, p, args["sum"], args["stats"], args["count"], 0.4, 5., 8, table, lights, shapes,
                                                              0.01, 16, 64, True)


# ---------------------------------------------------------------- the cases are not vacuous, and no decision in them is close
def test_the_cases_are_the_proposed_ones_at_the_proposed_speeds():
    assert CMV.CASES == {
        "demo-moving-8": ("demo", 3, LR.APERTURE, None, 8, 0.1, 16, 256),
        "cornell-moving-8": ("cornell", 3, 0., None, 8, 0.1, 16, 256),
        "pool-moving-5": ("pool", 3, LR.APERTURE, None, 5, 0.1, 16, 256),
        "spheres-moving-8": ("synthetic256", 6, LR.APERTURE, None, 8, 0.1, 16, 256),
        "demo-moving-soft-64": ("demo", 3, LR.APERTURE, (1.5, 3.), 64, 0.05, 16, 256),
        "pool-moving-1": ("pool", 3, LR.APERTURE, None, 1, 0.1, 16, 40),
    }
    assert CMV.SPEED == {name: MV.SPEED[case[0]] for name, case in CMV.CASES.items()}
    assert sorted(CMV.FOUND) == sorted(CMV.DIFFER) == sorted(CMV.CASES)
    for name, motion in CMV.MOTION.items():
        assert CMV.CASES[name] == CMR.CASES[motion]


@pytest.mark.parametrize("name", sorted(CMV.CASES))
def test_cases_converge_pixel_by_pixel_with_every_decision_clear(Y, name):
    scene, depth, aperture, radii, ns, tol, lo, hi = CMV.CASES[name]
    s = CMV.case_samples(Y, name)
    recs, nearest = CR.run(s, 32, 32, ns, tol, lo, hi)                  # (asserts the margin of every free decision)
    counts = [int(l.sum()) for l, _ in recs]
    final = recs[-1][1].n
    print("%s: %d passes, listed %s, %d samples cast (plain: %d), %d distinct counts, largest %d; the nearest decision is %.3g x 12 n ymax TIGHT away"
          % (name, len(recs), counts, sum(counts) * ns, 1024 * int(final.max()), len(np.unique(final)), int(final.max()), nearest))
    assert nearest > 1.
    assert (len(recs), sum(counts) * ns, len(np.unique(final))) == CMV.FOUND[name]
    warm = -(-max(lo, 2) // ns)                                         # passes until a pixel can settle
    assert counts[:warm] == [1024] * warm and counts[-1] == 0
    assert all(0 < c < 1024 for c in counts[warm:-1]) and len(counts) > warm + 2
    assert final.max() <= hi and final.min() >= max(lo, ns)
    # the left fold: every pixel holds the plain moving-shapes run's sum and mean at its own count
    ref_s, ref_m = CR.prefix_sums(s, final)
    assert recs[-1][1].S.tobytes() == ref_s.tobytes() and recs[-1][1].mean.tobytes() == ref_m.tobytes()
    # not vacuous: what moves beside the spheres changes which pixels go on being sampled -- the final count of more than 5 % of
    # the frame differs from the same case with only the spheres moving
    kinds = Y.kinds(scene)
    assert any(k != MV.ORC_SPHERE for k in kinds)
    only = CMV.case_samples(Y, name, spheres_only=True)
    still, _ = CR.run(only, 32, 32, ns, tol, lo, hi, check=False)
    differ = int((still[-1][1].n != final).sum())
    print("    %d pixels end with another count than with only the spheres moving" % differ)
    assert differ == CMV.DIFFER[name] and differ > 0.05 * 1024
    # ... and with only the spheres moving the yardstick is the moving spheres': its samples and what it finds
    if name in CMV.MOTION:
        motion = CMV.MOTION[name]
        assert np.ascontiguousarray(only).tobytes() == np.ascontiguousarray(CMR.case_samples(CMR.Yardstick(Y.pkg, Y.O, Y.orc), motion)).tobytes()
        assert (len(still), sum(int(l.sum()) for l, _ in still) * ns, len(np.unique(still[-1][1].n))) == CMR.FOUND[motion]
    else:
        assert not any(k == MV.ORC_SPHERE for k in kinds) or scene == "pool"


# ---------------------------------------------------------------- the staging rule, stand-alone under the sanitizers
def test_staging_rule_has_three_tick_kinds_under_asan_ubsan(entry, tmp_path):
    exe = tmp_path / "staging_kinds"
    subprocess.check_call([
        "g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
        "-I", os.path.join(entry.ROOT, "include"), "-I", os.path.join(entry.PKG_DIR, "csrc"),
        os.path.join(entry.PKG_DIR, "csrc", "rm_sampling.cpp"), os.path.join(entry.ROOT, "tests", "native", "staging_kinds_main.cpp"),
        "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([str(exe)], capture_output=True, env=env)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert b"staging kinds ok: 48 cases" in out.stdout
