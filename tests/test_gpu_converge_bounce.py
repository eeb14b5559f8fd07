"""Diffuse bounce in converging frames on the GPU (-m gpu): rm_accumulate_converging_bounce_device and rm_render_converging_bounce
through the C ABI, the Python bindings and the C++ mirror.

A converging frame is, pixel by pixel, the plain frame at that pixel's own count (tests/test_gpu_converge.py): so the bounce's
converging call is held byte for byte to rm_accumulate_bounce_device -- which tests/test_gpu_bounce.py holds to the yardstick,
tests/bounce_reference.py -- and, with strength 0, to rm_accumulate_converging_device in every buffer it writes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bounce_reference as BR
import denoise_reference as DR
import lens_reference as LR
import radiance_reference as RR
import test_gpu_bounce as GB
import test_gpu_converge as GC
import test_gpu_lens as GL
import workloads

pytestmark = pytest.mark.gpu

TIGHT = BR.TIGHT
NAN, BYTE = GC.NAN, GC.BYTE
KEYS = ("sum", "stats", "count", "mean", "rgb8", "mask")


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_converge_bounce"))


@pytest.fixture(scope="module")
def Y(pkg, O, entry, orc, tmp_path_factory):
    return BR.Yardstick(pkg, O, orc, BR.compile_helper(O, entry, tmp_path_factory.mktemp("orb_converge_bounce")))


def bounce_tables(pkg, c, n_rows, radii):
    import torch
    table, offsets = GC.device_tables(c, n_rows, radii)
    return table, offsets, torch.from_numpy(pkg.backend.bounce_sequence(0, n_rows)).to("cuda:0")


def bounce_pass(pkg, c, f, depth, aperture, focus, ns, tol, lo, hi, tables, strength, fresh, outputs=True):
    p = pkg.backend.make_params(workloads.FOV, float(f.h), float(f.w), depth)
    table, offsets, bounce = tables
    c.accumulate_converging_bounce_device(p, f.sum, f.stats, f.count, aperture, focus, ns, table, bounce, strength, tol, lo, hi, fresh,
                                          offsets=offsets, mean=f.mean if outputs else None, rgb8=f.rgb8 if outputs else None,
                                          mask=f.mask if outputs else None, workspace=f.ws[:f.ws_words])


def plain_bounce_snapshots(pkg, c, Y, name, depth, aperture, focus, ns, n_passes, radii, strength):
    """The plain run -- rm_accumulate_bounce_device in passes of ns over the library's sequences: count -> (sum, mean, bytes)."""
    import torch
    p = pkg.backend.make_params(workloads.FOV, 32., 32., depth)
    total = torch.full((32, 32, 3), NAN, dtype=torch.float64, device="cuda:0")
    mean = torch.full((32, 32, 3), NAN, dtype=torch.float64, device="cuda:0")
    rgb8 = torch.full((32, 32, 3), BYTE, dtype=torch.uint8, device="cuda:0")
    out = {}
    for k in range(n_passes):
        offsets = np.zeros((ns, Y.n_lights(name), 3)) if radii is None else c.light_sequence(k * ns, ns, radii)
        c.accumulate_bounce_device(p, total, aperture, focus, c.lens_sequence(k * ns, ns), offsets, pkg.backend.bounce_sequence(k * ns, ns),
                                   strength, k * ns, mean=mean, rgb8=rgb8)
        torch.cuda.synchronize()
        out[(k + 1) * ns] = (total.cpu().numpy().copy(), mean.cpu().numpy().copy(), rgb8.cpu().numpy().copy())
    return out


# ---------------------------------------------------------------- 1. strength 0 is the converging call
@pytest.mark.parametrize("name,depth", [("demo", 3), ("cornell", 3), ("synthetic256", 6)])
def test_strength_zero_is_the_converging_pass_byte_for_byte(pkg, ctx, Y, name, depth):
    """Three passes of 5 samples (12 pixels a wave, four idle lanes) at a tolerance that settles some pixels, with stored and
    with offset lights: sum, stats, count, list, mean, bytes and mask.  The bounce table holds NaN: it is not read."""
    import torch
    aperture, focus = GL.LENS[name]
    GL.upload(ctx, Y.scene(name)[0])
    for radii in (None, (GB.RADII,) * Y.n_lights(name)):
        tables = GC.device_tables(ctx, 32, radii)
        nan_bounce = torch.full((32, 2), NAN, dtype=torch.float64, device="cuda:0")
        f, g = GC.Frame(pkg, 32, 32), GC.Frame(pkg, 32, 32)
        for k in range(3):
            GC.converge_pass(pkg, ctx, f, depth, aperture, focus, 5, 0.05, 5, 32, tables, k == 0)
            bounce_pass(pkg, ctx, g, depth, aperture, focus, 5, 0.05, 5, 32, tables + (nan_bounce,), 0., k == 0)
            a, b = f.snapshot(), g.snapshot()
            assert a["listed"] == b["listed"] and np.array_equal(a["list"], b["list"])
            for key in KEYS:
                assert a[key].tobytes() == b[key].tobytes(), "%s, radii %s, pass %d: %s" % (name, radii, k, key)
        assert 0 < a["listed"] <= 1024 and a["mean"].any()


# ---------------------------------------------------------------- 2. a negative tolerance is the plain bounce frame
@pytest.mark.parametrize("name,depth", [("demo", 3), ("cornell", 3), ("synthetic256", 6)])
def test_a_negative_tolerance_is_the_plain_bounce_run_byte_for_byte(pkg, ctx, Y, name, depth):
    aperture, focus = GL.LENS[name]
    GL.upload(ctx, Y.scene(name)[0])
    for radii in (None, (GB.RADII,) * Y.n_lights(name)):
        plain = plain_bounce_snapshots(pkg, ctx, Y, name, depth, aperture, focus, 5, 3, radii, 1.)
        f, tables = GC.Frame(pkg, 32, 32), bounce_tables(pkg, ctx, 16, radii)
        for k in range(3):
            bounce_pass(pkg, ctx, f, depth, aperture, focus, 5, -1., 16, 16, tables, 1., k == 0)
            got, n = f.snapshot(), 5 * (k + 1)
            assert got["listed"] == 1024 and np.all(got["count"] == n)
            for key, ref in zip(("sum", "mean", "rgb8"), plain[n]):
                assert not (key != "rgb8" and np.isnan(got[key]).any())
                assert got[key].tobytes() == ref.tobytes(), "%s, radii %s, %d samples: %s differs in %d pixels" % (
                    name, radii, n, key, int((got[key] != ref).any(axis=2).sum()))
    # ... and the last of them, with area lights, is the yardstick's frame over the library's three sequences
    table, bounce = ctx.lens_sequence(0, 15), pkg.backend.bounce_sequence(0, 15)
    ref_sum, ref_mean = Y.bounce(name, 32, 32, depth, aperture, focus, table, ctx.light_sequence(0, 15, radii), bounce, 1., (15,))
    assert GL.worst(got["mean"], ref_mean) < TIGHT and GL.worst(got["sum"], ref_sum) < 15 * TIGHT


@pytest.mark.parametrize("name", BR.CONVERGING_VIEWS)
def test_a_negative_tolerance_is_the_plain_bounce_run_from_behind(pkg, ctx, Y, name):
    """The same under two of the views of BR.VIEWS -- inside the Cornell box, where every sample bounces off a back face, and
    behind the screens, on the basis's -z pole: through the pinhole with stored lights and through the lens with offset lights."""
    with GB.looking(pkg, ctx, Y, name) as (scene, depth, view, focus):
        for aperture, radii in ((0., None), (LR.APERTURE, (GB.RADII,) * Y.n_lights(scene))):
            plain = plain_bounce_snapshots(pkg, ctx, Y, scene, depth, aperture, focus, 5, 3, radii, 1.)
            f, tables = GC.Frame(pkg, 32, 32), bounce_tables(pkg, ctx, 16, radii)
            for k in range(3):
                bounce_pass(pkg, ctx, f, depth, aperture, focus, 5, -1., 16, 16, tables, 1., k == 0)
                got, n = f.snapshot(), 5 * (k + 1)
                assert got["listed"] == 1024 and np.all(got["count"] == n)
                for key, ref in zip(("sum", "mean", "rgb8"), plain[n]):
                    assert not (key != "rgb8" and np.isnan(got[key]).any())
                    assert got[key].tobytes() == ref.tobytes(), "%s, radii %s, %d samples: %s differs in %d pixels" % (
                        name, radii, n, key, int((got[key] != ref).any(axis=2).sum()))
            # ... and the last of them is the yardstick's frame under the view, whose samples are the ones the view is there for
            table, bounce = ctx.lens_sequence(0, 15), pkg.backend.bounce_sequence(0, 15)
            offsets = GB.zero_offsets(Y, scene, 15) if radii is None else ctx.light_sequence(0, 15, radii)
            c = Y.counters(scene, 32, 32, depth, aperture, focus, table, offsets, bounce, 1., view)
            if aperture == 0.:
                BR.assert_covers(name, c)
                assert name != "cornell-inside" or c["back"] == 15 * 1024
            ref_sum, ref_mean = Y.bounce(scene, 32, 32, depth, aperture, focus, table, offsets, bounce, 1., (15,), view)
            d_mean, d_sum = GL.worst(got["mean"], ref_mean), GL.worst(got["sum"], ref_sum)
            print("%s, aperture %g, radii %s, 3 x 5 samples: max |delta| mean %.3e, sum %.3e (%d samples bounce, %d from behind, %d on the -z pole)"
                  % (name, aperture, radii, d_mean, d_sum, c["bouncing"], c["back"], c["pole_down"]))
            assert d_mean < TIGHT and d_sum < 15 * TIGHT
            assert GL.worst(ref_mean, Y.bounce(scene, 32, 32, depth, aperture, focus, table, offsets, bounce, 1., (15,))[1]) > 0.05


# ---------------------------------------------------------------- 3. every pixel at its own count
@pytest.mark.parametrize("name,radii", [("demo", None), ("penumbra", (GB.RADII,) * 3)])
def test_every_pixel_holds_the_plain_bounce_run_at_its_own_count(pkg, ctx, Y, name, radii):
    depth, ns, tol, lo, hi = 3, 8, 0.05, 8, 64
    GL.upload(ctx, Y.scene(name)[0])
    f, tables = GC.Frame(pkg, 32, 32), bounce_tables(pkg, ctx, hi, radii)
    for k in range(hi // ns + 2):
        bounce_pass(pkg, ctx, f, depth, 0., LR.FOCUS, ns, tol, lo, hi, tables, 1., k == 0)
        last = f.snapshot()
        if last["listed"] == 0:
            break
    counts = last["count"]
    assert last["listed"] == 0 and len(np.unique(counts)) >= 3 and counts.max() <= hi and counts.min() >= lo
    plain = plain_bounce_snapshots(pkg, ctx, Y, name, depth, 0., LR.FOCUS, ns, int(counts.max()) // ns, radii, 1.)
    for c in np.unique(counts):
        at = counts == c
        for key, ref in zip(("sum", "mean", "rgb8"), plain[int(c)]):
            assert last[key][at].tobytes() == ref[at].tobytes(), "%s: %s of the pixels with %d samples" % (name, key, c)
    print("%s: %d distinct counts, %d .. %d; every pixel is the plain bounce run at its own count" % (name, len(np.unique(counts)), counts.min(), counts.max()))


# ---------------------------------------------------------------- 4. the tick
NS, TOL, LO, HI = 8, 0.05, 8, 64


def device_frame(pkg, c, p, passes, strength, radii=None, n_lights=2):
    """The frame `passes` ticks build, in buffers of the test's own -> (sum, stats, count, mean, bytes) tensors"""
    import torch
    h, w = p.frame_height, p.frame_width
    total, stats = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0"), torch.zeros((h, w, 2), dtype=torch.float64, device="cuda:0")
    count, mean = torch.zeros((h, w), dtype=torch.int32, device="cuda:0"), torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    rgb8 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")
    table, offsets, bounce = bounce_tables(pkg, c, HI, radii)
    for k in range(passes):
        c.accumulate_converging_bounce_device(p, total, stats, count, 0., LR.FOCUS, NS, table, bounce, strength, TOL, LO, HI, k == 0,
                                              offsets=offsets, mean=mean, rgb8=rgb8)
    torch.cuda.synchronize()
    return total, stats, count, mean, rgb8


def report_of(rep):
    return (rep.samples_cast, rep.listed, rep.passes, rep.max_count)


CPP_MAIN = r"""
#include <cstdio>
#include "rusty_marcher.hpp"
using namespace rusty_marcher;
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    scene::Scene sc = scene::Scene::create_default();
    framebuffer::FrameBuffer fb = framebuffer::create_frame_buffer(32, 32);
    renderer::Renderer r = renderer::create_renderer(1.5, 32., 32.);
    const rm_converge c{0.05, 8u, 64u};
    for (int k = 0; k < 3; k++) {
        const rm_converge_report rep = r.render_converging_bounce(fb, sc, c, 8u, 1., {}, 0., 5.);
        std::printf("passes %u max %u\n", rep.passes, rep.max_count);
    }
    std::FILE *f = std::fopen(argv[1], "wb");
    if (!f) return 3;
    for (const auto &row : fb.buffer) std::fwrite(row.data(), sizeof(Vec3f), row.size(), f);
    std::fclose(f);
    std::printf("plain %u\n", r.render_converging(fb, sc, c, 8u, {}, 0., 5.).passes);
    std::printf("bounce %u\n", r.render_converging_bounce(fb, sc, c, 8u, 1., {}, 0., 5.).passes);
    std::printf("strength %u\n", r.render_converging_bounce(fb, sc, c, 8u, 0.5, {}, 0., 5.).passes);
    return 0;
}
"""


def test_the_tick_through_c_python_and_the_cpp_mirror(pkg, entry, ctx, Y, capsys, tmp_path):
    L, B = pkg.lib(), pkg._lib
    scene = Y.scene("demo")[0]
    GL.upload(ctx, scene)
    p = pkg.backend.make_params(workloads.FOV, 32., 32., 3)

    def tick(strength=1., restart=False, radii=None, **kw):
        return ctx.render_converging_bounce(p, 0., LR.FOCUS, NS, TOL, LO, HI, strength, radii, restart, **kw)[1]

    def plain(restart=False, **kw):
        return ctx.render_converging(p, 0., LR.FOCUS, NS, TOL, LO, HI, restart=restart, **kw)[1]

    # three ticks: the frame goes on, and is the device call's over the library's three sequences
    host, host8 = np.full((32, 32, 3), NAN), np.full((32, 32, 3), BYTE, np.uint8)
    assert tick(restart=True).passes == 1 and tick().passes == 2
    rep = tick(host_rgb=host, host_rgb8=host8)
    total, stats, count, mean, rgb8 = device_frame(pkg, ctx, p, 3, 1.)
    assert rep.passes == 3 and rep.max_count == int(count.max()) == 24
    assert host.tobytes() == mean.cpu().numpy().tobytes() and host8.tobytes() == rgb8.cpu().numpy().tobytes()
    first = report_of(rep)
    # what begins the frame again, one at a time
    assert tick(0.5).passes == 1 and tick(0.5).passes == 2            # a changed strength
    assert tick().passes == 1                                         # ... and back
    assert plain().passes == 1 and plain().passes == 2                # bounce -> plain
    assert tick().passes == 1                                         # plain -> bounce
    assert tick(0.).passes == 1                                       # a strength of zero is a strength
    assert tick(radii=(1.5, 1.5)).passes == 1 and tick(radii=(1.5, 1.5)).passes == 2   # radii
    try:                                                              # a camera move, history on or off
        ctx.converge_history((0.1, 0.9, 32))
        assert tick().passes == 1 and tick().passes == 2
        ctx.look_at((0.5, 0., 0.), (0.5, 0., -10.))
        assert tick().passes == 1 and ctx.history_info()["last_reprojected"] == 0
    finally:
        ctx.converge_history(None)
        ctx.orient(None)
        GL.upload(ctx, scene)
    # ... and the frame of the first three ticks again, byte for byte
    assert tick(restart=True).passes == 1 and tick().passes == 2
    again = np.full((32, 32, 3), NAN)
    assert report_of(tick(host_rgb=again)) == first and again.tobytes() == host.tobytes()
    # a refused call changes nothing
    lens, conv = B.rm_lens(0., LR.FOCUS, NS, 0), B.rm_converge(TOL, LO, HI)
    D = C.POINTER(C.c_double)
    for bad in (-1., NAN, float("inf")):
        before = again.copy()
        st = L.rm_render_converging_bounce(ctx.ptr, C.byref(p), C.byref(lens), C.byref(conv), None, 0, bad, 0, again.ctypes.data_as(D), None, None, None)
        assert st == B.RM_ERR_INVALID_ARG and b"strength" in L.rm_last_error(ctx.ptr) and again.tobytes() == before.tobytes()
    assert tick().passes == 4
    # run to the end: a finished picture launches nothing
    for k in range(HI // NS + 2):
        rep = tick()
        if rep.listed == 0:
            break
    assert rep.listed == 0
    timing_rep = ctx.render_converging_bounce(p, 0., LR.FOCUS, NS, TOL, LO, HI, 1., host_rgb=host)
    assert timing_rep[0].kernel_ms == 0. and timing_rep[1].listed == 0 and timing_rep[1].passes == rep.passes
    # Renderer.render_converging_bounce and render_converged_bounce
    r = pkg.create_renderer(workloads.FOV, 32., 32.)
    r.max_depth = 3
    fb = pkg.create_frame_buffer(32, 32)
    capsys.readouterr()
    for k in range(3):
        got = r.render_converging_bounce(fb, scene, TOL, NS, 1., LO, HI, focus=LR.FOCUS, restart=(k == 0))
    assert "compute units used" in capsys.readouterr().out
    assert report_of(got) == first and r.last_samples == 24 and fb.buffer.tobytes() == again.tobytes()
    end = r.render_converged_bounce(fb, scene, TOL, NS, 1., LO, HI, focus=LR.FOCUS)
    assert end.listed == 0 and end.passes == rep.passes and fb.buffer.tobytes() == host.tobytes()
    # the C++ mirror, from compiled code
    src, exe, dump = tmp_path / "tick.cpp", tmp_path / "tick", tmp_path / "tick.f64"
    src.write_text(CPP_MAIN)
    lib_dir = os.path.join(entry.PKG_DIR, "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(entry.ROOT, "include"), "-I", os.path.join(entry.PKG_DIR, "host"),
                           str(src), "-o", str(exe), "-L", lib_dir, "-lrusty_marcher_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath," + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")])
    log = subprocess.check_output([str(exe), str(dump)]).decode()
    assert [l for l in log.splitlines() if l.split()[0] in ("passes", "plain", "bounce", "strength")] == \
        ["passes 1 max 8", "passes 2 max 16", "passes 3 max 24", "plain 1", "bounce 1", "strength 1"]
    assert np.fromfile(str(dump)).tobytes() == again.tobytes()


def test_the_filter_serves_the_bounce_tick_and_leaves_its_frame_alone(pkg, ctx, Y):
    """rm_render_denoised after the bounce tick: the yardstick's filter (tests/denoise_reference.py) over that tick's buffers --
    rebuilt with the device call, whose bytes the tick's are -- byte for byte; the converging frame goes on as if unfiltered."""
    GL.upload(ctx, Y.scene("demo")[0])
    p = pkg.backend.make_params(workloads.FOV, 32., 32., 3)

    def tick(restart=False, **kw):
        return ctx.render_converging_bounce(p, 0., LR.FOCUS, NS, TOL, LO, HI, 1., None, restart, **kw)[1]

    for k in range(3):
        tick(restart=(k == 0))
    total, stats, count, mean, _ = device_frame(pkg, ctx, p, 3, 1.)
    hits = ctx.primary_hits_device(p).raw.cpu().numpy().view(DR.HIT_DTYPE).reshape(32, 32)
    for guides, iterations in ((True, 5), (False, 2)):
        ctl = DR.Control(iterations=iterations)
        want, _, want8 = DR.denoise(total.cpu().numpy(), stats.cpu().numpy(), count.cpu().numpy().view(np.uint32), hits if guides else None, ctl)
        got, got8 = np.full((32, 32, 3), NAN), np.full((32, 32, 3), BYTE, np.uint8)
        ctx.render_denoised(p, iterations=iterations, guides=guides, host_rgb=got, host_rgb8=got8)
        assert got.tobytes() == want.tobytes() and got8.tobytes() == want8.tobytes(), (guides, iterations)
        assert got.tobytes() != mean.cpu().numpy().tobytes()
    # the frame was left alone: the next tick is the fourth pass of the unfiltered run
    after = np.full((32, 32, 3), NAN)
    rep = tick(host_rgb=after)
    assert rep.passes == 4 and after.tobytes() == device_frame(pkg, ctx, p, 4, 1.)[3].cpu().numpy().tobytes()
