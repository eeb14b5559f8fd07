"""The variance-guided filter's tick on the GPU (-m gpu): rm_render_denoised through the Python binding and Renderer.render_denoised.

The tick filters the context's converging frame, whose buffers no call hands out.  But the converging tick is, byte for byte, the
device call over the library's own sequences (tests/test_gpu_converge.py holds it to that), so the same frame is built here with
rm_accumulate_converging_device into buffers of the test's own, filtered with rm_denoise_device -- which tests/test_gpu_denoise.py
holds to the yardstick -- and the tick must write those bytes."""
import numpy as np
import pytest

import workloads

pytestmark = pytest.mark.gpu

NAN, BYTE = float("nan"), 0xA5
H, W, ROWS = 72, 64, 64                                                # 72 % 32 = 8 rows the filter leaves alone
NS, TOL, LO, HI = 8, 0.02, 8, 64
APERTURE, FOCUS = 0., 5.                                               # a pinhole: the guide's view is the picture's


@pytest.fixture()
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    c.orient(None)
    c.upload(workloads.product_scene(pkg, "demo").flatten())
    yield c
    c.close()


def params(pkg, h=H, w=W, depth=3):
    return pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)


def tick(c, p, restart=False, **kw):
    return c.render_converging(p, APERTURE, FOCUS, NS, TOL, LO, HI, restart=restart, **kw)


def device_frame(c, p, passes):
    """The frame `passes` ticks build, in buffers of the test's own -> (sum, stats, count, mean) tensors"""
    import torch
    h, w = p.frame_height, p.frame_width
    total, stats = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0"), torch.zeros((h, w, 2), dtype=torch.float64, device="cuda:0")
    count, mean = torch.zeros((h, w), dtype=torch.int32, device="cuda:0"), torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    table = torch.from_numpy(c.lens_sequence(0, HI)).to("cuda:0")
    for k in range(passes):
        c.accumulate_converging_device(p, total, stats, count, APERTURE, FOCUS, NS, table, TOL, LO, HI, k == 0, mean=mean)
    torch.cuda.synchronize()
    return total, stats, count, mean


def report_of(rep):
    return (rep.samples_cast, rep.listed, rep.passes, rep.max_count)


def test_the_tick_is_the_device_call_over_the_converging_frame(pkg, ctx):
    import torch
    p = params(pkg)
    host = np.full((H, W, 3), NAN)
    for k in range(3):
        tick(ctx, p, restart=(k == 0), host_rgb=host)
    total, stats, count, mean = device_frame(ctx, p, 3)
    assert host[:ROWS].tobytes() == mean.cpu().numpy()[:ROWS].tobytes()     # (the same frame, as the converging frames promise)
    hits = ctx.primary_hits_device(p)
    seen = {}
    for guides in (True, False):
        for iterations in (0, 2, 5):
            out = torch.full((H, W, 3), NAN, dtype=torch.float64, device="cuda:0")
            rgb8 = torch.full((H, W, 3), BYTE, dtype=torch.uint8, device="cuda:0")
            ctx.denoise_device(p, total, stats, count, out, iterations=iterations, hits=hits if guides else None, rgb8=rgb8)
            torch.cuda.synchronize()
            got, got8 = np.full((H, W, 3), NAN), np.full((H, W, 3), BYTE, np.uint8)
            timing = ctx.render_denoised(p, iterations=iterations, guides=guides, host_rgb=got, host_rgb8=got8)
            assert got[:ROWS].tobytes() == out.cpu().numpy()[:ROWS].tobytes(), (guides, iterations)
            assert got8[:ROWS].tobytes() == rgb8.cpu().numpy()[:ROWS].tobytes(), (guides, iterations)
            assert np.isnan(got[ROWS:]).all() and (got8[ROWS:] == BYTE).all()    # rows from `rows` on are not the tick's
            assert timing.kernel_ms > 0. and timing.total_ms >= timing.kernel_ms
            seen[(guides, iterations)] = got[:ROWS].copy()
    assert seen[(True, 0)].tobytes() == host[:ROWS].tobytes()              # no iterations: the converging frame's mean
    assert seen[(True, 0)].tobytes() == seen[(False, 0)].tobytes()
    # the guide matters on the demo: with it the filter leaves the silhouettes alone
    assert seen[(True, 5)].tobytes() != seen[(False, 5)].tobytes() and seen[(True, 5)].tobytes() != host[:ROWS].tobytes()
    # without outputs the tick still runs
    assert ctx.render_denoised(p).kernel_ms > 0.


def test_a_converging_tick_after_the_filter_continues_the_same_frame(pkg, ctx):
    p = params(pkg)

    def run(filtered):
        out = []
        for k in range(5):
            mean, rgb8 = np.full((H, W, 3), NAN), np.full((H, W, 3), BYTE, np.uint8)
            _, rep = tick(ctx, p, restart=(k == 0), host_rgb=mean, host_rgb8=rgb8)
            out.append((mean.tobytes(), rgb8.tobytes(), report_of(rep)))
            if filtered and k >= 1:
                ctx.render_denoised(p, guides=(k % 2 == 0), host_rgb=np.zeros((H, W, 3)))
                ctx.render_denoised(p, iterations=k, guides=(k % 2 == 1))
        return out

    plain, filtered = run(False), run(True)
    assert plain == filtered
    assert plain[-1][2][2] == 5 and plain[-1][2][0] > plain[1][2][0]         # five passes, and they did go on sampling
    # ... and the frame the ticks left is still the device call's: sum, stats and count could not have changed unseen
    total, stats, count, mean = device_frame(ctx, p, 5)
    assert mean.cpu().numpy()[:ROWS].tobytes() == np.frombuffer(filtered[-1][0]).reshape(H, W, 3)[:ROWS].tobytes()
    assert int(count.cpu().numpy().max()) == filtered[-1][2][3]


def test_the_tick_is_refused_without_a_frame_and_after_a_change_of_geometry(pkg, ctx):
    B = pkg._lib
    p = params(pkg)
    host = np.full((H, W, 3), NAN)
    with pytest.raises(B.BackendError, match="rm_render_denoised: no converging frame") as e:
        ctx.render_denoised(p, host_rgb=host)
    assert e.value.status == B.RM_ERR_INVALID_ARG and np.isnan(host).all()
    tick(ctx, p, restart=True)
    ctx.render_denoised(p, host_rgb=host)
    assert np.isfinite(host[:ROWS]).all()
    for h, w in ((H, 96), (104, W), (32, 32)):
        other = np.full((h, w, 3), NAN)
        with pytest.raises(B.BackendError, match="rm_render_denoised: the converging frame is 64 x 72, params say %d x %d" % (w, h)) as e:
            ctx.render_denoised(params(pkg, h, w), host_rgb=other)
        assert e.value.status == B.RM_ERR_INVALID_ARG and np.isnan(other).all()
    # the library's own checks of the control, by name (the wrapper's are in front of them: straight through ctypes)
    import ctypes as C
    bad = B.rm_denoise(4., .1, 1e-10, 1., 6, 5)
    assert ctx.L.rm_render_denoised(ctx.ptr, C.byref(p), C.byref(bad), 1, None, None, None) == B.RM_ERR_INVALID_ARG
    assert b"rm_render_denoised: denoise.iterations = 6 is outside 0..5" in ctx.L.rm_last_error(ctx.ptr)
    assert ctx.L.rm_render_denoised(ctx.ptr, C.byref(p), None, 1, None, None, None) == B.RM_ERR_INVALID_ARG
    assert b"rm_render_denoised: NULL denoise" in ctx.L.rm_last_error(ctx.ptr)
    # a refused tick left the frame and the filter's state usable
    again = np.full((H, W, 3), NAN)
    ctx.render_denoised(p, host_rgb=again)
    assert again.tobytes() == host.tobytes()


def test_renderer_render_denoised_end_to_end(pkg, capsys):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    scene = workloads.product_scene(pkg, "demo")
    r = pkg.create_renderer(workloads.FOV, 64., 64.)
    frame = pkg.create_frame_buffer(64, 64)
    for k in range(3):
        rep = r.render_converging(frame, scene, TOL, NS, min_samples=LO, max_samples=HI, restart=(k == 0))
    noisy = frame.buffer.copy()
    out = pkg.create_frame_buffer(64, 64)
    message = r.render_denoised(out, scene)
    assert message in capsys.readouterr().out and r.last_timing.kernel_ms > 0. and r.last_samples == rep.max_count
    assert frame.buffer.tobytes() == noisy.tobytes()                      # the other frame buffer is the caller's
    # the same through the device calls on the renderer's context, with the wrapper's defaults
    c = pkg.backend.default_context(0)
    p = pkg.backend.make_params(r.fov, r.height, r.width, r.max_depth)
    p.frame_width, p.frame_height = 64, 64
    table = torch.from_numpy(c.lens_sequence(0, HI)).to("cuda:0")
    total, stats = torch.zeros((64, 64, 3), dtype=torch.float64, device="cuda:0"), torch.zeros((64, 64, 2), dtype=torch.float64, device="cuda:0")
    count, want = torch.zeros((64, 64), dtype=torch.int32, device="cuda:0"), torch.zeros((64, 64, 3), dtype=torch.float64, device="cuda:0")
    for k in range(3):
        c.accumulate_converging_device(p, total, stats, count, 0., 1., NS, table, TOL, LO, HI, k == 0)
    c.denoise_device(p, total, stats, count, want, hits=c.primary_hits_device(p))
    torch.cuda.synchronize()
    assert out.buffer.tobytes() == want.cpu().numpy().tobytes()
    assert out.buffer.tobytes() != noisy.tobytes()
    unguided = pkg.create_frame_buffer(64, 64)
    r.render_denoised(unguided, scene, guides=False, iterations=2)
    assert unguided.buffer.tobytes() != out.buffer.tobytes()
    # the converging frame goes on where it was
    assert r.render_converging(frame, scene, TOL, NS, min_samples=LO, max_samples=HI).passes == 4
