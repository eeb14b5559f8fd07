"""Progressive frames on the GPU (-m gpu): rm_accumulate_lens_device and rm_render_progressive through the C ABI, the Python
bindings and the C++ mirror, against tests/progressive_reference.py -- the lens rays in numpy, cast by the CPU oracle's
cast_ray, folded in table order across passes (pinned on the CPU by tests/test_progressive_abi.py) -- and against the lens
frames of rm_render_lens_device.

What the header calls byte for byte is demanded byte for byte; against the yardstick every channel of every pixel of the rows
a pass writes is demanded within TIGHT = 1e-9 of the mean (n TIGHT of a sum of n samples), no pixel left out.  Largest
deviations observed on an MI355X are recorded in DESIGN.md section 6h."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lens_reference as LR
import progressive_reference as PR
import radiance_reference as RR
import test_gpu_lens as GL
import test_gpu_query as GQ
import workloads

pytestmark = pytest.mark.gpu

TIGHT = PR.TIGHT
LENS = GL.LENS
SCENES = [("demo", 3), ("cornell", 3), ("synthetic256", 6)]          # depth 6: the kernels with STACK = 32; 256 spheres: the hierarchy
NAN = float("nan")
BYTE = 0x5a                                                          # what a byte buffer holds beforehand


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_progressive"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return PR.Yardstick(pkg, O, orc)


def run_passes(pkg, c, w, h, depth, aperture, focus, table, sizes, want_mean=True, want_bytes=True, flags=0):
    """Passes of the sizes `sizes` over consecutive slices of `table` on torch's current stream, the first with n_before = 0,
    into buffers that held NaN (and BYTE) -> (sum, mean, bytes) as numpy, None for what was not asked for."""
    import torch
    p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)
    p.flags = flags
    total = torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda:0")
    mean = torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda:0") if want_mean else None
    rgb8 = torch.full((h, w, 3), BYTE, dtype=torch.uint8, device="cuda:0") if want_bytes else None
    torch.cuda.synchronize()
    done = 0
    assert sum(sizes) == len(table)
    for n in sizes:
        c.accumulate_lens_device(p, total, aperture, focus, np.ascontiguousarray(table[done:done + n]), done, mean=mean, rgb8=rgb8)
        done += n
    torch.cuda.synchronize()
    return (total.cpu().numpy(), mean.cpu().numpy() if want_mean else None, rgb8.cpu().numpy() if want_bytes else None)


# ---------------------------------------------------------------- 1. passes over slices are one lens launch
@pytest.mark.parametrize("name,depth", SCENES)
def test_passes_over_slices_are_the_lens_frame_byte_for_byte(pkg, ctx, Y, name, depth):
    """The sum buffer holds NaN beforehand: a first pass that read it, or began from 0. +, or folded in another order than the
    lens kernel, would not give the lens frame's bytes."""
    aperture, focus = LENS[name]
    GL.upload(ctx, Y.scene(name)[0])
    for what, table in (("library table", ctx.lens_table(16)), ("sequence", ctx.lens_sequence(0, 16))):
        lens = GL.lens_frame(pkg, ctx, 32, 32, depth, aperture, focus, table, fill=NAN)
        assert not np.isnan(lens).any()
        for sizes in ((4, 4, 4, 4), (5, 7, 4), (1,) * 16):
            total, mean, _ = run_passes(pkg, ctx, 32, 32, depth, aperture, focus, table, sizes)
            assert mean.tobytes() == lens.tobytes(), "%s, %s, passes %s: %d pixels differ" % (name, what, sizes, int((mean != lens).any(axis=2).sum()))
            assert not np.isnan(total).any()
    for what, table in (("library table", ctx.lens_table(64)), ("sequence", ctx.lens_sequence(0, 64))):
        lens = GL.lens_frame(pkg, ctx, 32, 32, depth, aperture, focus, table, fill=NAN)
        _, mean, _ = run_passes(pkg, ctx, 32, 32, depth, aperture, focus, table, (64,))
        assert mean.tobytes() == lens.tobytes(), "%s, %s, one pass of 64" % (name, what)


# ---------------------------------------------------------------- 2. more samples than a lens frame can hold
@pytest.mark.parametrize("name,depth", [("demo", 3), ("synthetic256", 6)])
def test_200_samples_in_five_passes_match_the_yardstick(pkg, ctx, Y, name, depth):
    aperture, focus = LENS[name]
    GL.upload(ctx, Y.scene(name)[0])
    table = ctx.lens_sequence(0, 200)
    assert table.tobytes() == PR.lens_sequence(0, 200).tobytes()
    total, mean, _ = run_passes(pkg, ctx, 32, 32, depth, aperture, focus, table, (40,) * 5)
    ref_sum, ref_mean = Y.progressive(name, 32, 32, depth, aperture, focus, table, (40,) * 5)
    d_mean, d_sum = GL.worst(mean, ref_mean), GL.worst(total, ref_sum)
    print("%s depth %d, 5 x 40 samples: max |delta| mean %.3e, sum %.3e" % (name, depth, d_mean, d_sum))
    assert not np.isnan(mean).any() and not np.isnan(total).any()
    assert d_mean < TIGHT and d_sum < 200 * TIGHT


# ---------------------------------------------------------------- 3. the display bytes
def test_bytes_are_to_vec_of_the_mean(pkg, ctx, Y):
    """The demo's frame has channels above 1 (the highlights) and at 0: both ends of the clamp are exercised."""
    aperture, focus = LENS["demo"]
    GL.upload(ctx, Y.scene("demo")[0])
    table = ctx.lens_sequence(0, 200)
    _, ref_mean = Y.progressive("demo", 32, 32, 3, aperture, focus, table, (40,) * 5)
    assert (ref_mean > 1.).any(), "no channel above 1: the clamp has nothing to do"
    _, mean, rgb8 = run_passes(pkg, ctx, 32, 32, 3, aperture, focus, table, (40,) * 5)
    assert (mean > 1.).any()
    assert rgb8.tobytes() == PR.to_bytes(mean).tobytes()
    off = np.abs(rgb8.astype(np.int32) - PR.to_bytes(ref_mean).astype(np.int32))
    print("demo, 200 samples: %d of %d bytes differ from the yardstick's (by at most %d)" % (int((off > 0).sum()), off.size, int(off.max())))
    assert off.max() <= 1
    # ... after every pass, not only the last: the bytes of a single pass of 3
    _, mean3, rgb3 = run_passes(pkg, ctx, 32, 32, 3, aperture, focus, table[:3], (3,))
    assert rgb3.tobytes() == PR.to_bytes(mean3).tobytes() and rgb3.tobytes() != rgb8.tobytes()


# ---------------------------------------------------------------- 4. the optional outputs
def test_the_sum_does_not_depend_on_the_optional_outputs(pkg, ctx, Y):
    aperture, focus = LENS["demo"]
    GL.upload(ctx, Y.scene("demo")[0])
    table = ctx.lens_sequence(0, 12)
    full = run_passes(pkg, ctx, 32, 32, 3, aperture, focus, table, (5, 7))
    bare = run_passes(pkg, ctx, 32, 32, 3, aperture, focus, table, (5, 7), want_mean=False, want_bytes=False)
    only_mean = run_passes(pkg, ctx, 32, 32, 3, aperture, focus, table, (5, 7), want_bytes=False)
    only_bytes = run_passes(pkg, ctx, 32, 32, 3, aperture, focus, table, (5, 7), want_mean=False)
    assert bare[0].tobytes() == full[0].tobytes() and not np.isnan(full[0]).any()
    assert only_mean[0].tobytes() == full[0].tobytes() and only_mean[1].tobytes() == full[1].tobytes()
    assert only_bytes[0].tobytes() == full[0].tobytes() and only_bytes[2].tobytes() == full[2].tobytes()


# ---------------------------------------------------------------- 5. idle lanes
def test_idle_lanes_leave_nothing_unwritten(pkg, ctx, Y):
    """5 samples: P = 12 pixels a group, four idle lanes a wave; 7: P = 9, one idle lane; 1,024 pixels are no multiple of either,
    so the last group has idle pixels too."""
    assert 1024 % (64 // 5) and 1024 % (64 // 7)
    aperture, focus = LENS["demo"]
    GL.upload(ctx, Y.scene("demo")[0])
    table = ctx.lens_sequence(0, 12)
    total, mean, rgb8 = run_passes(pkg, ctx, 32, 32, 3, aperture, focus, table, (5, 7))
    ref_sum, ref_mean = Y.progressive("demo", 32, 32, 3, aperture, focus, table, (5, 7))
    assert not np.isnan(total).any() and not np.isnan(mean).any()
    assert GL.worst(mean, ref_mean) < TIGHT and GL.worst(total, ref_sum) < 12 * TIGHT
    assert rgb8.tobytes() == PR.to_bytes(mean).tobytes()             # (no BYTE left but where the mean says so)
    # the first pass alone: its mean and bytes are there before the second overwrites them
    _, mean5, rgb5 = run_passes(pkg, ctx, 32, 32, 3, aperture, focus, table[:5], (5,))
    assert not np.isnan(mean5).any() and rgb5.tobytes() == PR.to_bytes(mean5).tobytes()
    assert GL.worst(mean5, Y.progressive("demo", 32, 32, 3, aperture, focus, table[:5], (5,))[1]) < TIGHT


# ---------------------------------------------------------------- 6. the rows a pass leaves alone
def test_rows_below_the_last_patch_row_and_the_memory_behind_the_buffers_keep_their_bytes(pkg, ctx, Y):
    """32 x 40: rows = 32.  The three buffers, their eight last rows and a guard region behind each hold NaN / BYTE beforehand."""
    import torch
    aperture, focus = LENS["demo"]
    GL.upload(ctx, Y.scene("demo")[0])
    p = pkg.backend.make_params(workloads.FOV, 40., 32., 3)
    n, guard = 40 * 32 * 3, 4096
    bufs = [torch.full((n + guard,), NAN, dtype=torch.float64, device="cuda:0"), torch.full((n + guard,), NAN, dtype=torch.float64, device="cuda:0"),
            torch.full((n + guard,), BYTE, dtype=torch.uint8, device="cuda:0")]
    before = [b.cpu().numpy().copy() for b in bufs]
    total, mean, rgb8 = (b[:n].view(40, 32, 3) for b in bufs)
    table = ctx.lens_sequence(0, 12)
    ctx.accumulate_lens_device(p, total, aperture, focus, table[:7], 0, mean=mean, rgb8=rgb8)
    ctx.accumulate_lens_device(p, total, aperture, focus, table[7:], 7, mean=mean, rgb8=rgb8)
    torch.cuda.synchronize()
    after = [b.cpu().numpy() for b in bufs]
    got = [a[:n].reshape(40, 32, 3) for a in after]
    ref_sum, ref_mean = Y.progressive("demo", 32, 40, 3, aperture, focus, table, (7, 5))
    assert GL.worst(got[0][:32], ref_sum[:32]) < 12 * TIGHT and GL.worst(got[1][:32], ref_mean[:32]) < TIGHT
    assert got[2][:32].tobytes() == PR.to_bytes(got[1][:32]).tobytes()
    for a, b in zip(after, before):
        assert a[32 * 32 * 3:].tobytes() == b[32 * 32 * 3:].tobytes()  # rows 32-39 and the guard, bit for bit
    # the host path copies the rows [0, 32) only
    host, host8 = np.full((40, 32, 3), -3.5), np.full((40, 32, 3), 7, np.uint8)
    ctx.render_progressive(p, aperture, focus, 7, restart=True, host_rgb=host, host_rgb8=host8)
    _, n_total = ctx.render_progressive(p, aperture, focus, 5, host_rgb=host, host_rgb8=host8)
    assert n_total == 12
    assert host[:32].tobytes() == got[1][:32].tobytes() and np.all(host[32:] == -3.5)
    assert host8[:32].tobytes() == got[2][:32].tobytes() and np.all(host8[32:] == 7)


# ---------------------------------------------------------------- 7. the grid
def test_a_capped_grid_changes_nothing(pkg, ctx, Y, monkeypatch):
    """RM_LENS_MAX_BLOCKS = 1 and 3 (read at rm_init: contexts of their own) cap this kernel's grid too and drive its loop over
    the groups and its tail."""
    aperture, focus = LENS["demo"]
    scene = Y.scene("demo")[0]
    GL.upload(ctx, scene)
    table = ctx.lens_sequence(0, 86)
    plans = ((1, 1), (5, 7), (16, 4), (64, 22))
    free = {s: run_passes(pkg, ctx, 32, 32, 3, aperture, focus, table[:sum(s)], s) for s in plans}
    for cap in (1, 3):
        monkeypatch.setenv("RM_LENS_MAX_BLOCKS", str(cap))
        c = pkg.backend.Context(0)
        try:
            c.upload(scene.flatten())
            for s in plans:
                got = run_passes(pkg, c, 32, 32, 3, aperture, focus, table[:sum(s)], s)
                for a, b, what in zip(got, free[s], ("sum", "mean", "bytes")):
                    assert a.tobytes() == b.tobytes(), "%d workgroup(s), passes %s: %s" % (cap, s, what)
        finally:
            c.close()


# ---------------------------------------------------------------- 8. the oriented context
def test_oriented_context(pkg, ctx, Y):
    scene = Y.scene("demo")[0]
    GL.upload(ctx, scene)
    try:
        lo, hi = GQ.bounds_of(scene.flatten().desc())
        pos, _, _ = ctx.camera()
        eye = np.array([pos.x, pos.y, pos.z]) + np.array([0.12, 0.06, 0.]) * np.linalg.norm(hi - lo)
        ctx.look_at(tuple(eye), tuple((lo + hi) / 2.))
        pos, basis, on = ctx.camera()
        assert on
        view = ((pos.x, pos.y, pos.z), RR.basis_tuple(basis))
        focus = float(np.linalg.norm((lo + hi) / 2. - eye))
        table = ctx.lens_sequence(0, 8)
        total, mean, rgb8 = run_passes(pkg, ctx, 32, 32, 3, LR.APERTURE, focus, table, (4, 4))
        ref_sum, ref_mean = Y.progressive("demo", 32, 32, 3, LR.APERTURE, focus, table, (4, 4), view)
        plain = Y.progressive("demo", 32, 32, 3, LR.APERTURE, focus, table, (4, 4))[1]
        print("demo from the side, 2 x 4 samples: max |delta| mean %.3e, sum %.3e" % (GL.worst(mean, ref_mean), GL.worst(total, ref_sum)))
        assert GL.worst(mean, ref_mean) < TIGHT and GL.worst(total, ref_sum) < 8 * TIGHT
        assert GL.worst(ref_mean, plain) > 0.05                        # ... and it is another picture than the fixed view's
        assert rgb8.tobytes() == PR.to_bytes(mean).tobytes()
    finally:
        ctx.orient(None)


# ---------------------------------------------------------------- 9. aperture 0 is the supersampled frame
@pytest.mark.parametrize("name,depth", [("demo", 3), ("synthetic256", 6)])
def test_aperture_0_in_two_passes_is_the_refine_kernels_frame_byte_for_byte(pkg, ctx, Y, name, depth):
    import torch
    GL.upload(ctx, Y.scene(name)[0])
    p = pkg.backend.make_params(workloads.FOV, 32., 32., depth)
    dev = torch.zeros((32, 32, 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.render_device(p, dev.data_ptr())
    torch.cuda.synchronize()
    ws = ctx.refine_device(p, dev, 2, -1.)
    torch.cuda.synchronize()
    assert int(ws[0]) == 32 * 32
    refined = dev.cpu().numpy()
    table = LR.supersample_table(2)                                   # (i/2, j/2, 0, 0), j outer and i inner
    _, mean, _ = run_passes(pkg, ctx, 32, 32, depth, 0., LR.FOCUS, table, (2, 2))
    assert mean.tobytes() == refined.tobytes(), "%d pixels differ" % int((mean != refined).any(axis=2).sum())


# ---------------------------------------------------------------- 10. the host path
CPP_MAIN = r"""
#include <cstdio>
#include "rusty_marcher.hpp"
using namespace rusty_marcher;
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    scene::Scene sc = scene::Scene::create_default();
    framebuffer::FrameBuffer fb = framebuffer::create_frame_buffer(32, 32);
    renderer::Renderer r = renderer::create_renderer(1.5, 32., 32.);
    for (int k = 0; k < 3; k++) {
        r.render_progressive(fb, sc, 0.4, 5., 8u);
        std::printf("samples %u\n", r.last_samples);
    }
    std::FILE *f = std::fopen(argv[1], "wb");
    if (!f) return 3;
    for (const auto &row : fb.buffer) std::fwrite(row.data(), sizeof(Vec3f), row.size(), f);
    std::fclose(f);
    r.render_progressive(fb, sc, 0.4, 5., 8u, true);
    std::printf("restarted %u\n", r.last_samples);
    std::printf("kernel %.6f ms\n", r.last_timing.kernel_ms);
    return 0;
}
"""


def test_host_path_python_and_the_cpp_mirror(pkg, entry, ctx, Y, capsys, tmp_path):
    assert workloads.FOV == 1.5 and (LR.APERTURE, LR.FOCUS) == (0.4, 5.)
    L, B = pkg.lib(), pkg._lib
    scene = Y.scene("demo")[0]
    GL.upload(ctx, scene)
    _, device, device8 = run_passes(pkg, ctx, 32, 32, 3, LR.APERTURE, LR.FOCUS, ctx.lens_sequence(0, 24), (8, 8, 8))
    p = pkg.backend.make_params(workloads.FOV, 32., 32., 3)
    host, host8 = np.full((32, 32, 3), -3.5), np.full((32, 32, 3), 7, np.uint8)

    def tick(params=p, aperture=LR.APERTURE, restart=False, **kw):
        return ctx.render_progressive(params, aperture, LR.FOCUS, 8, restart, **kw)[1]

    # rm_render_progressive: three ticks of 8
    assert tick(restart=True) == 8 and tick() == 16
    timing, total = ctx.render_progressive(p, LR.APERTURE, LR.FOCUS, 8, host_rgb=host, host_rgb8=host8)
    assert total == 24 and host.tobytes() == device.tobytes() and host8.tobytes() == device8.tobytes()
    assert timing.kernel_ms > 0. and timing.total_ms >= timing.kernel_ms
    # what begins the frame again, one at a time (each followed by a tick that goes on: 16)
    assert tick(restart=True) == 8 and tick() == 16
    pos, _, _ = ctx.camera()
    ctx.set_camera((pos.x + 0.25, pos.y, pos.z))
    assert tick() == 8 and tick() == 16
    ctx.look_at((pos.x + 0.25, pos.y, pos.z), (0., 0., -10.))
    assert ctx.camera()[2] and tick() == 8 and tick() == 16
    ctx.orient(None)
    assert tick() == 8 and tick() == 16
    assert tick(aperture=0.5) == 8 and tick(aperture=0.5) == 16
    deeper = pkg.backend.make_params(workloads.FOV, 32., 32., 4)
    assert tick(params=deeper) == 8 and tick(params=deeper) == 16
    ctx.upload(Y.scene("cornell")[0].flatten())
    assert tick(params=deeper) == 8 and tick(params=deeper) == 16
    # ... and what does not: the identical scene again, RM_FLAG_FAST_FP, a refused call in between
    ctx.upload(Y.scene("cornell")[0].flatten())
    assert tick(params=deeper) == 24
    deeper.flags = B.RM_FLAG_FAST_FP
    assert tick(params=deeper) == 32
    bad, n_total = B.rm_lens(LR.APERTURE, 0., 8, 0), C.c_uint32(77)
    before = host.copy()
    st = L.rm_render_progressive(ctx.ptr, C.byref(deeper), C.byref(bad), 0, host.ctypes.data_as(C.POINTER(C.c_double)), None, C.byref(n_total), None)
    assert st == B.RM_ERR_INVALID_ARG and b"focus" in L.rm_last_error(ctx.ptr) and n_total.value == 77 and host.tobytes() == before.tobytes()
    assert tick(params=deeper) == 40
    # back to the demo: the frame of the first three ticks again, byte for byte (the sequence starts over)
    GL.upload(ctx, scene)
    assert tick() == 8 and tick() == 16
    again = np.full((32, 32, 3), -3.5)
    assert tick(host_rgb=again) == 24 and again.tobytes() == device.tobytes()
    # Renderer.render_progressive: the prints and the return value of render(), the total in last_samples
    r = pkg.create_renderer(workloads.FOV, 32., 32.)
    fb = pkg.create_frame_buffer(32, 32)
    capsys.readouterr()
    message = r.render_progressive(fb, scene, LR.APERTURE, LR.FOCUS, 8, restart=True)
    out = capsys.readouterr().out
    assert message.startswith("Scene rendered in ") and message in out
    assert "Rendering using patches of size 32, using 1 patches overall" in out and "compute units used" in out
    assert r.last_samples == 8 and r.last_timing.kernel_ms > 0.
    r.render_progressive(fb, scene, LR.APERTURE, LR.FOCUS, 8)
    assert r.last_samples == 16
    r.render_progressive(fb, scene, LR.APERTURE, LR.FOCUS, 8)
    assert r.last_samples == 24 and fb.buffer.tobytes() == device.tobytes()
    r.max_depth = 4
    r.render_progressive(fb, scene, LR.APERTURE, LR.FOCUS, 8)
    assert r.last_samples == 8 and fb.buffer.tobytes() != device.tobytes()
    # the C++ mirror, from compiled code
    src, exe, dump = tmp_path / "tick.cpp", tmp_path / "tick", tmp_path / "tick.f64"
    src.write_text(CPP_MAIN)
    lib_dir = os.path.join(entry.PKG_DIR, "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(entry.ROOT, "include"), "-I", os.path.join(entry.PKG_DIR, "host"),
                           str(src), "-o", str(exe), "-L", lib_dir, "-lrusty_marcher_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath," + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")])
    log = subprocess.check_output([str(exe), str(dump)]).decode()
    assert [l for l in log.splitlines() if l.startswith(("samples", "restarted"))] == ["samples 8", "samples 16", "samples 24", "restarted 8"]
    assert "kernel " in log
    assert np.fromfile(str(dump)).tobytes() == device.tobytes()


# ---------------------------------------------------------------- 11. saturation
def test_a_saturated_frame_stands(pkg, ctx, Y):
    """1,024 ticks of 64 fill the frame to RM_PROGRESSIVE_MAX_SAMPLES; the next tick launches nothing and returns it as it stands."""
    GL.upload(ctx, Y.scene("demo")[0])
    p = pkg.backend.make_params(workloads.FOV, 32., 32., 3)
    assert ctx.render_progressive(p, LR.APERTURE, LR.FOCUS, 64, restart=True)[1] == 64
    for k in range(2, 1024):
        total = ctx.render_progressive(p, LR.APERTURE, LR.FOCUS, 64)[1]
    assert total == 65472
    before, before8 = np.full((32, 32, 3), NAN), np.full((32, 32, 3), BYTE, np.uint8)
    assert ctx.render_progressive(p, LR.APERTURE, LR.FOCUS, 64, host_rgb=before, host_rgb8=before8)[1] == 65536 == PR.MAX_SAMPLES
    assert not np.isnan(before).any() and before8.tobytes() == PR.to_bytes(before).tobytes()
    for n in (64, 1):
        after, after8 = np.full((32, 32, 3), NAN), np.full((32, 32, 3), BYTE, np.uint8)
        timing, total = ctx.render_progressive(p, LR.APERTURE, LR.FOCUS, n, host_rgb=after, host_rgb8=after8)
        assert total == 65536 and timing.kernel_ms == 0.
        assert after.tobytes() == before.tobytes() and after8.tobytes() == before8.tobytes()
    assert ctx.render_progressive(p, LR.APERTURE, LR.FOCUS, 64)[1] == 65536   # both outputs NULL
    assert ctx.render_progressive(p, LR.APERTURE, LR.FOCUS, 64, restart=True)[1] == 64


# ---------------------------------------------------------------- 12. state
def test_progressive_calls_leave_the_render_state_alone(pkg):
    import torch
    demo = workloads.product_scene(pkg, "demo")
    p = pkg.backend.make_params(workloads.FOV, 1080., 1920., 5)
    small = pkg.backend.make_params(workloads.FOV, 64., 64., 5)

    def frames(with_progressive):
        c = pkg.backend.Context(0)
        try:
            c.upload(demo.flatten())
            out = []
            if with_progressive:
                total = torch.zeros((1080, 1920, 3), dtype=torch.float64, device="cuda:0")
                rgb8 = torch.zeros((1080, 1920, 3), dtype=torch.uint8, device="cuda:0")
            for k in range(3):
                f = np.zeros((1080, 1920, 3))
                c.render(p, f)
                out.append(f)
                if with_progressive and k < 2:                       # before, between and after: progressive calls behind frames 1 and 2
                    before = (c.uploads(), c.launch_stats())
                    c.accumulate_lens_device(p, total, LR.APERTURE, LR.FOCUS, c.lens_sequence(2 * k, 2), 2 * k, rgb8=rgb8)
                    torch.cuda.synchronize()
                    host = np.zeros((64, 64, 3))
                    assert c.render_progressive(small, LR.APERTURE, LR.FOCUS, 4, host_rgb=host)[1] == 4 * (k + 1)
                    assert bool((total[:1056] != 0.).any()) and bool((rgb8[:1056] != 0).any()) and host.any()
                    assert (c.uploads(), c.launch_stats()) == before
            return out
        finally:
            c.close()

    plain, ticked = frames(False), frames(True)
    for k, (a, b) in enumerate(zip(plain, ticked)):
        assert a.tobytes() == b.tobytes(), "frame %d differs once progressive calls ran" % (k + 1)


# ---------------------------------------------------------------- 13. errors
def test_refusals_leave_the_buffers_alone(pkg, ctx, Y):
    import torch
    L, B = pkg.lib(), pkg._lib
    GL.upload(ctx, Y.scene("demo")[0])
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 3)
    total = torch.full((64, 64, 3), 7.25, dtype=torch.float64, device="cuda:0")
    mean = torch.full((64, 64, 3), 7.25, dtype=torch.float64, device="cuda:0")
    rgb8 = torch.full((64, 64, 3), 7, dtype=torch.uint8, device="cuda:0")
    table = torch.from_numpy(PR.lens_sequence(0, 4)).to("cuda:0")
    host, host8 = np.full((64, 64, 3), 7.25), np.full((64, 64, 3), 7, np.uint8)
    D, U8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    nan, inf = float("nan"), float("inf")
    # a standing frame of 4 samples: a refused call leaves its count alone too
    good = B.rm_lens(LR.APERTURE, LR.FOCUS, 4, 0)
    assert ctx.render_progressive(p, LR.APERTURE, LR.FOCUS, 4, restart=True)[1] == 4
    ticks = [4]

    def untouched():
        torch.cuda.synchronize()
        return bool((total == 7.25).all()) and bool((mean == 7.25).all()) and bool((rgb8 == 7).all()) and np.all(host == 7.25) and np.all(host8 == 7)

    def device_call(c, params, lens, t=table, s=total, m=mean, n_before=4):
        lp = C.byref(lens) if lens is not None else None
        vp = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
        st = L.rm_accumulate_lens_device(c.ptr, C.byref(params), lp, vp(t), n_before, vp(s), vp(m), vp(rgb8), None)
        msg = L.rm_last_error(c.ptr).decode()
        assert st != 0 and untouched()
        return st, msg

    def call(c, params, lens):
        """Both entry points: the same status, the same message, nothing written, the standing frame's count unchanged."""
        st, msg = device_call(c, params, lens)
        n_total = C.c_uint32(77)
        st_h = L.rm_render_progressive(c.ptr, C.byref(params), C.byref(lens) if lens is not None else None, 0, host.ctypes.data_as(D),
                                       host8.ctypes.data_as(U8), C.byref(n_total), None)
        msg_h = L.rm_last_error(c.ptr).decode()
        assert st_h == st and msg_h.replace("rm_render_progressive", "rm_accumulate_lens_device") == msg
        assert n_total.value == 77 and untouched()
        return st, msg

    E = B.RM_ERR_INVALID_ARG
    for aperture in (-1e-9, nan, inf, -inf):
        st, msg = call(ctx, p, B.rm_lens(aperture, LR.FOCUS, 4, 0))
        assert st == E and "aperture" in msg
    for focus in (0., -5., nan, inf):
        st, msg = call(ctx, p, B.rm_lens(LR.APERTURE, focus, 4, 0))
        assert st == E and "focus" in msg
    for n in (0, 65, 2 ** 32 - 1):
        st, msg = call(ctx, p, B.rm_lens(LR.APERTURE, LR.FOCUS, n, 0))
        assert st == E and "n_samples" in msg
    st, msg = call(ctx, p, None)
    assert st == E and "NULL lens" in msg
    for flag in (B.RM_FLAG_U8_COMPACT, B.RM_FLAG_F64_COMPACT, B.RM_FLAG_FAST_FP | B.RM_FLAG_F64_COMPACT):
        p.flags = flag
        assert call(ctx, p, good)[0] == E
    p.flags = 0
    p.patch_row_begin, p.patch_row_end = 0, 1                        # a non-default band
    assert call(ctx, p, good)[0] == E
    p.patch_row_begin, p.patch_row_end = 0, 0
    p.max_depth = 33
    assert call(ctx, p, good)[0] == B.RM_ERR_DEPTH
    p.max_depth = 3
    p.background.y = inf
    st, msg = call(ctx, p, good)
    assert st == E and "background" in msg
    p.background.y = 0.1
    odd = pkg.backend.make_params(workloads.FOV, 64., 100., 3)
    assert call(ctx, odd, good)[0] == B.RM_ERR_DIMENSIONS
    huge = pkg.backend.make_params(workloads.FOV, 65536., 32768., 3)  # rows * frame_width = 2^31: checked before any pointer is touched
    st, msg = call(ctx, huge, good)
    assert st == B.RM_ERR_DIMENSIONS and "2^31" in msg
    fresh = pkg.backend.Context(0)
    try:
        assert call(fresh, p, good)[0] == B.RM_ERR_NO_SCENE
    finally:
        fresh.close()
    # the device call's own: table and sum there, the mean not the sum, the total within the cap
    st, msg = device_call(ctx, p, good, t=None)
    assert st == E and "table" in msg
    st, msg = device_call(ctx, p, good, s=None)
    assert st == E and "sum" in msg
    st, msg = device_call(ctx, p, good, m=total)
    assert st == E and "device_mean == device_sum" in msg
    for n_before, n in ((65533, 4), (65536, 1), (65473, 64), (2 ** 32 - 1, 1), (2 ** 32 - 1, 64)):
        st, msg = device_call(ctx, p, B.rm_lens(LR.APERTURE, LR.FOCUS, n, 0), n_before=n_before)
        assert st == E and "n_before + n_samples" in msg, msg
    # the standing frame went through all that untouched: the next tick goes on from its 4 samples
    assert ctx.render_progressive(p, LR.APERTURE, LR.FOCUS, 4)[1] == 8
    # what is tolerated: the total at the cap exactly; RM_FLAG_FAST_FP (ignored: the kernel is the strict flavour); a frame without
    # a whole patch row
    small = pkg.backend.make_params(workloads.FOV, 32., 32., 3)
    s32 = torch.zeros((32, 32, 3), dtype=torch.float64, device="cuda:0")
    m32 = torch.full((32, 32, 3), NAN, dtype=torch.float64, device="cuda:0")
    ctx.accumulate_lens_device(small, s32, LR.APERTURE, LR.FOCUS, PR.lens_sequence(65532, 4), 65532, mean=m32)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(m32).any())
    table4 = PR.lens_sequence(0, 4)
    strict = run_passes(pkg, ctx, 32, 32, 3, LR.APERTURE, LR.FOCUS, table4, (2, 2))
    fast = run_passes(pkg, ctx, 32, 32, 3, LR.APERTURE, LR.FOCUS, table4, (2, 2), flags=B.RM_FLAG_FAST_FP)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(strict, fast)) and strict[1].any()
    short = run_passes(pkg, ctx, 64, 31, 3, LR.APERTURE, LR.FOCUS, table4, (4,))
    assert np.isnan(short[0]).all() and np.isnan(short[1]).all() and np.all(short[2] == BYTE)   # rows == 0: RM_OK, nothing done
    h31 = np.full((31, 64, 3), 7.25)
    t31, n31 = ctx.render_progressive(pkg.backend.make_params(workloads.FOV, 31., 64., 3), LR.APERTURE, LR.FOCUS, 4, host_rgb=h31)
    assert np.all(h31 == 7.25) and n31 == 0 and t31.kernel_ms == 0.
    assert untouched()
