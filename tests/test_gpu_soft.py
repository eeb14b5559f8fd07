"""Area lights on the GPU (-m gpu): rm_accumulate_soft_device and rm_render_progressive_soft through the C ABI, the Python
bindings and the C++ mirror, against tests/soft_reference.py -- the lens rays in numpy, row s of every pixel cast by the CPU
oracle's cast_ray against the scene with its lights moved by row s of the offset table, folded in table order across passes
(pinned on the CPU by tests/test_soft_abi.py) -- and against the frames of rm_accumulate_lens_device.

What the header calls byte for byte is demanded byte for byte; against the yardstick every channel of every pixel of the rows
a pass writes is demanded within TIGHT = 1e-9 of the mean (n TIGHT of a sum of n samples), no pixel left out.  Largest
deviations observed on an MI355X are recorded in DESIGN.md section 6i."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lens_reference as LR
import progressive_reference as PR
import radiance_reference as RR
import soft_reference as SR
import test_gpu_lens as GL
import test_gpu_progressive as GP
import test_gpu_query as GQ
import workloads

pytestmark = pytest.mark.gpu

TIGHT = SR.TIGHT
NAN, BYTE = GP.NAN, GP.BYTE
# scene -> (depth, radii): depth 6 takes the kernels with STACK = 32, the 256 spheres those with the hierarchy; the penumbra
# scene has lights on opposite sides of its floor and an odd number of them
SCENES = {"demo": (3, (1.5, 3.)), "penumbra": (3, SR.PENUMBRA_RADII), "synthetic256": (6, (1.5, 1.5))}


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_soft"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return SR.Yardstick(pkg, O, orc)


def run_soft(pkg, c, w, h, depth, aperture, focus, table, offsets, sizes, want_mean=True, want_bytes=True):
    """Passes of the sizes `sizes` over consecutive slices of `table` and `offsets` on torch's current stream, the first with
    n_before = 0, into buffers that held NaN (and BYTE) -> (sum, mean, bytes) as numpy, None for what was not asked for."""
    import torch
    p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)
    total = torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda:0")
    mean = torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda:0") if want_mean else None
    rgb8 = torch.full((h, w, 3), BYTE, dtype=torch.uint8, device="cuda:0") if want_bytes else None
    torch.cuda.synchronize()
    done = 0
    assert sum(sizes) == len(table) == len(offsets)
    for n in sizes:
        c.accumulate_soft_device(p, total, aperture, focus, np.ascontiguousarray(table[done:done + n]),
                                 np.ascontiguousarray(offsets[done:done + n]), done, mean=mean, rgb8=rgb8)
        done += n
    torch.cuda.synchronize()
    return (total.cpu().numpy(), mean.cpu().numpy() if want_mean else None, rgb8.cpu().numpy() if want_bytes else None)


# ---------------------------------------------------------------- 1. zero offsets are the plain accumulate
@pytest.mark.parametrize("name,depth", [("demo", 3), ("cornell", 3), ("synthetic256", 6)])
def test_zero_offsets_are_the_plain_accumulate_byte_for_byte(pkg, ctx, Y, name, depth):
    """Two passes of 5 samples: 12 pixels a wave, four idle lanes.  +0. in the first pass, -0. in the second."""
    aperture, focus = GL.LENS[name]
    GL.upload(ctx, Y.scene(name)[0])
    table = ctx.lens_sequence(0, 10)
    zeros = np.zeros((10, Y.n_lights(name), 3))
    zeros[5:] = -0.
    plain = GP.run_passes(pkg, ctx, 32, 32, depth, aperture, focus, table, (5, 5))
    soft = run_soft(pkg, ctx, 32, 32, depth, aperture, focus, table, zeros, (5, 5))
    for a, b, what in zip(soft, plain, ("sum", "mean", "bytes")):
        assert not (what != "bytes" and np.isnan(a).any())
        assert a.tobytes() == b.tobytes(), "%s: %s differs in %d pixels" % (name, what, int((a != b).any(axis=2).sum()))
    assert plain[1].any()


# ---------------------------------------------------------------- 2. parity with the yardstick
@pytest.mark.parametrize("n", [1, 5, 64])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_soft_frames_match_the_yardstick(pkg, ctx, Y, name, n):
    """The library's sequence, and a random offset table that differs for every light and every row: a swapped light, or a lane
    that reads another sample's row, is another picture."""
    depth, radii = SCENES[name]
    GL.upload(ctx, Y.scene(name)[0])
    assert len(radii) == Y.n_lights(name)
    rng = np.random.default_rng(20261900 + n)
    table = ctx.lens_sequence(3, n)
    for aperture in (0., LR.APERTURE):
        hard = GP.run_passes(pkg, ctx, 32, 32, depth, aperture, LR.FOCUS, table, (n,))[1]      # the same table, lights where they stand
        for what, offsets in (("sequence", ctx.light_sequence(3, n, radii)), ("random", SR.random_offsets(rng, n, len(radii)))):
            total, mean, rgb8 = run_soft(pkg, ctx, 32, 32, depth, aperture, LR.FOCUS, table, offsets, (n,))
            ref_sum, ref_mean = Y.soft(name, 32, 32, depth, aperture, LR.FOCUS, table, offsets, (n,))
            d_mean, d_sum = GL.worst(mean, ref_mean), GL.worst(total, ref_sum)
            moved = int((np.abs(ref_mean - hard) > 0.05).any(axis=2).sum())
            print("%s depth %d, %d samples, aperture %g, %s offsets: max |delta| mean %.3e, sum %.3e (%d pixels differ from the hard frame)"
                  % (name, depth, n, aperture, what, d_mean, d_sum, moved))
            assert not np.isnan(mean).any() and not np.isnan(total).any()
            assert d_mean < TIGHT and d_sum < n * TIGHT
            assert rgb8.tobytes() == PR.to_bytes(mean).tobytes()
            assert moved > 0                                          # (the lights did move: not the hard frame again)


# ---------------------------------------------------------------- 3. folding
def test_three_passes_over_slices_are_one_pass_byte_for_byte(pkg, ctx, Y):
    depth, radii = SCENES["penumbra"]
    GL.upload(ctx, Y.scene("penumbra")[0])
    table, offsets = ctx.lens_sequence(0, 12), ctx.light_sequence(0, 12, radii)
    one = run_soft(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table, offsets, (12,))
    three = run_soft(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table, offsets, (5, 4, 3))
    for a, b, what in zip(three, one, ("sum", "mean", "bytes")):
        assert a.tobytes() == b.tobytes(), what
    assert not np.isnan(one[1]).any()
    # the optional outputs change nothing in the sum
    bare = run_soft(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table, offsets, (5, 4, 3), want_mean=False, want_bytes=False)
    assert bare[0].tobytes() == one[0].tobytes()


def test_200_rows_in_five_passes_match_the_yardstick(pkg, ctx, Y):
    depth, radii = SCENES["demo"]
    GL.upload(ctx, Y.scene("demo")[0])
    table, offsets = ctx.lens_sequence(0, 200), ctx.light_sequence(0, 200, radii)
    assert offsets.tobytes() == SR.light_sequence(0, 200, radii).tobytes()
    total, mean, rgb8 = run_soft(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table, offsets, (40,) * 5)
    ref_sum, ref_mean = Y.soft("demo", 32, 32, depth, LR.APERTURE, LR.FOCUS, table, offsets, (40,) * 5)
    d_mean, d_sum = GL.worst(mean, ref_mean), GL.worst(total, ref_sum)
    print("demo depth %d, 5 x 40 samples, radii %s: max |delta| mean %.3e, sum %.3e" % (depth, radii, d_mean, d_sum))
    assert not np.isnan(mean).any() and d_mean < TIGHT and d_sum < 200 * TIGHT
    assert rgb8.tobytes() == PR.to_bytes(mean).tobytes()


# ---------------------------------------------------------------- 4. the oriented context
def test_oriented_context(pkg, ctx, Y):
    depth, radii = SCENES["demo"]
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
        table, offsets = ctx.lens_sequence(0, 8), ctx.light_sequence(0, 8, radii)
        total, mean, _ = run_soft(pkg, ctx, 32, 32, depth, LR.APERTURE, focus, table, offsets, (4, 4))
        ref_sum, ref_mean = Y.soft("demo", 32, 32, depth, LR.APERTURE, focus, table, offsets, (4, 4), view)
        fixed = Y.soft("demo", 32, 32, depth, LR.APERTURE, focus, table, offsets, (4, 4))[1]
        print("demo from the side, 2 x 4 samples: max |delta| mean %.3e, sum %.3e" % (GL.worst(mean, ref_mean), GL.worst(total, ref_sum)))
        assert GL.worst(mean, ref_mean) < TIGHT and GL.worst(total, ref_sum) < 8 * TIGHT
        assert GL.worst(ref_mean, fixed) > 0.05                        # ... and it is another picture than the fixed view's
    finally:
        ctx.orient(None)


# ---------------------------------------------------------------- 5. the grid
def test_a_capped_grid_changes_nothing(pkg, ctx, Y, monkeypatch):
    """RM_LENS_MAX_BLOCKS = 1 and 3 (read at rm_init: contexts of their own) cap this kernel's grid too and drive its loop over
    the groups and its tail."""
    depth, radii = SCENES["penumbra"]
    scene = Y.scene("penumbra")[0]
    GL.upload(ctx, scene)
    table, offsets = ctx.lens_sequence(0, 86), ctx.light_sequence(0, 86, radii)
    plans = ((1, 1), (5, 7), (64, 22))
    free = {s: run_soft(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table[:sum(s)], offsets[:sum(s)], s) for s in plans}
    for cap in (1, 3):
        monkeypatch.setenv("RM_LENS_MAX_BLOCKS", str(cap))
        c = pkg.backend.Context(0)
        try:
            c.upload(scene.flatten())
            for s in plans:
                got = run_soft(pkg, c, 32, 32, depth, LR.APERTURE, LR.FOCUS, table[:sum(s)], offsets[:sum(s)], s)
                for a, b, what in zip(got, free[s], ("sum", "mean", "bytes")):
                    assert a.tobytes() == b.tobytes(), "%d workgroup(s), passes %s: %s" % (cap, s, what)
        finally:
            c.close()


# ---------------------------------------------------------------- 6. the buffers
def test_rows_below_the_last_patch_row_and_the_memory_behind_the_buffers_keep_their_bytes(pkg, ctx, Y):
    """32 x 40: rows = 32.  The three buffers, their eight last rows and a guard region behind each hold NaN / BYTE beforehand;
    the offset table is read from an allocation of exactly its size and from one with NaN rows behind it."""
    import torch
    depth, radii = SCENES["penumbra"]
    GL.upload(ctx, Y.scene("penumbra")[0])
    p = pkg.backend.make_params(workloads.FOV, 40., 32., depth)
    n, guard = 40 * 32 * 3, 4096
    table, offsets = ctx.lens_sequence(0, 12), ctx.light_sequence(0, 12, radii)
    ref_sum, ref_mean = Y.soft("penumbra", 32, 40, depth, LR.APERTURE, LR.FOCUS, table, offsets, (7, 5))

    def run(guarded_offsets):
        bufs = [torch.full((n + guard,), NAN, dtype=torch.float64, device="cuda:0"), torch.full((n + guard,), NAN, dtype=torch.float64, device="cuda:0"),
                torch.full((n + guard,), BYTE, dtype=torch.uint8, device="cuda:0")]
        before = [b.cpu().numpy().copy() for b in bufs]
        total, mean, rgb8 = (b[:n].view(40, 32, 3) for b in bufs)
        done = 0
        for k in (7, 5):
            exact = torch.from_numpy(np.ascontiguousarray(offsets[done:done + k])).to("cuda:0")     # k x 3 x 3 doubles, no more
            assert exact.numel() == k * len(radii) * 3
            if guarded_offsets:
                wide = torch.full((k + 64, len(radii), 3), NAN, dtype=torch.float64, device="cuda:0")
                wide[:k] = exact
                exact = wide[:k]
            assert exact.is_contiguous()
            ctx.accumulate_soft_device(p, total, LR.APERTURE, LR.FOCUS, table[done:done + k], exact, done, mean=mean, rgb8=rgb8)
            done += k
        torch.cuda.synchronize()
        after = [b.cpu().numpy() for b in bufs]
        for a, b in zip(after, before):
            assert a[32 * 32 * 3:].tobytes() == b[32 * 32 * 3:].tobytes()  # rows 32-39 and the guard, bit for bit
        return [a[:n].reshape(40, 32, 3)[:32] for a in after]

    got = run(False)
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()      # no pixel of [0, rows) left unwritten
    assert GL.worst(got[0], ref_sum[:32]) < 12 * TIGHT and GL.worst(got[1], ref_mean[:32]) < TIGHT
    assert got[2].tobytes() == PR.to_bytes(got[1]).tobytes()
    for a, b, what in zip(run(True), got, ("sum", "mean", "bytes")):
        assert a.tobytes() == b.tobytes(), "NaN rows behind the offset table changed the %s" % what
    # the host path copies the rows [0, 32) only
    host, host8 = np.full((40, 32, 3), -3.5), np.full((40, 32, 3), 7, np.uint8)
    ctx.render_progressive_soft(p, radii, LR.APERTURE, LR.FOCUS, 7, restart=True, host_rgb=host, host_rgb8=host8)
    _, n_total = ctx.render_progressive_soft(p, radii, LR.APERTURE, LR.FOCUS, 5, host_rgb=host, host_rgb8=host8)
    assert n_total == 12
    assert host[:32].tobytes() == got[1].tobytes() and np.all(host[32:] == -3.5)
    assert host8[:32].tobytes() == got[2].tobytes() and np.all(host8[32:] == 7)


# ---------------------------------------------------------------- 7. the host path
CPP_MAIN = r"""
#include <cstdio>
#include "rusty_marcher.hpp"
using namespace rusty_marcher;
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    scene::Scene sc = scene::Scene::create_default();
    framebuffer::FrameBuffer fb = framebuffer::create_frame_buffer(32, 32);
    renderer::Renderer r = renderer::create_renderer(1.5, 32., 32.);
    const std::vector<double> radii{1.5, 3.};
    for (int k = 0; k < 3; k++) {
        r.render_progressive_soft(fb, sc, radii, 0.4, 5., 8u);
        std::printf("samples %u\n", r.last_samples);
    }
    std::FILE *f = std::fopen(argv[1], "wb");
    if (!f) return 3;
    for (const auto &row : fb.buffer) std::fwrite(row.data(), sizeof(Vec3f), row.size(), f);
    std::fclose(f);
    r.render_progressive(fb, sc, 0.4, 5., 8u);
    std::printf("plain %u\n", r.last_samples);
    r.render_progressive_soft(fb, sc, radii, 0.4, 5., 8u);
    std::printf("soft %u\n", r.last_samples);
    r.render_progressive_soft(fb, sc, {1.5, 2.}, 0.4, 5., 8u);
    std::printf("radius %u\n", r.last_samples);
    return 0;
}
"""


def test_host_path_c_python_and_the_cpp_mirror(pkg, entry, ctx, Y, capsys, tmp_path):
    assert workloads.FOV == 1.5 and (LR.APERTURE, LR.FOCUS) == (0.4, 5.)
    L, B = pkg.lib(), pkg._lib
    depth, radii = SCENES["demo"]
    scene = Y.scene("demo")[0]
    GL.upload(ctx, scene)
    table, offsets = ctx.lens_sequence(0, 24), ctx.light_sequence(0, 24, radii)
    _, device, device8 = run_soft(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table, offsets, (8, 8, 8))
    ref_mean = Y.soft("demo", 32, 32, depth, LR.APERTURE, LR.FOCUS, table, offsets, (8, 8, 8))[1]
    assert GL.worst(device, ref_mean) < TIGHT                         # rows [N, N + 8) of both sequences, tick after tick
    p = pkg.backend.make_params(workloads.FOV, 32., 32., depth)
    host, host8 = np.full((32, 32, 3), -3.5), np.full((32, 32, 3), 7, np.uint8)

    def soft(r=radii, restart=False, **kw):
        return ctx.render_progressive_soft(p, r, LR.APERTURE, LR.FOCUS, 8, restart, **kw)[1]

    def plain(restart=False, **kw):
        return ctx.render_progressive(p, LR.APERTURE, LR.FOCUS, 8, restart, **kw)[1]

    # three ticks of 8 with the same radii: the frame goes on, and is the device call's
    assert soft(restart=True) == 8 and soft() == 16
    timing, total = ctx.render_progressive_soft(p, radii, LR.APERTURE, LR.FOCUS, 8, host_rgb=host, host_rgb8=host8)
    assert total == 24 and host.tobytes() == device.tobytes() and host8.tobytes() == device8.tobytes()
    assert timing.kernel_ms > 0. and timing.total_ms >= timing.kernel_ms
    # the same through the C entry point itself
    r64 = np.ascontiguousarray(radii, dtype=np.float64)
    lens, n_total, again = B.rm_lens(LR.APERTURE, LR.FOCUS, 8, 0), C.c_uint32(0), np.full((32, 32, 3), -3.5)
    D = C.POINTER(C.c_double)
    for k in range(3):
        st = L.rm_render_progressive_soft(ctx.ptr, C.byref(p), C.byref(lens), r64.ctypes.data_as(D), 2, 1 if k == 0 else 0,
                                          again.ctypes.data_as(D), None, C.byref(n_total), None)
        assert st == 0 and n_total.value == 8 * (k + 1)
    assert again.tobytes() == device.tobytes()
    # what begins the frame again, one at a time (each followed by a tick that goes on: 16)
    assert soft((1.5, 2.)) == 8 and soft((1.5, 2.)) == 16             # a changed radius
    assert soft() == 8 and soft() == 16                               # ... and back
    assert plain() == 8 and plain() == 16                             # soft -> plain
    hard = np.full((32, 32, 3), -3.5)
    assert plain(host_rgb=hard) == 24
    assert hard.tobytes() == GP.run_passes(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table, (8, 8, 8))[1].tobytes()
    assert soft() == 8 and soft() == 16                               # plain -> soft
    assert soft(restart=True) == 8 and soft() == 16                   # restart
    assert soft((0., 0.)) == 8                                        # radii of zero are radii: not the plain call's frame
    assert plain() == 8
    # ... and the frame of the first three ticks again, byte for byte (both sequences start over)
    assert soft() == 8 and soft() == 16
    again.fill(-3.5)
    assert soft(host_rgb=again) == 24 and again.tobytes() == device.tobytes()
    # a refused call in between changes neither the count nor the key
    for bad_radii, n_lights in (((1.5, -1.), 2), ((1.5, NAN), 2), ((1.5, 3., 1.), 3), ((1.5,), 1)):
        b64, before = np.ascontiguousarray(bad_radii, dtype=np.float64), again.copy()
        n_total.value = 77
        st = L.rm_render_progressive_soft(ctx.ptr, C.byref(p), C.byref(lens), b64.ctypes.data_as(D), n_lights, 0, again.ctypes.data_as(D), None,
                                          C.byref(n_total), None)
        assert st == B.RM_ERR_INVALID_ARG and n_total.value == 77 and again.tobytes() == before.tobytes()
        assert (b"radii" in L.rm_last_error(ctx.ptr)) or (b"n_lights" in L.rm_last_error(ctx.ptr))
    assert soft() == 32
    # Renderer.render_progressive_soft and render_soft_shadows: the prints and the return value of render()
    r = pkg.create_renderer(workloads.FOV, 32., 32.)
    r.max_depth = depth
    fb = pkg.create_frame_buffer(32, 32)
    capsys.readouterr()
    message = r.render_progressive_soft(fb, scene, radii, LR.APERTURE, LR.FOCUS, 8, restart=True)
    out = capsys.readouterr().out
    assert message.startswith("Scene rendered in ") and message in out and "compute units used" in out
    assert r.last_samples == 8 and r.last_timing.kernel_ms > 0.
    first = fb.buffer.copy()
    r.render_progressive_soft(fb, scene, radii, LR.APERTURE, LR.FOCUS, 8)
    r.render_progressive_soft(fb, scene, radii, LR.APERTURE, LR.FOCUS, 8)
    assert r.last_samples == 24 and fb.buffer.tobytes() == device.tobytes()
    r.render_soft_shadows(fb, scene, radii, 8, LR.APERTURE, LR.FOCUS)    # one restarted tick
    assert r.last_samples == 8 and fb.buffer.tobytes() == first.tobytes()
    r.render_soft_shadows(fb, scene, radii, 8)                           # ... through a pinhole by default
    pinhole = run_soft(pkg, ctx, 32, 32, depth, 0., 1., table[:8], offsets[:8], (8,))[1]
    assert r.last_samples == 8 and fb.buffer.tobytes() == pinhole.tobytes()
    # the C++ mirror, from compiled code
    src, exe, dump = tmp_path / "tick.cpp", tmp_path / "tick", tmp_path / "tick.f64"
    src.write_text(CPP_MAIN)
    lib_dir = os.path.join(entry.PKG_DIR, "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(entry.ROOT, "include"), "-I", os.path.join(entry.PKG_DIR, "host"),
                           str(src), "-o", str(exe), "-L", lib_dir, "-lrusty_marcher_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath," + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")])
    log = subprocess.check_output([str(exe), str(dump)]).decode()
    assert [l for l in log.splitlines() if l.split()[0] in ("samples", "plain", "soft", "radius")] == \
        ["samples 8", "samples 16", "samples 24", "plain 8", "soft 8", "radius 8"]
    assert np.fromfile(str(dump)).tobytes() == device.tobytes()


def test_a_saturated_frame_stands(pkg, ctx, Y):
    """1,024 ticks of 64 fill the frame to RM_PROGRESSIVE_MAX_SAMPLES; the next tick launches nothing and returns it as it stands."""
    depth, radii = SCENES["demo"]
    GL.upload(ctx, Y.scene("demo")[0])
    p = pkg.backend.make_params(workloads.FOV, 32., 32., depth)
    assert ctx.render_progressive_soft(p, radii, 0., LR.FOCUS, 64, restart=True)[1] == 64
    for k in range(2, 1024):
        total = ctx.render_progressive_soft(p, radii, 0., LR.FOCUS, 64)[1]
    assert total == 65472
    before, before8 = np.full((32, 32, 3), NAN), np.full((32, 32, 3), BYTE, np.uint8)
    assert ctx.render_progressive_soft(p, radii, 0., LR.FOCUS, 64, host_rgb=before, host_rgb8=before8)[1] == 65536 == SR.MAX_SAMPLES
    assert not np.isnan(before).any() and before8.tobytes() == PR.to_bytes(before).tobytes()
    for n in (64, 1):
        after, after8 = np.full((32, 32, 3), NAN), np.full((32, 32, 3), BYTE, np.uint8)
        timing, total = ctx.render_progressive_soft(p, radii, 0., LR.FOCUS, n, host_rgb=after, host_rgb8=after8)
        assert total == 65536 and timing.kernel_ms == 0.
        assert after.tobytes() == before.tobytes() and after8.tobytes() == before8.tobytes()
    assert ctx.render_progressive_soft(p, radii, 0., LR.FOCUS, 64, restart=True)[1] == 64


# ---------------------------------------------------------------- 8. state
def test_soft_calls_leave_the_render_state_alone(pkg):
    import torch
    demo = workloads.product_scene(pkg, "demo")
    radii = SCENES["demo"][1]
    p = pkg.backend.make_params(workloads.FOV, 480., 640., 5)
    small = pkg.backend.make_params(workloads.FOV, 64., 64., 5)

    def frames(with_soft):
        c = pkg.backend.Context(0)
        try:
            c.upload(demo.flatten())
            out = []
            if with_soft:
                total = torch.zeros((480, 640, 3), dtype=torch.float64, device="cuda:0")
                rgb8 = torch.zeros((480, 640, 3), dtype=torch.uint8, device="cuda:0")
            for k in range(3):
                f = np.zeros((480, 640, 3))
                c.render(p, f)
                out.append(f)
                if with_soft and k < 2:                              # before, between and after: soft calls behind frames 1 and 2
                    before = (c.uploads(), c.launch_stats())
                    c.accumulate_soft_device(p, total, LR.APERTURE, LR.FOCUS, c.lens_sequence(2 * k, 2), c.light_sequence(2 * k, 2, radii),
                                             2 * k, rgb8=rgb8)
                    torch.cuda.synchronize()
                    host = np.zeros((64, 64, 3))
                    assert c.render_progressive_soft(small, radii, LR.APERTURE, LR.FOCUS, 4, host_rgb=host)[1] == 4 * (k + 1)
                    assert bool((total[:480] != 0.).any()) and bool((rgb8[:480] != 0).any()) and host.any()
                    assert (c.uploads(), c.launch_stats()) == before
            return out
        finally:
            c.close()

    plain, ticked = frames(False), frames(True)
    for k, (a, b) in enumerate(zip(plain, ticked)):
        assert a.tobytes() == b.tobytes(), "frame %d differs once soft calls ran" % (k + 1)


def test_a_plain_progressive_run_is_the_same_with_soft_calls_on_another_context(pkg, ctx, Y):
    depth, radii = SCENES["demo"]
    scene = Y.scene("demo")[0]
    p = pkg.backend.make_params(workloads.FOV, 32., 32., depth)

    def ticks(c, other=None):
        out = []
        for k in range(3):
            host, host8 = np.full((32, 32, 3), NAN), np.full((32, 32, 3), BYTE, np.uint8)
            assert c.render_progressive(p, LR.APERTURE, LR.FOCUS, 8, restart=(k == 0), host_rgb=host, host_rgb8=host8)[1] == 8 * (k + 1)
            out.append((host, host8))
            if other is not None:
                assert other.render_progressive_soft(p, radii, LR.APERTURE, LR.FOCUS, 8)[1] >= 8
        return out

    GL.upload(ctx, scene)
    alone = ticks(ctx)
    other = pkg.backend.Context(0)
    try:
        other.upload(scene.flatten())
        beside = ticks(ctx, other)
    finally:
        other.close()
    for (a, a8), (b, b8) in zip(alone, beside):
        assert a.tobytes() == b.tobytes() and a8.tobytes() == b8.tobytes()
    assert alone[2][0].tobytes() == GP.run_passes(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, ctx.lens_sequence(0, 24), (8, 8, 8))[1].tobytes()


# ---------------------------------------------------------------- 9. errors
def test_refusals_leave_the_buffers_and_the_count_alone(pkg, ctx, Y):
    import torch
    L, B = pkg.lib(), pkg._lib
    depth, radii = SCENES["demo"]
    GL.upload(ctx, Y.scene("demo")[0])
    p = pkg.backend.make_params(workloads.FOV, 64., 64., depth)
    total = torch.full((64, 64, 3), 7.25, dtype=torch.float64, device="cuda:0")
    mean = torch.full((64, 64, 3), 7.25, dtype=torch.float64, device="cuda:0")
    rgb8 = torch.full((64, 64, 3), 7, dtype=torch.uint8, device="cuda:0")
    table = torch.from_numpy(PR.lens_sequence(0, 4)).to("cuda:0")
    offsets = torch.from_numpy(SR.light_sequence(0, 4, radii)).to("cuda:0")
    host, host8 = np.full((64, 64, 3), 7.25), np.full((64, 64, 3), 7, np.uint8)
    D, U8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    good = B.rm_lens(LR.APERTURE, LR.FOCUS, 4, 0)
    r64 = np.ascontiguousarray(radii, dtype=np.float64)
    # a standing frame of 4 samples: a refused call leaves its count alone too
    assert ctx.render_progressive_soft(p, radii, LR.APERTURE, LR.FOCUS, 4, restart=True)[1] == 4

    def untouched():
        torch.cuda.synchronize()
        return bool((total == 7.25).all()) and bool((mean == 7.25).all()) and bool((rgb8 == 7).all()) and np.all(host == 7.25) and np.all(host8 == 7)

    def device_call(lens=good, t=table, o=offsets, n_lights=2, s=total, m=mean, n_before=4, params=p):
        vp = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
        st = L.rm_accumulate_soft_device(ctx.ptr, C.byref(params), C.byref(lens), vp(t), vp(o), n_lights, n_before, vp(s), vp(m), vp(rgb8), None)
        msg = L.rm_last_error(ctx.ptr).decode()
        assert st != 0 and untouched()
        return st, msg

    def host_call(r=r64, n_lights=2, lens=good, params=p):
        n_total = C.c_uint32(77)
        st = L.rm_render_progressive_soft(ctx.ptr, C.byref(params), C.byref(lens), r.ctypes.data_as(D) if r is not None else None, n_lights, 0,
                                          host.ctypes.data_as(D), host8.ctypes.data_as(U8), C.byref(n_total), None)
        msg = L.rm_last_error(ctx.ptr).decode()
        assert st != 0 and n_total.value == 77 and untouched()
        return st, msg

    E = B.RM_ERR_INVALID_ARG
    # the area lights' own
    for n_lights in (0, 1, 3, 2 ** 32 - 1):
        st, msg = device_call(n_lights=n_lights)
        assert st == E and "n_lights" in msg and "the resident scene has 2" in msg
        st, msg = host_call(n_lights=n_lights, r=np.full(4, 1.5))
        assert st == E and "n_lights" in msg
    st, msg = device_call(o=None)
    assert st == E and "NULL offsets" in msg
    st, msg = host_call(r=None)
    assert st == E and "NULL radii" in msg
    for bad in (-1e-9, NAN, float("inf"), -float("inf")):
        st, msg = host_call(r=np.array([1.5, bad]))
        assert st == E and "radii[1]" in msg
    # the progressive frames' own, through the new entry points
    st, msg = device_call(t=None)
    assert st == E and "table" in msg
    st, msg = device_call(s=None)
    assert st == E and "sum" in msg
    st, msg = device_call(m=total)
    assert st == E and "device_mean == device_sum" in msg
    for n_before, n in ((65533, 4), (65536, 1), (2 ** 32 - 1, 64)):
        st, msg = device_call(lens=B.rm_lens(LR.APERTURE, LR.FOCUS, n, 0), n_before=n_before)
        assert st == E and "n_before + n_samples" in msg, msg
    for lens, word in ((B.rm_lens(-1., LR.FOCUS, 4, 0), "aperture"), (B.rm_lens(LR.APERTURE, 0., 4, 0), "focus"), (B.rm_lens(LR.APERTURE, LR.FOCUS, 65, 0), "n_samples")):
        for st, msg in (device_call(lens=lens), host_call(lens=lens)):
            assert st == E and word in msg
    odd = pkg.backend.make_params(workloads.FOV, 64., 100., depth)
    assert device_call(params=odd)[0] == B.RM_ERR_DIMENSIONS and host_call(params=odd)[0] == B.RM_ERR_DIMENSIONS
    fresh = pkg.backend.Context(0)
    try:
        n_total = C.c_uint32(77)
        assert L.rm_render_progressive_soft(fresh.ptr, C.byref(p), C.byref(good), r64.ctypes.data_as(D), 2, 0, None, None, C.byref(n_total),
                                            None) == B.RM_ERR_NO_SCENE and n_total.value == 77
    finally:
        fresh.close()
    # the Python wrapper hands the library's refusal on
    with pytest.raises(B.BackendError, match="n_lights"):
        ctx.render_progressive_soft(p, (1.5, 1.5, 1.5), LR.APERTURE, LR.FOCUS, 4)
    # the standing frame went through all that untouched: the next tick goes on from its 4 samples
    assert ctx.render_progressive_soft(p, radii, LR.APERTURE, LR.FOCUS, 4)[1] == 8
    # what is tolerated: a frame without a whole patch row; a scene without lights and a NULL table
    small = pkg.backend.make_params(workloads.FOV, 32., 32., depth)
    short = run_soft(pkg, ctx, 64, 31, depth, LR.APERTURE, LR.FOCUS, PR.lens_sequence(0, 4), SR.light_sequence(0, 4, radii), (4,))
    assert np.isnan(short[0]).all() and np.isnan(short[1]).all() and np.all(short[2] == BYTE)   # rows == 0: RM_OK, nothing done
    dark = pkg.Scene.new()
    dark.shapes.append(pkg.sphere.create(pkg.Vec3f(0., 0., -6.), 2., pkg.Reflectance(**RR.GLASS)))
    c = pkg.backend.Context(0)
    try:
        c.upload(dark.flatten())
        none = run_soft(pkg, c, 32, 32, depth, 0., LR.FOCUS, PR.lens_sequence(0, 4), np.zeros((4, 0, 3)), (4,))
        lens_only = GP.run_passes(pkg, c, 32, 32, depth, 0., LR.FOCUS, PR.lens_sequence(0, 4), (4,))
        assert none[1].tobytes() == lens_only[1].tobytes() and not np.isnan(none[1]).any()
        assert c.render_progressive_soft(small, (), 0., LR.FOCUS, 4)[1] == 4
    finally:
        c.close()
    assert untouched()
