"""Converging frames on the GPU (-m gpu): rm_accumulate_converging_device and rm_render_converging through the C ABI, the Python
bindings and the C++ mirror, against the frames of rm_accumulate_lens_device / rm_accumulate_soft_device and against
tests/converge_reference.py -- the select rule and the fold in numpy over every row of the sequences for every pixel, cast by
the CPU oracle (pinned on the CPU by tests/test_converge_abi.py, which also shows that no decision of these cases is close).

What the header calls byte for byte is demanded byte for byte.  Against the yardstick masks, lists (as sets) and counts are
demanded exactly, every channel of the mean within TIGHT = 1e-9, of the sum within n TIGHT, Y within 3 n TIGHT and Q within
6 n (ymax + 1.5 TIGHT) TIGHT (converge_reference.py has the derivation), no pixel left out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import converge_reference as CR
import lens_reference as LR
import progressive_reference as PR
import radiance_reference as RR
import soft_reference as SR
import test_gpu_lens as GL
import test_gpu_progressive as GP
import test_gpu_query as GQ
import workloads

pytestmark = pytest.mark.gpu

TIGHT = CR.TIGHT
NAN, BYTE = GP.NAN, GP.BYTE
WORD = 0x5a5a5a5a                                                      # what a count or a workspace holds beforehand


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_converge"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return CR.Yardstick(pkg, O, orc)


class Frame:
    """The device buffers of a converging frame, h x w, each with `guard` elements behind it; everything holds NaN / BYTE /
    WORD beforehand."""

    def __init__(self, pkg, h, w, guard=0):
        import torch
        self.h, self.w, self.guard = h, w, guard
        self.ws_words = (4 * (1 + (h - h % 32) * w) + 255) // 256 * 64

        def make(per_pixel, dtype, fill):
            return torch.full((h * w * per_pixel + guard,), fill, dtype=dtype, device="cuda:0")

        self.raw = {"sum": make(3, torch.float64, NAN), "stats": make(2, torch.float64, NAN), "count": make(1, torch.int32, WORD),
                    "mean": make(3, torch.float64, NAN), "rgb8": make(3, torch.uint8, BYTE), "mask": make(1, torch.uint8, BYTE)}
        self.ws = torch.full((self.ws_words + guard,), WORD, dtype=torch.int32, device="cuda:0")
        n = h * w
        self.sum, self.stats = self.raw["sum"][:n * 3].view(h, w, 3), self.raw["stats"][:n * 2].view(h, w, 2)
        self.count, self.mean = self.raw["count"][:n].view(h, w), self.raw["mean"][:n * 3].view(h, w, 3)
        self.rgb8, self.mask = self.raw["rgb8"][:n * 3].view(h, w, 3), self.raw["mask"][:n].view(h, w)

    def snapshot(self):
        """Everything as numpy: the six buffers [h][w][...] and the list as a sorted array."""
        import torch
        torch.cuda.synchronize()
        out = {k: getattr(self, k).cpu().numpy().copy() for k in self.raw}
        out["count"] = out["count"].view(np.uint32)
        ws = self.ws.cpu().numpy().view(np.uint32)
        if ws[0] == WORD and np.all(ws == WORD):                          # no call has touched the workspace yet
            out["listed"], out["list"] = None, ws[:0]
            return out
        assert ws[0] <= (self.h - self.h % 32) * self.w
        out["listed"], out["list"] = int(ws[0]), np.sort(ws[1:1 + ws[0]])
        return out


def device_tables(c, n_rows, radii):
    import torch
    table = torch.from_numpy(c.lens_sequence(0, n_rows)).to("cuda:0")
    offsets = None if radii is None else torch.from_numpy(c.light_sequence(0, n_rows, radii)).to("cuda:0")
    return table, offsets


def converge_pass(pkg, c, f, depth, aperture, focus, ns, tol, lo, hi, tables, fresh, outputs=True):
    p = pkg.backend.make_params(workloads.FOV, float(f.h), float(f.w), depth)
    table, offsets = tables
    c.accumulate_converging_device(p, f.sum, f.stats, f.count, aperture, focus, ns, table, tol, lo, hi, fresh, offsets=offsets,
                                   mean=f.mean if outputs else None, rgb8=f.rgb8 if outputs else None, mask=f.mask if outputs else None,
                                   workspace=f.ws[:f.ws_words])


def run_case(pkg, c, name, passes=None, h=32, w=32, focus=LR.FOCUS, every=True):
    """The passes of a case of converge_reference.CASES, the first fresh, until a pass lists nothing (or `passes` of them) ->
    the snapshots after each pass (after the last only where `every` is off)."""
    scene, depth, aperture, radii, ns, tol, lo, hi = CR.CASES[name]
    f, tables, out, k = Frame(pkg, h, w), device_tables(c, hi, radii), [], 0
    while passes is None or k < passes:
        converge_pass(pkg, c, f, depth, aperture, focus, ns, tol, lo, hi, tables, k == 0)
        k += 1
        snap = f.snapshot() if every or passes == k or passes is None else None
        out.append(snap)
        if passes is None and snap["listed"] == 0:
            break
        assert k <= 8 * (hi // ns + 2)                                  # (a safety stop, as converge_reference.run's)
    return out


def plain_snapshots(pkg, c, depth, aperture, focus, ns, n_passes, radii, h=32, w=32):
    """The plain run -- rm_accumulate_lens_device, with radii rm_accumulate_soft_device -- in passes of ns: count -> (sum, mean,
    bytes) after that many samples."""
    import torch
    p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)
    total = torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda:0")
    mean = torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda:0")
    rgb8 = torch.full((h, w, 3), BYTE, dtype=torch.uint8, device="cuda:0")
    out = {}
    for k in range(n_passes):
        table = c.lens_sequence(k * ns, ns)
        if radii is None:
            c.accumulate_lens_device(p, total, aperture, focus, table, k * ns, mean=mean, rgb8=rgb8)
        else:
            c.accumulate_soft_device(p, total, aperture, focus, table, c.light_sequence(k * ns, ns, radii), k * ns, mean=mean, rgb8=rgb8)
        torch.cuda.synchronize()
        out[(k + 1) * ns] = (total.cpu().numpy().copy(), mean.cpu().numpy().copy(), rgb8.cpu().numpy().copy())
    return out


# ---------------------------------------------------------------- 1. tolerance < 0 is the plain run
@pytest.mark.parametrize("name,depth", [("demo", 3), ("cornell", 3), ("synthetic256", 6)])
def test_a_negative_tolerance_is_the_plain_run_byte_for_byte(pkg, ctx, Y, name, depth):
    """A fresh pass and two continued ones of 5 samples (12 pixels a wave, four idle lanes), under a cap of 16: with stored
    lights against rm_accumulate_lens_device, with offset lights against rm_accumulate_soft_device."""
    aperture, focus = GL.LENS[name]
    GL.upload(ctx, Y.scene(name)[0])
    for radii in (None, (1.5,) * Y.n_lights(name)):
        plain = plain_snapshots(pkg, ctx, depth, aperture, focus, 5, 3, radii)
        f, tables = Frame(pkg, 32, 32), device_tables(ctx, 16, radii)
        for k in range(4):
            converge_pass(pkg, ctx, f, depth, aperture, focus, 5, -1., 16, 16, tables, k == 0)
            got = f.snapshot()
            if k == 3:                                                # 15 + 5 > 16: every pixel is capped, nothing is listed or touched
                assert got["listed"] == 0 and not got["mask"].any()
                assert all(got[key].tobytes() == before[key].tobytes() for key in ("sum", "stats", "count", "mean", "rgb8"))
                break
            n = 5 * (k + 1)
            assert got["listed"] == 1024 and np.array_equal(got["list"], np.arange(1024)) and np.all(got["mask"] == 1)
            assert np.all(got["count"] == n)
            for key, ref in zip(("sum", "mean", "rgb8"), plain[n]):
                assert not (key != "rgb8" and np.isnan(got[key]).any())
                assert got[key].tobytes() == ref.tobytes(), "%s, radii %s, %d samples: %s differs in %d pixels" % (
                    name, radii, n, key, int((got[key] != ref).any(axis=2).sum()))
            before = got
        assert plain[15][1].any()


# ---------------------------------------------------------------- 2. the left fold
@pytest.mark.parametrize("name", ["demo-8", "penumbra-8"])
def test_every_pixel_holds_the_plain_run_at_its_own_count(pkg, ctx, Y, name):
    """A converging frame run to its end, the plain run's snapshots after each pass beside it: with stored lights (demo-8) and
    with offset lights (penumbra-8)."""
    scene, depth, aperture, radii, ns, tol, lo, hi = CR.CASES[name]
    GL.upload(ctx, Y.scene(scene)[0])
    last = run_case(pkg, ctx, name, every=False)[-1]
    counts = last["count"]
    assert last["listed"] == 0 and len(np.unique(counts)) >= 3 and counts.max() + ns <= hi and counts.min() >= lo
    plain = plain_snapshots(pkg, ctx, depth, aperture, LR.FOCUS, ns, int(counts.max()) // ns, radii)
    for c in np.unique(counts):
        at = counts == c
        for key, ref in zip(("sum", "mean", "rgb8"), plain[int(c)]):
            assert last[key][at].tobytes() == ref[at].tobytes(), "%s: %s of the pixels with %d samples" % (name, key, c)
    print("%s: %d distinct counts, %d .. %d; every pixel is the plain run at its own count" % (name, len(np.unique(counts)), counts.min(), counts.max()))


# ---------------------------------------------------------------- 3. parity with the reference
def compare(name, k, got, listed, st, ymax, rows=32, w=32):
    """A pass's snapshot against the reference's record: exact masks, lists and counts, the bounds of the module docstring."""
    assert np.array_equal(got["mask"][:rows].reshape(-1).astype(bool), listed), "%s, pass %d: mask" % (name, k)
    assert np.array_equal(got["list"], np.flatnonzero(listed)), "%s, pass %d: list" % (name, k)
    assert np.array_equal(got["count"][:rows].reshape(-1), st.n), "%s, pass %d: counts" % (name, k)
    n = st.n.astype(np.float64)
    d_mean = np.abs(got["mean"][:rows].reshape(-1, 3) - st.mean).max(axis=1)
    d_sum = np.abs(got["sum"][:rows].reshape(-1, 3) - st.S).max(axis=1)
    d_y = np.abs(got["stats"][:rows].reshape(-1, 2)[:, 0] - st.Y)
    d_q = np.abs(got["stats"][:rows].reshape(-1, 2)[:, 1] - st.Q)
    assert not np.isnan(d_mean).any() and not np.isnan(d_sum).any() and not np.isnan(d_y).any() and not np.isnan(d_q).any()
    assert (d_mean < TIGHT).all() and (d_sum < n * TIGHT).all(), "%s, pass %d" % (name, k)
    assert (d_y < 3. * n * TIGHT).all() and (d_q < 6. * n * (ymax + 1.5 * TIGHT) * TIGHT).all(), "%s, pass %d" % (name, k)
    assert got["rgb8"][:rows].tobytes() == PR.to_bytes(got["mean"][:rows]).tobytes()
    return d_mean.max(), (d_sum / n).max(), (d_y / n).max(), (d_q / n).max()


@pytest.mark.parametrize("name", sorted(CR.CASES))
def test_converging_frames_match_the_reference_pass_by_pass(pkg, ctx, Y, name):
    scene, depth, aperture, radii, ns, tol, lo, hi = CR.CASES[name]
    GL.upload(ctx, Y.scene(scene)[0])
    s = CR.case_samples(Y, name)
    ymax = float(np.abs(CR.y_of(s)).max())
    recs, nearest = CR.run(s, 32, 32, ns, tol, lo, hi)
    got = run_case(pkg, ctx, name)
    assert len(got) == len(recs) == CR.FOUND[name][0]
    worst = np.zeros(4)
    for k, (g, (listed, st)) in enumerate(zip(got, recs)):
        assert g["listed"] == int(listed.sum())
        worst = np.maximum(worst, compare(name, k, g, listed, st, ymax))
    print("%s: %d passes, %d samples cast; max |delta| mean %.3e, sum / n %.3e, Y / n %.3e, Q / n %.3e (nearest decision %.3g x its margin)"
          % (name, len(got), sum(g["listed"] for g in got) * ns, worst[0], worst[1], worst[2], worst[3], nearest))
    assert sum(g["listed"] for g in got) * ns == CR.FOUND[name][1]


# ---------------------------------------------------------------- 4. unlisted pixels
def test_unlisted_pixels_keep_every_byte(pkg, ctx, Y):
    """Three passes of demo-8, then mean, bytes and mask are filled with sentinels and a fourth pass runs: it lists 273 pixels."""
    import torch
    scene, depth, aperture, radii, ns, tol, lo, hi = CR.CASES["demo-8"]
    GL.upload(ctx, Y.scene(scene)[0])
    f, tables = Frame(pkg, 32, 32), device_tables(ctx, hi, radii)
    for k in range(3):
        converge_pass(pkg, ctx, f, depth, aperture, LR.FOCUS, ns, tol, lo, hi, tables, k == 0)
    before = f.snapshot()
    f.mean.fill_(NAN), f.rgb8.fill_(BYTE), f.mask.fill_(7), f.ws.fill_(WORD)
    converge_pass(pkg, ctx, f, depth, aperture, LR.FOCUS, ns, tol, lo, hi, tables, False)
    after = f.snapshot()
    listed = after["mask"].astype(bool)
    assert set(np.unique(after["mask"])) == {0, 1} and after["listed"] == int(listed.sum()) == 273
    assert np.array_equal(after["list"], np.flatnonzero(listed.reshape(-1)))
    assert np.isnan(after["mean"][~listed]).all() and np.all(after["rgb8"][~listed] == BYTE)
    assert not np.isnan(after["mean"][listed]).any()
    for key in ("sum", "stats", "count"):
        assert after[key][~listed].tobytes() == before[key][~listed].tobytes(), key
    assert np.all(after["count"][listed] == before["count"][listed] + ns)
    ws = f.ws.cpu().numpy().view(np.uint32)
    assert np.all(ws[1 + 273:] == WORD)                                # nothing behind the list's end
    # without the optional outputs the same sum, stats and count
    g = Frame(pkg, 32, 32)
    for k in range(4):
        converge_pass(pkg, ctx, g, depth, aperture, LR.FOCUS, ns, tol, lo, hi, tables, k == 0, outputs=False)
    bare = g.snapshot()
    assert all(bare[key].tobytes() == after[key].tobytes() for key in ("sum", "stats", "count")) and np.array_equal(bare["list"], after["list"])
    assert np.isnan(bare["mean"]).all() and np.all(bare["rgb8"] == BYTE) and np.all(bare["mask"] == BYTE)


# ---------------------------------------------------------------- 5. the buffers
TALL = ("penumbra", 3, LR.APERTURE, SR.PENUMBRA_RADII, 8, 0.1, 16, 64)  # 32 x 40: rows = 32


def test_rows_below_the_last_patch_row_and_the_memory_behind_the_buffers_keep_their_bytes(pkg, ctx, Y):
    """32 x 40.  The six buffers and the workspace, their eight last rows and a guard region behind each hold NaN / BYTE / WORD
    beforehand; both tables have NaN rows behind the max_samples the call may read."""
    import torch
    scene, depth, aperture, radii, ns, tol, lo, hi = TALL
    GL.upload(ctx, Y.scene(scene)[0])
    s = Y.samples(scene, 32, 40, depth, aperture, LR.FOCUS, hi, radii)
    recs, nearest = CR.run(s, 32, 32, ns, tol, lo, hi)
    ymax = float(np.abs(CR.y_of(s)).max())
    f = Frame(pkg, 40, 32, guard=4096)
    held = {k: v.cpu().numpy().copy() for k, v in f.raw.items()}
    table, offsets = device_tables(ctx, hi, radii)
    wide_t = torch.full((hi + 64, 4), NAN, dtype=torch.float64, device="cuda:0")
    wide_o = torch.full((hi + 64, len(radii), 3), NAN, dtype=torch.float64, device="cuda:0")
    wide_t[:hi], wide_o[:hi] = table, offsets
    p = pkg.backend.make_params(workloads.FOV, 40., 32., depth)
    for k, (listed, st) in enumerate(recs):
        # (the wrapper takes the tables' rows for table_rows: hand it max_samples of them, the NaN rows lie behind)
        ctx.accumulate_converging_device(p, f.sum, f.stats, f.count, aperture, LR.FOCUS, ns, wide_t[:hi], tol, lo, hi, k == 0, offsets=wide_o[:hi],
                                         mean=f.mean, rgb8=f.rgb8, mask=f.mask, workspace=f.ws[:f.ws_words])
        got = f.snapshot()
        assert got["listed"] == int(listed.sum())
        compare("32 x 40", k, got, listed, st, ymax)
    assert got["listed"] == 0 and len(np.unique(got["count"][:32])) >= 3
    for key, per in (("sum", 3), ("stats", 2), ("count", 1), ("mean", 3), ("rgb8", 3), ("mask", 1)):
        after = f.raw[key].cpu().numpy()
        assert after[32 * 32 * per:].tobytes() == held[key][32 * 32 * per:].tobytes(), "%s: rows 32-39 or the guard" % key
    ws = f.ws.cpu().numpy().view(np.uint32)
    assert f.ws_words == ctx.converge_workspace(p) // 4 and np.all(ws[1 + 1024:] == WORD)


# ---------------------------------------------------------------- 6. the grid
def test_a_capped_grid_changes_nothing(pkg, ctx, Y, monkeypatch):
    """RM_LENS_MAX_BLOCKS = 1 and 3 (read at rm_init: contexts of their own) cap the shade kernel's grid and drive its loop over
    the groups of the list and its tail: eight passes of penumbra-8 and of demo-5, the lists as sets."""
    for name in ("penumbra-8", "demo-5"):
        scene = Y.scene(CR.CASES[name][0])[0]
        GL.upload(ctx, scene)
        free = run_case(pkg, ctx, name, passes=8, every=False)[-1]
        assert 0 < free["listed"] < 1024
        for cap in (1, 3):
            monkeypatch.setenv("RM_LENS_MAX_BLOCKS", str(cap))
            c = pkg.backend.Context(0)
            try:
                c.upload(scene.flatten())
                got = run_case(pkg, c, name, passes=8, every=False)[-1]
                for key in ("sum", "stats", "count", "mean", "rgb8", "mask", "list"):
                    assert got[key].tobytes() == free[key].tobytes(), "%s, %d workgroup(s): %s" % (name, cap, key)
            finally:
                c.close()
            monkeypatch.delenv("RM_LENS_MAX_BLOCKS")


# ---------------------------------------------------------------- 7. the oriented context
def test_oriented_context(pkg, ctx, Y):
    scene = Y.scene("demo")[0]
    GL.upload(ctx, scene)
    try:
        lo_, hi_ = GQ.bounds_of(scene.flatten().desc())
        pos, _, _ = ctx.camera()
        eye = np.array([pos.x, pos.y, pos.z]) + np.array([0.12, 0.06, 0.]) * np.linalg.norm(hi_ - lo_)
        ctx.look_at(tuple(eye), tuple((lo_ + hi_) / 2.))
        pos, basis, on = ctx.camera()
        assert on
        view = ((pos.x, pos.y, pos.z), RR.basis_tuple(basis))
        focus = float(np.linalg.norm((lo_ + hi_) / 2. - eye))
        radii, ns, tol, lo, hi = (1.5, 3.), 8, 0.1, 16, 64
        s = Y.samples("demo", 32, 32, 3, LR.APERTURE, focus, hi, radii, view)
        fixed = Y.samples("demo", 32, 32, 3, LR.APERTURE, focus, hi, radii)
        ymax = float(np.abs(CR.y_of(s)).max())
        recs, nearest = CR.run(s, 32, 32, ns, tol, lo, hi)
        f, tables = Frame(pkg, 32, 32), device_tables(ctx, hi, radii)
        worst = np.zeros(4)
        for k, (listed, st) in enumerate(recs):
            converge_pass(pkg, ctx, f, 3, LR.APERTURE, focus, ns, tol, lo, hi, tables, k == 0)
            worst = np.maximum(worst, compare("demo from the side", k, f.snapshot(), listed, st, ymax))
        print("demo from the side, %d passes: max |delta| mean %.3e (nearest decision %.3g x its margin)" % (len(recs), worst[0], nearest))
        assert f.snapshot()["listed"] == 0 and len(recs) > 3
        assert np.abs(s[:, :8].mean(axis=1) - fixed[:, :8].mean(axis=1)).max() > 0.05      # another picture than the fixed view's
    finally:
        ctx.orient(None)


# ---------------------------------------------------------------- 8. the tick
CPP_MAIN = r"""
#include <cstdio>
#include "rusty_marcher.hpp"
using namespace rusty_marcher;
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    scene::Scene sc = scene::Scene::create_default();
    framebuffer::FrameBuffer fb = framebuffer::create_frame_buffer(32, 32);
    renderer::Renderer r = renderer::create_renderer(1.5, 32., 32.);
    r.max_depth = 3;
    const rm_converge c{0.1, 16u, 256u};
    rm_converge_report rep = r.render_converging(fb, sc, c, 8u, {}, 0.4, 5., true);
    std::printf("first %u %u\n", rep.listed, rep.passes);
    while (rep.listed > 0u) rep = r.render_converging(fb, sc, c, 8u, {}, 0.4, 5.);
    std::printf("done %u %llu %u %u\n", rep.passes, (unsigned long long)rep.samples_cast, rep.max_count, r.last_samples);
    std::FILE *f = std::fopen(argv[1], "wb");
    if (!f) return 3;
    for (const auto &row : fb.buffer) std::fwrite(row.data(), sizeof(Vec3f), row.size(), f);
    std::fclose(f);
    rep = r.render_converging(fb, sc, c, 8u, {}, 0.4, 5.);
    std::printf("again %u %u\n", rep.listed, rep.passes);
    rep = r.render_converging(fb, sc, c, 8u, {1.5, 3.}, 0.4, 5.);
    std::printf("soft %u %u\n", rep.listed, rep.passes);
    return 0;
}
"""


def test_the_tick_through_c_python_and_the_cpp_mirror(pkg, entry, ctx, Y, capsys, tmp_path):
    assert workloads.FOV == 1.5 and (LR.APERTURE, LR.FOCUS) == (0.4, 5.)
    L, B = pkg.lib(), pkg._lib
    scene_name, depth, aperture, radii, ns, tol, lo, hi = CR.CASES["demo-8"]
    n_passes, cast, _ = CR.FOUND["demo-8"]
    scene = Y.scene(scene_name)[0]
    GL.upload(ctx, scene)
    device = run_case(pkg, ctx, "demo-8")
    assert len(device) == n_passes
    p = pkg.backend.make_params(workloads.FOV, 32., 32., depth)
    host, host8 = np.full((32, 32, 3), -3.5), np.full((32, 32, 3), 7, np.uint8)

    def tick(restart=False, t=tol, r=None, a=aperture, n=ns, most=hi, **kw):
        return ctx.render_converging(p, a, LR.FOCUS, n, t, lo, most, radii=r, restart=restart, **kw)

    def plain(restart=False, **kw):
        return ctx.render_progressive(p, aperture, LR.FOCUS, 8, restart, **kw)[1]

    # the frame of rm_render_progressive on the same context: begun before, continued in between and after
    plain_mean = np.full((32, 32, 3), -3.5)
    assert plain(restart=True) == 8
    before = (ctx.uploads(), ctx.launch_stats())
    # tick by tick the device call's frame, to the end
    seen = 0
    for k in range(n_passes):
        timing, rep = tick(restart=(k == 0), host_rgb=host, host_rgb8=host8)
        seen += device[k]["listed"]
        assert (rep.listed, rep.passes, rep.samples_cast) == (device[k]["listed"], k + 1, seen * ns), k
        assert rep.max_count == int(device[k]["count"].max())
        assert host.tobytes() == device[k]["mean"].tobytes() and host8.tobytes() == device[k]["rgb8"].tobytes(), k
        assert timing.kernel_ms > 0. and timing.total_ms >= timing.kernel_ms
        if k == 4:
            assert plain() == 16                                       # the other call's frame goes on, and so does this one
    assert rep.listed == 0 and rep.samples_cast == cast
    # a finished picture: nothing is launched, the report says 0, the frame stands
    for _ in range(2):
        again, again8 = np.full((32, 32, 3), NAN), np.full((32, 32, 3), BYTE, np.uint8)
        timing, rep = tick(host_rgb=again, host_rgb8=again8)
        assert timing.kernel_ms == 0. and (rep.listed, rep.passes, rep.samples_cast) == (0, n_passes, cast)
        assert again.tobytes() == host.tobytes() and again8.tobytes() == host8.tobytes()
    assert (ctx.uploads(), ctx.launch_stats()) == before              # the counters of renders and uploads were left alone
    assert plain(host_rgb=plain_mean) == 24
    assert plain_mean.tobytes() == GP.run_passes(pkg, ctx, 32, 32, depth, aperture, LR.FOCUS, ctx.lens_sequence(0, 24), (8, 8, 8))[1].tobytes()
    # a tightened tolerance continues: the reference's next pass on the finished state, not a fresh frame
    s = CR.case_samples(Y, "demo-8")
    recs, _ = CR.run(s, 32, 32, ns, tol, lo, hi)
    st = recs[-1][1].copy()
    listed, near = CR.one_pass(st, s, ns, 0.05, lo, hi, False, float(np.abs(CR.y_of(s)).max()))
    assert 0 < int(listed.sum()) < 1024
    timing, rep = tick(t=0.05, host_rgb=again)
    assert (rep.listed, rep.passes, rep.samples_cast) == (int(listed.sum()), n_passes + 1, cast + int(listed.sum()) * ns)
    assert GL.worst(again, st.mean.reshape(32, 32, 3)) < TIGHT and timing.kernel_ms > 0.
    # ... and another n_samples or cap continues too
    assert tick(t=0.05, n=4)[1].passes == n_passes + 2 and tick(t=0.05, most=512)[1].passes == n_passes + 3
    # what begins the frame again, one at a time, each followed by a tick that goes on
    for kw in (dict(restart=True), dict(r=(1.5, 3.)), dict(r=(1.5, 2.)), dict(r=(0., 0.)), dict(), dict(a=0.3)):
        first = tick(**kw)[1]
        assert (first.listed, first.passes, first.samples_cast, first.max_count) == (1024, 1, 1024 * ns, ns), kw
        kw.pop("restart", None)
        assert tick(**kw)[1].passes == 2
    # ... the camera moved, turned and turned back, as rm_render_progressive's frame
    pos, _, _ = ctx.camera()
    ctx.set_camera((pos.x + 0.25, pos.y, pos.z))
    assert tick()[1].passes == 1 and tick()[1].passes == 2
    ctx.look_at((pos.x + 0.25, pos.y, pos.z), (0., 0., -10.))
    assert ctx.camera()[2] and tick()[1].passes == 1 and tick()[1].passes == 2
    ctx.orient(None)
    assert tick()[1].passes == 1 and tick()[1].passes == 2
    ctx.set_camera((pos.x, pos.y, pos.z))
    assert tick()[1].passes == 1 and tick()[1].passes == 2
    # ... and the params: the depth cap, the view, the frame's size, the background
    def other(params):
        return ctx.render_converging(params, aperture, LR.FOCUS, ns, tol, lo, hi)[1]
    deeper = pkg.backend.make_params(workloads.FOV, 32., 32., depth + 1)
    wider = pkg.backend.make_params(workloads.FOV + 0.25, 32., 32., depth)
    taller = pkg.backend.make_params(workloads.FOV, 64., 32., depth)
    tinted = pkg.backend.make_params(workloads.FOV, 32., 32., depth)
    tinted.background.y = 0.25
    for params, pixels in ((deeper, 1024), (wider, 1024), (taller, 2048), (tinted, 1024), (p, 1024)):
        first = other(params)
        assert (first.listed, first.passes, first.max_count) == (pixels, 1, ns) and other(params).passes == 2
    # what does not: RM_FLAG_FAST_FP, tolerated, ignored and not part of the key
    fast = pkg.backend.make_params(workloads.FOV, 32., 32., depth)
    fast.flags = B.RM_FLAG_FAST_FP
    assert other(fast).passes == 3
    ctx.upload(workloads.product_scene(pkg, "cornell").flatten())     # another scene
    assert tick()[1].passes == 1
    GL.upload(ctx, scene)
    assert tick()[1].passes == 1 and tick()[1].passes == 2
    # offset lights through the tick: the device call's frame with both sequences, three ticks
    GL.upload(ctx, Y.scene("penumbra")[0])
    soft = run_case(pkg, ctx, "penumbra-8", passes=3)
    for k in range(3):
        rep = ctx.render_converging(p, 0., LR.FOCUS, 8, 0.1, 16, 256, radii=SR.PENUMBRA_RADII, restart=(k == 0), host_rgb=host)[1]
        assert rep.listed == soft[k]["listed"] and host.tobytes() == soft[k]["mean"].tobytes()
    GL.upload(ctx, scene)
    # the C entry point itself
    lens, conv, report = B.rm_lens(aperture, LR.FOCUS, ns, 0), B.rm_converge(tol, lo, hi), B.rm_converge_report()
    D = C.POINTER(C.c_double)
    for k in range(3):
        st_ = L.rm_render_converging(ctx.ptr, C.byref(p), C.byref(lens), C.byref(conv), None, 0, 1 if k == 0 else 0, again.ctypes.data_as(D), None,
                                     C.byref(report), None)
        assert st_ == 0 and (report.listed, report.passes) == (device[k]["listed"], k + 1)
    assert again.tobytes() == device[2]["mean"].tobytes()
    # a refused call in between changes nothing of the frame
    bad = B.rm_converge(float("nan"), lo, hi)
    report.passes = 77
    assert L.rm_render_converging(ctx.ptr, C.byref(p), C.byref(lens), C.byref(bad), None, 0, 0, again.ctypes.data_as(D), None, C.byref(report),
                                  None) == B.RM_ERR_INVALID_ARG and report.passes == 77
    assert again.tobytes() == device[2]["mean"].tobytes()
    assert tick(host_rgb=again)[1].passes == 4 and again.tobytes() == device[3]["mean"].tobytes()
    # Renderer.render_converging and render_converged: the prints of render(), the report returned
    r = pkg.create_renderer(workloads.FOV, 32., 32.)
    r.max_depth = depth
    fb = pkg.create_frame_buffer(32, 32)
    capsys.readouterr()
    rep = r.render_converging(fb, scene, tol, ns, lo, hi, aperture=aperture, focus=LR.FOCUS, restart=True)
    out = capsys.readouterr().out
    assert "Scene rendered in " in out and "compute units used" in out
    assert (rep.listed, rep.passes) == (1024, 1) and r.last_samples == ns and r.last_report is rep and r.last_timing.kernel_ms > 0.
    assert fb.buffer.tobytes() == device[0]["mean"].tobytes()
    rep = r.render_converged(fb, scene, tol, ns, lo, hi, aperture=aperture, focus=LR.FOCUS)
    assert (rep.listed, rep.passes, rep.samples_cast) == (0, n_passes, cast) and fb.buffer.tobytes() == device[-1]["mean"].tobytes()
    # the C++ mirror, from compiled code
    src, exe, dump = tmp_path / "tick.cpp", tmp_path / "tick", tmp_path / "tick.f64"
    src.write_text(CPP_MAIN)
    lib_dir = os.path.join(entry.PKG_DIR, "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(entry.ROOT, "include"), "-I", os.path.join(entry.PKG_DIR, "host"),
                           str(src), "-o", str(exe), "-L", lib_dir, "-lrusty_marcher_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath," + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")])
    log = subprocess.check_output([str(exe), str(dump)]).decode()
    top = int(device[-1]["count"].max())
    assert [l for l in log.splitlines() if l.split()[0] in ("first", "done", "again", "soft")] == \
        ["first 1024 1", "done %d %d %d %d" % (n_passes, cast, top, top), "again 0 %d" % n_passes, "soft 1024 1"]
    assert np.fromfile(str(dump)).tobytes() == device[-1]["mean"].tobytes()


NEAR_THE_CAP = [(8, 0.1)] * 11 + [(16, 0.05), (2, 0.05), (4, 0.05), (2, 0.05), (1, 0.05), (8, 0.05)]   # (n_samples, tolerance) a tick, cap 100


def test_the_tick_with_n_samples_and_tolerance_changing_near_the_cap(pkg, ctx, Y):
    """n_samples is not part of the frame's key, so the pass total N must stay a bound on every count whatever the slices were.
    Eleven ticks of 8 (N = 88); a tick of 16 with the tolerance halved: the pixels at 88 are capped (104 > 100) while settled
    ones with fewer samples are listed again and reach up to 96; then ticks of 2, 4, 2, 1, 8 under the cap of 100.  Every tick is
    the device call's frame byte for byte (its table has all 100 rows) and the reference's within TIGHT, lists counted exactly."""
    scene_name, depth, aperture, radii, _, _, lo, _ = CR.CASES["demo-8"]
    hi = 100
    GL.upload(ctx, Y.scene(scene_name)[0])
    s = CR.case_samples(Y, "demo-8")
    ymax = float(np.abs(CR.y_of(s)).max())
    p = pkg.backend.make_params(workloads.FOV, 32., 32., depth)
    f, tables, st = Frame(pkg, 32, 32), device_tables(ctx, hi, radii), CR.State(32, 32)
    host, cast, beyond = np.full((32, 32, 3), NAN), 0, 0
    for k, (ns, tol) in enumerate(NEAR_THE_CAP):
        before = st.n.copy()
        listed, _ = CR.one_pass(st, s, ns, tol, lo, hi, k == 0, ymax)
        converge_pass(pkg, ctx, f, depth, aperture, LR.FOCUS, ns, tol, lo, hi, tables, k == 0)
        got = f.snapshot()
        compare("near the cap", k, got, listed, st, ymax)
        timing, rep = ctx.render_converging(p, aperture, LR.FOCUS, ns, tol, lo, hi, restart=(k == 0), host_rgb=host)
        cast += int(listed.sum()) * ns
        assert (rep.listed, rep.passes, rep.samples_cast) == (int(listed.sum()), k + 1, cast), k
        assert int(st.n.max()) <= rep.max_count <= hi, k                # N is a bound on every count
        assert host.tobytes() == got["mean"].tobytes(), "tick %d (n_samples %d)" % (k, ns)
        if k >= 12:                                                     # listed pixels whose slice ends behind min(88 + ns, cap) rows
            beyond += int((listed & (before.astype(np.int64) + ns > min(88 + ns, hi))).sum())
    assert beyond > 0 and int(st.n.max()) == hi and len(np.unique(st.n)) > 12


def test_converging_calls_leave_the_render_state_alone(pkg):
    import torch
    demo = workloads.product_scene(pkg, "demo")
    p = pkg.backend.make_params(workloads.FOV, 480., 640., 5)
    small = pkg.backend.make_params(workloads.FOV, 64., 64., 5)

    def frames(with_calls):
        c = pkg.backend.Context(0)
        try:
            c.upload(demo.flatten())
            out = []
            if with_calls:
                bufs = dict(sum=torch.zeros((480, 640, 3), dtype=torch.float64, device="cuda:0"),
                            stats=torch.zeros((480, 640, 2), dtype=torch.float64, device="cuda:0"),
                            count=torch.zeros((480, 640), dtype=torch.int32, device="cuda:0"))
                table = torch.from_numpy(c.lens_sequence(0, 16)).to("cuda:0")
            for k in range(3):
                f = np.zeros((480, 640, 3))
                c.render(p, f)
                out.append(f)
                if with_calls and k < 2:                              # before, between and after: converging calls behind frames 1 and 2
                    before = (c.uploads(), c.launch_stats())
                    ws = c.accumulate_converging_device(p, bufs["sum"], bufs["stats"], bufs["count"], LR.APERTURE, LR.FOCUS, 2, table, 0.05, 2, 16, k == 0)
                    torch.cuda.synchronize()
                    host = np.zeros((64, 64, 3))
                    assert c.render_converging(small, LR.APERTURE, LR.FOCUS, 4, 0.05, 4, 64, host_rgb=host)[1].passes == k + 1
                    assert int(ws[0]) > 0 and bool((bufs["count"] == 2 * (k + 1)).any()) and host.any()
                    assert (c.uploads(), c.launch_stats()) == before
            return out
        finally:
            c.close()

    bare, ticked = frames(False), frames(True)
    for k, (a, b) in enumerate(zip(bare, ticked)):
        assert a.tobytes() == b.tobytes(), "frame %d differs once converging calls ran" % (k + 1)


# ---------------------------------------------------------------- 9. errors
def test_refusals_leave_the_buffers_and_the_frame_alone(pkg, ctx, Y):
    import torch
    L, B = pkg.lib(), pkg._lib
    depth, radii = 3, (1.5, 3.)
    GL.upload(ctx, Y.scene("demo")[0])
    p = pkg.backend.make_params(workloads.FOV, 64., 64., depth)
    f = Frame(pkg, 64, 64)
    held = f.snapshot()
    table, offsets = device_tables(ctx, 64, radii)
    host, host8 = np.full((64, 64, 3), 7.25), np.full((64, 64, 3), 7, np.uint8)
    D, U8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    good, conv = B.rm_lens(LR.APERTURE, LR.FOCUS, 4, 0), B.rm_converge(0.05, 16, 64)
    r64 = np.ascontiguousarray(radii, dtype=np.float64)
    # a standing frame of one pass: a refused call leaves it alone too
    assert ctx.render_converging(p, LR.APERTURE, LR.FOCUS, 4, 0.05, 16, 64, radii=radii, restart=True)[1].passes == 1

    def untouched():
        now = f.snapshot()
        ws = f.ws.cpu().numpy().view(np.uint32)
        return all(now[k].tobytes() == held[k].tobytes() for k in f.raw) and np.all(ws == WORD) and np.all(host == 7.25) and np.all(host8 == 7)

    vp = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None

    def device_call(lens=good, c=conv, t=table, rows=64, o=offsets, n_lights=2, params=p, buffers=True, **swap):
        b = dict(sum=f.sum, stats=f.stats, count=f.count, workspace=f.ws, mean=f.mean, rgb8=f.rgb8, mask=f.mask)
        b.update(swap)
        frame = B.rm_converge_frame(*(vp(b[k]) for k in ("sum", "stats", "count", "workspace", "mean", "rgb8", "mask")))
        st = L.rm_accumulate_converging_device(ctx.ptr, C.byref(params), C.byref(lens) if lens is not None else None,
                                               C.byref(c) if c is not None else None, vp(t), rows, vp(o), n_lights, 1,
                                               C.byref(frame) if buffers else None, None)
        msg = L.rm_last_error(ctx.ptr).decode()
        assert st != 0 and untouched(), msg
        return st, msg

    def host_call(r=r64, n_lights=2, lens=good, c=conv, params=p):
        report = B.rm_converge_report(77, 77, 77, 77, 0)
        st = L.rm_render_converging(ctx.ptr, C.byref(params), C.byref(lens), C.byref(c) if c is not None else None,
                                    r.ctypes.data_as(D) if r is not None else None, n_lights, 0, host.ctypes.data_as(D), host8.ctypes.data_as(U8),
                                    C.byref(report), None)
        msg = L.rm_last_error(ctx.ptr).decode()
        assert st != 0 and (report.samples_cast, report.listed, report.passes, report.max_count) == (77, 77, 77, 77) and untouched(), msg
        return st, msg

    E = B.RM_ERR_INVALID_ARG
    # rm_converge
    for st, msg in (device_call(c=B.rm_converge(NAN, 16, 64)), host_call(c=B.rm_converge(NAN, 16, 64))):
        assert st == E and "tolerance" in msg
    for most in (3, 0, 65, 65537, 2 ** 32 - 1):                        # below n_samples; beyond the table's rows; beyond the library's cap
        st, msg = device_call(c=B.rm_converge(0.05, 16, most))
        assert st == E and "max_samples" in msg, most
    for most in (3, 0, 65537, 2 ** 32 - 1):
        st, msg = host_call(c=B.rm_converge(0.05, 16, most))
        assert st == E and "max_samples" in msg, most
    st, msg = device_call(rows=63)                                     # a table shorter than max_samples
    assert st == E and "max_samples" in msg
    assert device_call(c=None)[1].endswith("NULL converge") and host_call(c=None)[1].endswith("NULL converge")
    # the buffers
    assert "NULL buffers" in device_call(buffers=False)[1]
    for key in ("sum", "stats", "count", "workspace"):
        st, msg = device_call(**{key: None})
        assert st == E and "NULL " + key in msg
    st, msg = device_call(mean=f.sum)
    assert st == E and "device_mean == device_sum" in msg
    st, msg = device_call(t=None)
    assert st == E and "table" in msg
    # the lights: n_lights counts where offsets are given, the radii where they are
    for n_lights in (0, 1, 3, 2 ** 32 - 1):
        st, msg = device_call(n_lights=n_lights)
        assert st == E and "n_lights" in msg and "the resident scene has 2" in msg
        st, msg = host_call(n_lights=n_lights, r=np.full(4, 1.5))
        assert st == E and "n_lights" in msg
    for bad in (-1e-9, NAN, float("inf")):
        st, msg = host_call(r=np.array([1.5, bad]))
        assert st == E and "radii[1]" in msg
    # the lens and the params, through the new entry points
    for lens, word in ((B.rm_lens(-1., LR.FOCUS, 4, 0), "aperture"), (B.rm_lens(LR.APERTURE, 0., 4, 0), "focus"), (B.rm_lens(LR.APERTURE, LR.FOCUS, 65, 0), "n_samples")):
        for st, msg in (device_call(lens=lens), host_call(lens=lens)):
            assert st == E and word in msg
    assert "NULL lens" in device_call(lens=None)[1]
    odd = pkg.backend.make_params(workloads.FOV, 64., 100., depth)
    assert device_call(params=odd)[0] == B.RM_ERR_DIMENSIONS and host_call(params=odd)[0] == B.RM_ERR_DIMENSIONS
    huge = pkg.backend.make_params(workloads.FOV, 65536., 32768., depth)   # rows * frame_width = 2^31: checked before any pointer is touched
    for st, msg in (device_call(params=huge), host_call(params=huge)):
        assert st == B.RM_ERR_DIMENSIONS and "2^31" in msg
    deep = pkg.backend.make_params(workloads.FOV, 64., 64., 1000)
    assert device_call(params=deep)[0] == B.RM_ERR_DEPTH and host_call(params=deep)[0] == B.RM_ERR_DEPTH
    fresh = pkg.backend.Context(0)
    try:
        report = B.rm_converge_report(77, 77, 77, 77, 0)
        assert L.rm_render_converging(fresh.ptr, C.byref(p), C.byref(good), C.byref(conv), None, 0, 0, None, None, C.byref(report),
                                      None) == B.RM_ERR_NO_SCENE and report.passes == 77
    finally:
        fresh.close()
    # the Python wrapper hands the library's refusal on
    with pytest.raises(B.BackendError, match="n_lights"):
        ctx.render_converging(p, LR.APERTURE, LR.FOCUS, 4, 0.05, 16, 64, radii=(1.5, 1.5, 1.5))
    # the standing frame went through all that untouched: the next tick is its second pass
    assert ctx.render_converging(p, LR.APERTURE, LR.FOCUS, 4, 0.05, 16, 64, radii=radii)[1].passes == 2
    # what is tolerated: a frame without a whole patch row; NULL offsets with any n_lights; a scene without lights
    short = Frame(pkg, 31, 64)
    converge_pass(pkg, ctx, short, depth, LR.APERTURE, LR.FOCUS, 4, 0.05, 16, 64, (table, offsets), True)
    got = short.snapshot()                                              # rows == 0: RM_OK, nothing done (the list's length is not cleared either)
    assert np.isnan(got["sum"]).all() and np.all(got["count"] == WORD) and np.all(short.ws.cpu().numpy().view(np.uint32) == WORD)
    tiny = pkg.backend.make_params(workloads.FOV, 31., 64., depth)
    rep = ctx.render_converging(tiny, LR.APERTURE, LR.FOCUS, 4, 0.05, 16, 64)[1]
    assert (rep.listed, rep.passes, rep.samples_cast, rep.max_count) == (0, 0, 0, 0)
    g = Frame(pkg, 64, 64)
    frame = B.rm_converge_frame(vp(g.sum), vp(g.stats), vp(g.count), vp(g.ws), None, None, None)
    assert L.rm_accumulate_converging_device(ctx.ptr, C.byref(p), C.byref(good), C.byref(conv), vp(table), 64, None, 7, 1, C.byref(frame), None) == 0
    assert g.snapshot()["listed"] == 64 * 64
    dark = pkg.Scene.new()
    dark.shapes.append(pkg.sphere.create(pkg.Vec3f(0., 0., -6.), 2., pkg.Reflectance(**RR.GLASS)))
    c = pkg.backend.Context(0)
    try:
        c.upload(dark.flatten())
        small = pkg.backend.make_params(workloads.FOV, 32., 32., depth)
        a, b = Frame(pkg, 32, 32), Frame(pkg, 32, 32)
        tables = device_tables(c, 16, ())
        assert tables[1].shape == (16, 0, 3)
        converge_pass(pkg, c, a, depth, 0., LR.FOCUS, 4, -1., 0, 16, tables, True)
        converge_pass(pkg, c, b, depth, 0., LR.FOCUS, 4, -1., 0, 16, (tables[0], None), True)
        lens_only = GP.run_passes(pkg, c, 32, 32, depth, 0., LR.FOCUS, PR.lens_sequence(0, 4), (4,))
        assert a.snapshot()["mean"].tobytes() == b.snapshot()["mean"].tobytes() == lens_only[1].tobytes()
        assert c.render_converging(small, 0., LR.FOCUS, 4, 0.05, 16, 64, radii=())[1].listed == 1024
    finally:
        c.close()
    assert untouched()
