"""Converging frames over a swept hierarchy on the GPU (-m gpu): rm_accumulate_converging_swept_device through the C ABI and
the Python bindings, against rm_accumulate_converging_moving_device pass for pass -- sums, stats, counts, means, bytes, masks,
lists and their lengths, byte for byte -- and against the plain swept run of rm_accumulate_swept_device at every pixel's own
count.  Frames are 32 x 32, passes of 4 or 5 samples, depth 3 to 6."""
import numpy as np
import pytest

import lens_reference as LR
import moving_reference as MV
import progressive_reference as PR
import radiance_reference as RR
import swept_reference as SW
import test_gpu_converge as GC
import test_gpu_converge_moving as GCM
import test_gpu_lens as GL
import test_gpu_progressive as GP
import test_gpu_swept as GS
import variant_matrix as VM
import workloads

pytestmark = pytest.mark.gpu

NAN, BYTE = GP.NAN, GP.BYTE
Frame = GC.Frame
MOVING, SWEPT = GCM.MOVING, "accumulate_converging_swept_device"
KEYS = ("sum", "stats", "count", "mean", "rgb8", "mask", "list")
NS, TOL, LO, HI = 4, 0.02, 8, 24                                       # samples a pass, tolerance, min_samples, max_samples


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_converge_swept"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return MV.Yardstick(pkg, O, orc)


def device_tables(ctx, Y, key, name, rows):
    table, lights, shapes, _ = GS.tables(ctx, Y, key, name, rows)
    return GCM.on_device(table, lights, shapes)


def passes_of(pkg, c, depth, tables, call, ns=NS, tol=TOL, lo=LO, hi=HI, most=8):
    """Passes of a frame, the first fresh, until one lists nothing -> the snapshots after each."""
    f, out = Frame(pkg, 32, 32), []
    for k in range(most):
        GCM.moving_pass(pkg, c, f, depth, VM.APERTURE, VM.FOCUS, ns, tol, lo, hi, tables, k == 0, call=call)
        out.append(f.snapshot())
        if out[-1]["listed"] == 0:
            break
    return out


# ---------------------------------------------------------------- 1. the flat pass's bytes, pass for pass
@pytest.mark.parametrize("name,depth", [("matrix-spheres", 5), ("matrix-spheres", 6), ("matrix-mesh", 5), ("cornell", 3), ("seventeen", 4),
                                        ("thirteen", 6), ("demo", 3)])
def test_swept_passes_are_the_flat_passes_byte_for_byte(pkg, ctx, Y, name, depth):
    key, scene = GS.scene_of(Y, name)
    GL.upload(ctx, scene)
    tables = device_tables(ctx, Y, key, name, HI)
    flat = passes_of(pkg, ctx, depth, tables, MOVING)
    swept = passes_of(pkg, ctx, depth, tables, SWEPT)
    assert len(flat) == len(swept) >= 3                                 # (two passes to min_samples, then the rule decides)
    for k, (a, b) in enumerate(zip(swept, flat)):
        assert a["listed"] == b["listed"], "%s pass %d: %d listed, the flat pass lists %d" % (name, k, a["listed"], b["listed"])
        for part in KEYS:
            assert a[part].tobytes() == b[part].tobytes(), "%s pass %d: %s differs" % (name, k, part)
    last = flat[-1]
    print("%s depth %d: %d passes, counts %d .. %d" % (name, depth, len(flat), last["count"].min(), last["count"].max()))
    assert not np.isnan(last["mean"]).any()
    if name.startswith("matrix-"):
        assert 0 < flat[2]["listed"] < 1024                             # some pixels settle at min_samples, some do not


# ---------------------------------------------------------------- 2. a pixel with count c holds the plain swept run after c rows
def plain_swept(pkg, c, depth, tables, ns, n_passes, handle):
    import torch
    p = pkg.backend.make_params(workloads.FOV, 32., 32., depth)
    total = torch.full((32, 32, 3), NAN, dtype=torch.float64, device="cuda:0")
    mean = torch.full((32, 32, 3), NAN, dtype=torch.float64, device="cuda:0")
    rgb8 = torch.full((32, 32, 3), BYTE, dtype=torch.uint8, device="cuda:0")
    table, lights, shapes = tables
    out = {}
    for k in range(n_passes):
        rows = slice(k * ns, (k + 1) * ns)
        c.accumulate_swept_device(p, total, VM.APERTURE, VM.FOCUS, table[rows].contiguous(), lights[rows].contiguous(), shapes[rows].contiguous(),
                                  k * ns, mean=mean, rgb8=rgb8, swept=handle)
        torch.cuda.synchronize()
        out[(k + 1) * ns] = (total.cpu().numpy().copy(), mean.cpu().numpy().copy(), rgb8.cpu().numpy().copy())
    return out


@pytest.mark.parametrize("name", ["matrix-spheres", "matrix-mesh"])
def test_every_pixel_holds_the_plain_swept_run_at_its_own_count(pkg, ctx, Y, name):
    key, scene = GS.scene_of(Y, name)
    GL.upload(ctx, scene)
    tables = device_tables(ctx, Y, key, name, HI)
    last = passes_of(pkg, ctx, 5, tables, SWEPT)[-1]
    counts = last["count"]
    assert len(np.unique(counts)) >= 3 and counts.min() >= LO and counts.max() <= HI
    lo, hi = pkg.backend.swept_extents(tables[2].cpu().numpy())
    handle = ctx.swept(lo, hi)
    try:
        plain = plain_swept(pkg, ctx, 5, tables, NS, int(counts.max()) // NS, handle)
    finally:
        handle.close()
    for c in np.unique(counts):
        at = counts == c
        for part, ref in zip(("sum", "mean", "rgb8"), plain[int(c)]):
            assert last[part][at].tobytes() == ref[at].tobytes(), "%s: %s of the pixels with %d samples" % (name, part, c)


# ---------------------------------------------------------------- 3. tolerance < 0 is the plain swept frame
def test_a_negative_tolerance_is_the_plain_swept_frame(pkg, ctx, Y):
    key, scene = GS.scene_of(Y, "matrix-mesh")
    GL.upload(ctx, scene)
    tables = device_tables(ctx, Y, key, "matrix-mesh", 15)
    handle = ctx.swept(*pkg.backend.swept_extents(tables[2].cpu().numpy()))
    try:
        plain = plain_swept(pkg, ctx, 5, tables, 5, 3, handle)
        f = Frame(pkg, 32, 32)
        for k in range(3):
            p = pkg.backend.make_params(workloads.FOV, 32., 32., 5)
            ctx.accumulate_converging_swept_device(p, f.sum, f.stats, f.count, VM.APERTURE, VM.FOCUS, 5, *tables, -1., 15, 15, k == 0, mean=f.mean,
                                                   rgb8=f.rgb8, mask=f.mask, workspace=f.ws[:f.ws_words], swept=handle)
            got = f.snapshot()
            n = 5 * (k + 1)
            assert got["listed"] == 1024 and np.all(got["count"] == n) and np.all(got["mask"] == 1)
            for part, ref in zip(("sum", "mean", "rgb8"), plain[n]):
                assert got[part].tobytes() == ref.tobytes(), "%d samples: %s differs" % (n, part)
    finally:
        handle.close()


# ---------------------------------------------------------------- 4. unlisted pixels keep every byte
def test_unlisted_pixels_keep_their_bytes(pkg, ctx, Y):
    key, scene = GS.scene_of(Y, "matrix-spheres")
    GL.upload(ctx, scene)
    tables = device_tables(ctx, Y, key, "matrix-spheres", HI)
    snaps = passes_of(pkg, ctx, 5, tables, SWEPT)
    seen = 0
    for before, after in zip(snaps[1:], snaps[2:]):                     # from the third pass on some pixels are settled
        listed = np.zeros(1024, bool)
        listed[after["list"]] = True
        kept = ~listed.reshape(32, 32)
        assert np.array_equal(after["mask"].astype(bool), ~kept)
        for part in ("sum", "stats", "count", "mean", "rgb8"):
            assert after[part][kept].tobytes() == before[part][kept].tobytes(), part
        assert (after["count"][~kept] == before["count"][~kept] + NS).all()
        seen += int(kept.sum())
    assert seen > 0
