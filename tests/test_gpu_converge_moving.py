"""Converging frames with moving shapes on the GPU (-m gpu): rm_accumulate_converging_moving_device and
rm_render_converging_moving through the C ABI, the Python bindings and the C++ mirror, against the frames of
rm_accumulate_converging_motion_device and rm_accumulate_moving_device and against tests/converge_moving_reference.py -- the
select rule and the fold in numpy over every row of the three sequences for every pixel of a scene whose every shape is moved,
cast by the CPU oracle (pinned on the CPU by tests/test_converge_moving_abi.py, which also shows that no decision of these cases
is close).

What the header calls byte for byte is demanded byte for byte.  Against the yardstick the bounds are tests/test_gpu_converge.py's:
masks, lists (as sets) and counts exactly, every channel of the mean within TIGHT = 1e-9, of the sum within n TIGHT, Y within
3 n TIGHT and Q within 6 n (ymax + 1.5 TIGHT) TIGHT, no pixel left out.  Every table entry is finite."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import converge_moving_reference as CMV
import converge_reference as CR
import lens_reference as LR
import motion_reference as MR
import moving_reference as MV
import progressive_reference as PR
import radiance_reference as RR
import soft_reference as SR
import test_gpu_converge as GC
import test_gpu_lens as GL
import test_gpu_progressive as GP
import test_gpu_query as GQ
import variant_matrix as VM
import workloads

pytestmark = pytest.mark.gpu

TIGHT = CR.TIGHT
NAN, BYTE, WORD = GP.NAN, GP.BYTE, GC.WORD
Frame, compare = GC.Frame, GC.compare
cells = pytest.mark.parametrize("cell", VM.CELLS, ids=VM.cell_id)
MOVING, MOTION = "accumulate_converging_moving_device", "accumulate_converging_motion_device"


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_converge_moving"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return CMV.Yardstick(pkg, O, orc)


@pytest.fixture(scope="module")
def matrix(pkg, O, orc):
    return VM.Matrix(pkg, O, orc)


def on_device(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0") for a in arrays)


def velocities_of(Y, scene, speed=None):
    return MV.velocities(Y.kinds(scene), MV.SPEED.get(scene, MV.CELL_SPEED) if speed is None else speed)


def library_tables(c, Y, scene, n_rows, radii, speed=None):
    """Rows [0, n_rows) of the library's three sequences for the scene and the test velocities, on the device; they are the
    yardstick's byte for byte."""
    speed = MV.SPEED.get(scene, MV.CELL_SPEED) if speed is None else speed
    table, lights, shapes = Y.tables(scene, n_rows, radii, speed)
    assert c.lens_sequence(0, n_rows).tobytes() == table.tobytes()
    assert c.motion_sequence(0, n_rows, velocities_of(Y, scene, speed), MV.SHUTTER).tobytes() == shapes.tobytes()
    if radii is not None:
        assert c.light_sequence(0, n_rows, radii).tobytes() == lights.tobytes()
    assert np.isfinite(shapes).all() and np.isfinite(lights).all()
    return on_device(table, lights, shapes)


def moving_pass(pkg, c, f, depth, aperture, focus, ns, tol, lo, hi, tables, fresh, outputs=True, call=MOVING):
    p = pkg.backend.make_params(workloads.FOV, float(f.h), float(f.w), depth)
    table, lights, shapes = tables
    getattr(c, call)(p, f.sum, f.stats, f.count, aperture, focus, ns, table, lights, shapes, tol, lo, hi, fresh,
                     mean=f.mean if outputs else None, rgb8=f.rgb8 if outputs else None, mask=f.mask if outputs else None,
                     workspace=f.ws[:f.ws_words])


def run_passes(pkg, c, depth, aperture, focus, ns, tol, lo, hi, tables, passes=None, h=32, w=32, every=True):
    """Passes of a frame, the first fresh, until a pass lists nothing (or `passes` of them) -> the snapshots after each pass
    (after the last only where `every` is off)."""
    f, out, k = Frame(pkg, h, w), [], 0
    while passes is None or k < passes:
        moving_pass(pkg, c, f, depth, aperture, focus, ns, tol, lo, hi, tables, k == 0)
        k += 1
        snap = f.snapshot() if every or passes == k or passes is None else None
        out.append(snap)
        if passes is None and snap["listed"] == 0:
            break
        assert k <= 8 * (hi // ns + 2)                                  # (a safety stop, as converge_reference.run's)
    return out


def run_case(pkg, c, Y, name, passes=None, h=32, w=32, every=True):
    scene, depth, aperture, radii, ns, tol, lo, hi = CMV.CASES[name]
    return run_passes(pkg, c, depth, aperture, LR.FOCUS, ns, tol, lo, hi, library_tables(c, Y, scene, hi, radii, CMV.SPEED[name]), passes, h, w, every)


def plain_moving_snapshots(pkg, c, depth, aperture, focus, ns, n_passes, tables, h=32, w=32):
    """The plain moving-shapes run -- rm_accumulate_moving_device over consecutive slices of the three tables -- in passes of ns:
    count -> (sum, mean, bytes) after that many rows."""
    import torch
    p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)
    total = torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda:0")
    mean = torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda:0")
    rgb8 = torch.full((h, w, 3), BYTE, dtype=torch.uint8, device="cuda:0")
    table, lights, shapes = tables
    out = {}
    for k in range(n_passes):
        rows = slice(k * ns, (k + 1) * ns)
        c.accumulate_moving_device(p, total, aperture, focus, table[rows].contiguous(), lights[rows].contiguous(), shapes[rows].contiguous(),
                                   k * ns, mean=mean, rgb8=rgb8)
        torch.cuda.synchronize()
        out[(k + 1) * ns] = (total.cpu().numpy().copy(), mean.cpu().numpy().copy(), rgb8.cpu().numpy().copy())
    return out


# ---------------------------------------------------------------- 1. parity with the yardstick, pass by pass
@pytest.mark.parametrize("name", sorted(CMV.CASES))
def test_converging_moving_frames_match_the_yardstick_pass_by_pass(pkg, ctx, Y, name):
    scene, depth, aperture, radii, ns, tol, lo, hi = CMV.CASES[name]
    GL.upload(ctx, Y.scene(scene)[0])
    s = CMV.case_samples(Y, name)
    ymax = float(np.abs(CR.y_of(s)).max())
    recs, nearest = CR.run(s, 32, 32, ns, tol, lo, hi)
    got = run_case(pkg, ctx, Y, name)
    assert len(got) == len(recs) == CMV.FOUND[name][0]
    worst = np.zeros(4)
    for k, (g, (listed, st)) in enumerate(zip(got, recs)):
        assert g["listed"] == int(listed.sum())
        worst = np.maximum(worst, compare(name, k, g, listed, st, ymax))
    print("%s: %d passes, %d samples cast; max |delta| mean %.3e, sum / n %.3e, Y / n %.3e, Q / n %.3e (nearest decision %.3g x its margin)"
          % (name, len(got), sum(g["listed"] for g in got) * ns, worst[0], worst[1], worst[2], worst[3], nearest))
    assert sum(g["listed"] for g in got) * ns == CMV.FOUND[name][1]
    assert len(np.unique(got[-1]["count"])) == CMV.FOUND[name][2]


# ---------------------------------------------------------------- 2. zero offsets and zero rows but the spheres'
@pytest.mark.parametrize("name,depth", [("demo", 3), ("cornell", 3), ("matrix-mesh", 5), ("matrix-spheres", 6)])
def test_zero_offsets_and_zero_rows_are_the_moving_spheres_pass_byte_for_byte(pkg, ctx, matrix, Y, name, depth):
    """Seven passes of 5 samples (12 pixels a wave, four idle lanes) under a cap of 40, area lights, both calls over the same
    three tables.  (a) every shape offset zero, +0. in the first half of the table and -0. in the second; (b) the test
    velocities' rows for the spheres and zero rows for every other shape.  The Cornell box holds no sphere: the moving spheres'
    call never reads its table, this one reads every row.  Both matrix scenes carry a hierarchy; both calls walk flat."""
    if name.startswith("matrix-"):
        bvh = name.split("-")[1]
        pair = matrix.pair(bvh, False)
        name = VM.register(Y, matrix.name(bvh, False), pair)
        scene, aperture, focus = pair[0], VM.APERTURE, VM.FOCUS
    else:
        scene, (aperture, focus) = Y.scene(name)[0], GL.LENS[name]
    GL.upload(ctx, scene)
    kinds = Y.kinds(name)
    ns, tol, lo, hi = 5, 0.1, 10, 40
    radii = (1.5,) * Y.n_lights(name)
    zeros = np.zeros((hi, len(kinds), 3))
    zeros[hi // 2:] = -0.
    only = MV.spheres_only(MR.motion_sequence(0, hi, velocities_of(Y, name), MV.SHUTTER), kinds)
    assert (only != 0.).any() == (MV.ORC_SPHERE in kinds)
    for offsets, what in ((zeros, "zero offsets"), (only, "zero rows but the spheres'")):
        tables = on_device(PR.lens_sequence(0, hi), SR.light_sequence(0, hi, radii), offsets)
        a, b = Frame(pkg, 32, 32), Frame(pkg, 32, 32)
        partial = 0
        for k in range(7):
            moving_pass(pkg, ctx, a, depth, aperture, focus, ns, tol, lo, hi, tables, k == 0, call=MOTION)
            moving_pass(pkg, ctx, b, depth, aperture, focus, ns, tol, lo, hi, tables, k == 0)
            spheres, shapes = a.snapshot(), b.snapshot()
            assert spheres["listed"] == shapes["listed"]
            partial += 0 < spheres["listed"] < 1024
            for key in ("sum", "stats", "count", "mean", "rgb8", "mask", "list"):
                assert not (key in ("sum", "stats", "mean") and np.isnan(shapes[key]).any())
                assert shapes[key].tobytes() == spheres[key].tobytes(), "%s, %s, pass %d: %s" % (name, what, k, key)
        print("%s, %s: %d of 7 passes list some of the pixels, %d distinct counts" % (name, what, partial, len(np.unique(spheres["count"]))))
        assert partial >= 1 and len(np.unique(spheres["count"])) >= 2  # lists of some pixels, pixels at rows of their own


# ---------------------------------------------------------------- 3. the left fold: own count
@pytest.mark.parametrize("name", ["demo-moving-8", "spheres-moving-8"])
def test_every_pixel_holds_the_plain_moving_run_at_its_own_count(pkg, ctx, Y, name):
    scene, depth, aperture, radii, ns, tol, lo, hi = CMV.CASES[name]
    GL.upload(ctx, Y.scene(scene)[0])
    tables = library_tables(ctx, Y, scene, hi, radii, CMV.SPEED[name])
    last = run_case(pkg, ctx, Y, name, every=False)[-1]
    counts = last["count"]
    assert last["listed"] == 0 and len(np.unique(counts)) >= 3 and counts.max() + ns <= hi and counts.min() >= lo
    plain = plain_moving_snapshots(pkg, ctx, depth, aperture, LR.FOCUS, ns, int(counts.max()) // ns, tables)
    for c in np.unique(counts):
        at = counts == c
        for key, ref in zip(("sum", "mean", "rgb8"), plain[int(c)]):
            assert last[key][at].tobytes() == ref[at].tobytes(), "%s: %s of the pixels with %d samples" % (name, key, c)
    print("%s: %d distinct counts, %d .. %d; every pixel is the plain moving-shapes run at its own count" % (
        name, len(np.unique(counts)), counts.min(), counts.max()))


# ---------------------------------------------------------------- 4. tolerance < 0 is the plain moving-shapes run; a random table
@pytest.mark.parametrize("aperture", [0., LR.APERTURE])
def test_a_negative_tolerance_is_the_plain_moving_run_byte_for_byte(pkg, ctx, Y, aperture):
    """A fresh pass and two continued ones of 5 samples under a cap of 16 on the pool scene, tables that are not the library's:
    another offset for every row, shape and light, none of them zero, so a lane that reads another row's offsets, a polygon
    moved by another shape's row or a pool vertex left where it was is another picture."""
    depth = 3
    GL.upload(ctx, Y.scene("pool")[0])
    kinds = Y.kinds("pool")
    rng = np.random.default_rng(20261020)
    tables = on_device(PR.lens_sequence(0, 16), SR.random_offsets(rng, 16, Y.n_lights("pool")), MV.random_offsets(rng, 16, kinds, MV.SPEED["pool"] / 3.))
    assert all(bool(np.isfinite(t.cpu().numpy()).all()) for t in tables)
    plain = plain_moving_snapshots(pkg, ctx, depth, aperture, LR.FOCUS, 5, 3, tables)
    f = Frame(pkg, 32, 32)
    for k in range(4):
        moving_pass(pkg, ctx, f, depth, aperture, LR.FOCUS, 5, -1., 16, 16, tables, k == 0)
        got = f.snapshot()
        if k == 3:                                                    # 15 + 5 > 16: every pixel is capped, nothing is listed or touched
            assert got["listed"] == 0 and not got["mask"].any()
            assert all(got[key].tobytes() == before[key].tobytes() for key in ("sum", "stats", "count", "mean", "rgb8"))
            break
        n = 5 * (k + 1)
        assert got["listed"] == 1024 and np.array_equal(got["list"], np.arange(1024)) and np.all(got["mask"] == 1)
        assert np.all(got["count"] == n)
        for key, ref in zip(("sum", "mean", "rgb8"), plain[n]):
            assert not (key != "rgb8" and np.isnan(got[key]).any())
            assert got[key].tobytes() == ref.tobytes(), "aperture %g, %d samples: %s differs in %d pixels" % (
                aperture, n, key, int((got[key] != ref).any(axis=2).sum()))
        before = got
    # ... and the yardstick's within the bounds: the plain moving-shapes run is not a picture of its own making
    table, lights, shapes = (t.cpu().numpy() for t in tables)
    s = Y.moving_samples("pool", 32, 32, depth, aperture, LR.FOCUS, table[:15], lights[:15], shapes[:15])
    recs, _ = CR.run(s, 32, 32, 5, -1., 16, 15, passes=3)
    worst = compare("random tables, aperture %g" % aperture, 2, before, recs[-1][0], recs[-1][1], float(np.abs(CR.y_of(s)).max()))
    print("pool, random tables, aperture %g: max |delta| mean %.3e" % (aperture, worst[0]))
    # the polygons' random offsets are seen: not the picture with only the sphere moved
    only = Y.moving_samples("pool", 32, 32, depth, aperture, LR.FOCUS, table[:15], lights[:15], MV.spheres_only(shapes[:15], kinds))
    assert int((np.abs(s.mean(axis=1) - only.mean(axis=1)) > 0.05).any(axis=1).sum()) > VM.SHARE * 1024


# ---------------------------------------------------------------- 5. the variant matrix
@cells
def test_every_cell_of_the_variant_matrix(pkg, ctx, matrix, Y, cell):
    """Both powers, both stacks, a sphere hierarchy and a triangle hierarchy in the image, all walked flat: the nine cells take
    all four instantiations (POW by the cell's materials, STACK 4 at depth 5 and 32 at depth 6: variant_matrix.claims).  The
    converging cells' parameters, every shape moving at CELL_SPEED -- the glass panes among them, so children go through moved
    quads --, point lights (zero offsets) and area lights, pass by pass until nothing is listed."""
    bvh, generic, depth = cell
    ns, tol, lo, hi = VM.CONVERGE
    pair = matrix.pair(bvh, generic)
    GL.upload(ctx, pair[0])
    name = VM.register(Y, matrix.name(bvh, generic), pair)
    for radii in (None, VM.RADII):
        table, lights, shapes = Y.tables(name, hi, radii, MV.CELL_SPEED)
        s = Y.moving_samples(name, VM.W, VM.H, depth, VM.APERTURE, VM.FOCUS, table, lights, shapes)
        ymax = float(np.abs(CR.y_of(s)).max())
        recs, nearest = CR.run(s, VM.W, VM.H, ns, tol, lo, hi)        # (asserts every free decision's margin)
        got = run_passes(pkg, ctx, depth, VM.APERTURE, VM.FOCUS, ns, tol, lo, hi, library_tables(ctx, Y, name, hi, radii, MV.CELL_SPEED),
                         h=VM.H, w=VM.W)
        assert len(got) == len(recs) and got[-1]["listed"] == 0
        worst = np.zeros(4)
        for k, (g, (listed, st)) in enumerate(zip(got, recs)):
            assert g["listed"] == int(listed.sum())
            worst = np.maximum(worst, compare(VM.cell_id(cell), k, g, listed, st, ymax, rows=VM.H, w=VM.W))
        print("%s, radii %s: %d passes, max |delta| mean %.3e (nearest decision %.3g x its margin)" % (VM.cell_id(cell), radii, len(got), worst[0], nearest))
        assert len(np.unique(got[-1]["count"])) >= 4
        if radii is None:                                             # the polygons and meshes did move: not the moving spheres' frame again
            only = Y.moving_samples(name, VM.W, VM.H, depth, VM.APERTURE, VM.FOCUS, table[:8], lights[:8], MV.spheres_only(shapes[:8], Y.kinds(name)))
            assert int((np.abs(s[:, :8].mean(axis=1) - only.mean(axis=1)) > 0.05).any(axis=1).sum()) == MV.BLURRED_CELLS[VM.cell_id(cell)]


# ---------------------------------------------------------------- 6. the buffers
TALL = ("pool", 3, LR.APERTURE, None, 8, 0.1, 16, 64)                   # 32 x 40: rows = 32


def test_rows_below_the_last_patch_row_and_the_memory_behind_the_buffers_keep_their_bytes(pkg, ctx, Y):
    """32 x 40.  The six buffers and the workspace (seven in all), their eight last rows and a guard region behind each hold NaN /
    BYTE / WORD beforehand; all three tables have rows behind the table_rows the call may read, finite ones that would give
    another picture (1e3)."""
    import torch
    scene, depth, aperture, radii, ns, tol, lo, hi = TALL
    GL.upload(ctx, Y.scene(scene)[0])
    table, lights, shapes = Y.tables(scene, hi, radii)
    s = Y.moving_samples(scene, 32, 40, depth, aperture, LR.FOCUS, table, lights, shapes)
    recs, nearest = CR.run(s, 32, 32, ns, tol, lo, hi)
    ymax = float(np.abs(CR.y_of(s)).max())
    f = Frame(pkg, 40, 32, guard=4096)
    held = {k: v.cpu().numpy().copy() for k, v in f.raw.items()}
    wide = []
    for t in on_device(table, lights, shapes):
        w = torch.full((hi + 64,) + tuple(t.shape[1:]), 1e3, dtype=torch.float64, device="cuda:0")
        w[:hi] = t
        wide.append(w[:hi])                                             # (the wrapper takes the tables' rows for table_rows; the other rows lie behind)
    p = pkg.backend.make_params(workloads.FOV, 40., 32., depth)
    for k, (listed, st) in enumerate(recs):
        ctx.accumulate_converging_moving_device(p, f.sum, f.stats, f.count, aperture, LR.FOCUS, ns, wide[0], wide[1], wide[2], tol, lo, hi, k == 0,
                                                mean=f.mean, rgb8=f.rgb8, mask=f.mask, workspace=f.ws[:f.ws_words])
        got = f.snapshot()
        assert got["listed"] == int(listed.sum())
        compare("32 x 40", k, got, listed, st, ymax)
    assert got["listed"] == 0 and len(np.unique(got["count"][:32])) >= 3
    print("32 x 40: %d passes (nearest decision %.3g x its margin)" % (len(recs), nearest))
    for key, per in (("sum", 3), ("stats", 2), ("count", 1), ("mean", 3), ("rgb8", 3), ("mask", 1)):
        after = f.raw[key].cpu().numpy()
        assert after[32 * 32 * per:].tobytes() == held[key][32 * 32 * per:].tobytes(), "%s: rows 32-39 or the guard" % key
    ws = f.ws.cpu().numpy().view(np.uint32)
    assert f.ws_words == ctx.converge_workspace(p) // 4 and np.all(ws[1 + 1024:] == WORD)


def test_unlisted_pixels_keep_every_byte(pkg, ctx, Y):
    """Three passes of demo-moving-8, then mean, bytes, mask and workspace are filled with sentinels and a fourth pass runs."""
    name = "demo-moving-8"
    scene, depth, aperture, radii, ns, tol, lo, hi = CMV.CASES[name]
    GL.upload(ctx, Y.scene(scene)[0])
    f, tables = Frame(pkg, 32, 32), library_tables(ctx, Y, scene, hi, radii, CMV.SPEED[name])
    for k in range(3):
        moving_pass(pkg, ctx, f, depth, aperture, LR.FOCUS, ns, tol, lo, hi, tables, k == 0)
    before = f.snapshot()
    f.mean.fill_(NAN), f.rgb8.fill_(BYTE), f.mask.fill_(7), f.ws.fill_(WORD)
    moving_pass(pkg, ctx, f, depth, aperture, LR.FOCUS, ns, tol, lo, hi, tables, False)
    after = f.snapshot()
    listed = after["mask"].astype(bool)
    n_listed = int(listed.sum())
    assert set(np.unique(after["mask"])) == {0, 1} and after["listed"] == n_listed and 0 < n_listed < 1024
    assert np.array_equal(after["list"], np.flatnonzero(listed.reshape(-1)))
    assert np.isnan(after["mean"][~listed]).all() and np.all(after["rgb8"][~listed] == BYTE)
    assert not np.isnan(after["mean"][listed]).any()
    for key in ("sum", "stats", "count"):
        assert after[key][~listed].tobytes() == before[key][~listed].tobytes(), key
    assert np.all(after["count"][listed] == before["count"][listed] + ns)
    ws = f.ws.cpu().numpy().view(np.uint32)
    assert np.all(ws[1 + n_listed:] == WORD)                           # nothing behind the list's end
    # without the optional outputs the same sum, stats and count
    g = Frame(pkg, 32, 32)
    for k in range(4):
        moving_pass(pkg, ctx, g, depth, aperture, LR.FOCUS, ns, tol, lo, hi, tables, k == 0, outputs=False)
    bare = g.snapshot()
    assert all(bare[key].tobytes() == after[key].tobytes() for key in ("sum", "stats", "count")) and np.array_equal(bare["list"], after["list"])
    assert np.isnan(bare["mean"]).all() and np.all(bare["rgb8"] == BYTE) and np.all(bare["mask"] == BYTE)


# ---------------------------------------------------------------- 7. the oriented context
def test_oriented_context(pkg, ctx, Y):
    """The demo from the side, area lights, three passes of 8 with tolerance < 0 (the view is the context's: the select rule has
    nothing to do with it, the rays have)."""
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
        radii, ns, hi = (1.5, 3.), 8, 24
        table, lights, shapes = Y.tables("demo", hi, radii)
        s = Y.moving_samples("demo", 32, 32, 3, LR.APERTURE, focus, table, lights, shapes, view)
        fixed = Y.moving_samples("demo", 32, 32, 3, LR.APERTURE, focus, table[:8], lights[:8], shapes[:8])
        ymax = float(np.abs(CR.y_of(s)).max())
        recs, _ = CR.run(s, 32, 32, ns, -1., 0, hi, passes=3)
        f, tables = Frame(pkg, 32, 32), on_device(table, lights, shapes)
        worst = np.zeros(4)
        for k, (listed, st) in enumerate(recs):
            moving_pass(pkg, ctx, f, 3, LR.APERTURE, focus, ns, -1., 0, hi, tables, k == 0)
            worst = np.maximum(worst, compare("demo from the side", k, f.snapshot(), listed, st, ymax))
        print("demo from the side, %d passes: max |delta| mean %.3e" % (len(recs), worst[0]))
        assert np.abs(s[:, :8].mean(axis=1) - fixed.mean(axis=1)).max() > 0.05      # another picture than the fixed view's
    finally:
        ctx.orient(None)


# ---------------------------------------------------------------- 8. the grid
def test_a_capped_grid_changes_nothing(pkg, ctx, Y, monkeypatch):
    """RM_LENS_MAX_BLOCKS = 1 (read at rm_init: a context of its own) caps this shade kernel's grid too and drives its loop over
    the groups of the list and its tail; 64 x 32: two patches a row.  Eight passes of pool-moving-5, the lists as sets."""
    name = "pool-moving-5"
    scene = Y.scene(CMV.CASES[name][0])[0]
    GL.upload(ctx, scene)
    free = run_case(pkg, ctx, Y, name, passes=8, h=32, w=64, every=False)[-1]
    assert 0 < free["listed"] < 2048
    monkeypatch.setenv("RM_LENS_MAX_BLOCKS", "1")
    c = pkg.backend.Context(0)
    try:
        c.upload(scene.flatten())
        got = run_case(pkg, c, Y, name, passes=8, h=32, w=64, every=False)[-1]
        for key in ("sum", "stats", "count", "mean", "rgb8", "mask", "list"):
            assert got[key].tobytes() == free[key].tobytes(), "%s, 1 workgroup: %s" % (name, key)
    finally:
        c.close()


# ---------------------------------------------------------------- 9. the render state
def test_converging_moving_calls_leave_the_render_state_alone(pkg, Y):
    import torch
    demo = workloads.product_scene(pkg, "demo")
    v = velocities_of(Y, "demo")
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 5)
    small = pkg.backend.make_params(workloads.FOV, 32., 64., 5)          # 64 x 32: two patches a row

    def frames(with_calls):
        c = pkg.backend.Context(0)
        try:
            c.upload(demo.flatten())
            out = []
            if with_calls:
                bufs = dict(sum=torch.zeros((32, 64, 3), dtype=torch.float64, device="cuda:0"),
                            stats=torch.zeros((32, 64, 2), dtype=torch.float64, device="cuda:0"),
                            count=torch.zeros((32, 64), dtype=torch.int32, device="cuda:0"))
                tables = on_device(c.lens_sequence(0, 16), np.zeros((16, 2, 3)), c.motion_sequence(0, 16, v, MV.SHUTTER))
            for k in range(3):
                f = np.zeros((64, 64, 3))
                c.render(p, f)
                out.append(f)
                if with_calls and k < 2:                              # before, between and after: calls behind frames 1 and 2
                    before = (c.uploads(), c.launch_stats())
                    ws = c.accumulate_converging_moving_device(small, bufs["sum"], bufs["stats"], bufs["count"], LR.APERTURE, LR.FOCUS, 2, tables[0],
                                                               tables[1], tables[2], 0.05, 2, 16, k == 0)
                    torch.cuda.synchronize()
                    host = np.zeros((32, 64, 3))
                    assert c.render_converging_moving(small, v, MV.SHUTTER, LR.APERTURE, LR.FOCUS, 4, 0.05, 4, 64, host_rgb=host)[1].passes == k + 1
                    assert int(ws[0]) > 0 and bool((bufs["count"] == 2 * (k + 1)).any()) and host.any()
                    assert (c.uploads(), c.launch_stats()) == before
            return out
        finally:
            c.close()

    bare, ticked = frames(False), frames(True)
    for k, (a, b) in enumerate(zip(bare, ticked)):
        assert a.tobytes() == b.tobytes(), "frame %d differs once converging moving calls ran" % (k + 1)


# ---------------------------------------------------------------- 10. errors
def test_refusals_of_the_device_call_leave_the_buffers_alone(pkg, ctx, Y):
    L, B = pkg.lib(), pkg._lib
    depth = 3
    GL.upload(ctx, Y.scene("demo")[0])
    n_shapes = Y.n_shapes("demo")
    p = pkg.backend.make_params(workloads.FOV, 64., 64., depth)
    f = Frame(pkg, 64, 64)
    held = f.snapshot()
    table, lights, shapes = library_tables(ctx, Y, "demo", 64, (1.5, 3.))
    good, conv = B.rm_lens(LR.APERTURE, LR.FOCUS, 4, 0), B.rm_converge(0.05, 16, 64)
    vp = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None

    def untouched():
        now = f.snapshot()
        ws = f.ws.cpu().numpy().view(np.uint32)
        return all(now[k].tobytes() == held[k].tobytes() for k in f.raw) and np.all(ws == WORD)

    def device_call(lens=good, c=conv, t=table, rows=64, o=lights, n_lights=2, so=shapes, ns=n_shapes, params=p, buffers=True, **swap):
        b = dict(sum=f.sum, stats=f.stats, count=f.count, workspace=f.ws, mean=f.mean, rgb8=f.rgb8, mask=f.mask)
        b.update(swap)
        frame = B.rm_converge_frame(*(vp(b[k]) for k in ("sum", "stats", "count", "workspace", "mean", "rgb8", "mask")))
        st = L.rm_accumulate_converging_moving_device(ctx.ptr, C.byref(params), C.byref(lens) if lens is not None else None,
                                                      C.byref(c) if c is not None else None, vp(t), rows, vp(o), n_lights, vp(so), ns, 1,
                                                      C.byref(frame) if buffers else None, None)
        msg = L.rm_last_error(ctx.ptr).decode()
        assert st != 0 and untouched(), msg
        return st, msg

    E = B.RM_ERR_INVALID_ARG
    # the moving shapes' own
    for ns in (0, n_shapes - 1, n_shapes + 1, 2 ** 32 - 1):
        st, msg = device_call(ns=ns)
        assert st == E and "n_shapes" in msg and "the resident scene has %d" % n_shapes in msg
    st, msg = device_call(so=None)
    assert st == E and "NULL shape offsets" in msg
    # the area lights' own: the count is the scene's whatever the table, and the table is required
    for n_lights in (0, 1, 3, 2 ** 32 - 1):
        st, msg = device_call(n_lights=n_lights)
        assert st == E and "n_lights" in msg and "the resident scene has 2" in msg
    st, msg = device_call(o=None)
    assert st == E and "NULL light offsets" in msg
    # rm_converge
    st, msg = device_call(c=B.rm_converge(NAN, 16, 64))
    assert st == E and "tolerance" in msg
    for most in (3, 0, 65, 65537, 2 ** 32 - 1):                        # below n_samples; beyond the table's rows; beyond the library's cap
        st, msg = device_call(c=B.rm_converge(0.05, 16, most))
        assert st == E and "max_samples" in msg, most
    st, msg = device_call(rows=63)                                     # tables shorter than max_samples
    assert st == E and "max_samples" in msg
    assert device_call(c=None)[1].endswith("NULL converge")
    # the buffers
    assert "NULL buffers" in device_call(buffers=False)[1]
    for key in ("sum", "stats", "count", "workspace"):
        st, msg = device_call(**{key: None})
        assert st == E and "NULL " + key in msg
    st, msg = device_call(mean=f.sum)
    assert st == E and "device_mean == device_sum" in msg
    st, msg = device_call(t=None)
    assert st == E and "table" in msg
    # the lens and the params
    for lens, word in ((B.rm_lens(-1., LR.FOCUS, 4, 0), "aperture"), (B.rm_lens(LR.APERTURE, 0., 4, 0), "focus"), (B.rm_lens(LR.APERTURE, LR.FOCUS, 65, 0), "n_samples")):
        st, msg = device_call(lens=lens)
        assert st == E and word in msg
    assert "NULL lens" in device_call(lens=None)[1]
    odd = pkg.backend.make_params(workloads.FOV, 64., 100., depth)
    assert device_call(params=odd)[0] == B.RM_ERR_DIMENSIONS
    huge = pkg.backend.make_params(workloads.FOV, 65536., 32768., depth)   # rows * frame_width = 2^31: checked before any pointer is touched
    st, msg = device_call(params=huge)
    assert st == B.RM_ERR_DIMENSIONS and "2^31" in msg
    deep = pkg.backend.make_params(workloads.FOV, 64., 64., 1000)
    assert device_call(params=deep)[0] == B.RM_ERR_DEPTH
    # a scene without a sphere: the moving spheres' call takes a NULL shape table, this one refuses it
    GL.upload(ctx, Y.scene("cornell")[0])
    nc, lc = Y.n_shapes("cornell"), Y.n_lights("cornell")
    frame = B.rm_converge_frame(vp(f.sum), vp(f.stats), vp(f.count), vp(f.ws), vp(f.mean), vp(f.rgb8), vp(f.mask))
    zl = on_device(np.zeros((64, lc, 3)))[0]
    assert L.rm_accumulate_converging_moving_device(ctx.ptr, C.byref(p), C.byref(good), C.byref(conv), vp(table), 64, vp(zl), lc, None, nc, 1,
                                                    C.byref(frame), None) == E
    assert "NULL shape offsets" in L.rm_last_error(ctx.ptr).decode() and untouched()
    GL.upload(ctx, Y.scene("demo")[0])
    fresh = pkg.backend.Context(0)
    try:
        frame = B.rm_converge_frame(vp(f.sum), vp(f.stats), vp(f.count), vp(f.ws), None, None, None)
        assert L.rm_accumulate_converging_moving_device(fresh.ptr, C.byref(p), C.byref(good), C.byref(conv), vp(table), 64, vp(lights), 2, vp(shapes),
                                                        n_shapes, 1, C.byref(frame), None) == B.RM_ERR_NO_SCENE
    finally:
        fresh.close()
    assert untouched()
    # the Python wrapper hands the library's refusal on
    with pytest.raises(B.BackendError, match="n_shapes"):
        ctx.accumulate_converging_moving_device(p, f.sum, f.stats, f.count, LR.APERTURE, LR.FOCUS, 4, table, lights, shapes[:, :-1].contiguous(),
                                                0.05, 16, 64, True)
    assert untouched()
    # what is tolerated: a frame without a whole patch row
    short = Frame(pkg, 31, 64)
    moving_pass(pkg, ctx, short, depth, LR.APERTURE, LR.FOCUS, 4, 0.05, 16, 64, (table, lights, shapes), True)
    got = short.snapshot()                                              # rows == 0: RM_OK, nothing done (the list's length is not cleared either)
    assert np.isnan(got["sum"]).all() and np.all(got["count"] == WORD) and np.all(short.ws.cpu().numpy().view(np.uint32) == WORD)


def test_a_scene_with_no_shape_at_all_takes_a_null_table(pkg, ctx):
    """Lights and a camera alone: every ray leaves the scene, and neither the device call nor the tick asks for shape offsets."""
    import torch
    L, B = pkg.lib(), pkg._lib
    empty = pkg.Scene.new()
    empty.lights.append(pkg.create_light(pkg.Vec3f(0., 5., 0.), pkg.Vec3f(1., 1., 1.), 1.))
    GL.upload(ctx, empty)
    p = pkg.backend.make_params(workloads.FOV, 32., 32., 3)
    lens, conv = B.rm_lens(LR.APERTURE, LR.FOCUS, 4, 0), B.rm_converge(0.1, 4, 16)
    table = torch.from_numpy(PR.lens_sequence(0, 16)).to("cuda:0")
    lights = torch.zeros((16, 1, 3), dtype=torch.float64, device="cuda:0")
    f = Frame(pkg, 32, 32)
    vp = lambda x: C.c_void_p(x.data_ptr())
    frame = B.rm_converge_frame(vp(f.sum), vp(f.stats), vp(f.count), vp(f.ws), vp(f.mean), vp(f.rgb8), vp(f.mask))
    for k in range(2):
        assert L.rm_accumulate_converging_moving_device(ctx.ptr, C.byref(p), C.byref(lens), C.byref(conv), vp(table), 16, vp(lights), 1, None, 0,
                                                        1 if k == 0 else 0, C.byref(frame), None) == 0, L.rm_last_error(ctx.ptr)
        got = f.snapshot()
        assert got["listed"] == (1024 if k == 0 else 0)                # a constant picture settles at min_samples
    assert not np.isnan(got["mean"]).any() and (got["mean"] == got["mean"][0, 0]).all() and np.all(got["count"] == 4)
    host, report = np.full((32, 32, 3), NAN), B.rm_converge_report()
    assert L.rm_render_converging_moving(ctx.ptr, C.byref(p), C.byref(lens), C.byref(conv), None, 0, None, 0, 1., 1, host.ctypes.data_as(C.POINTER(C.c_double)),
                                         None, C.byref(report), None) == 0, L.rm_last_error(ctx.ptr)
    assert (report.listed, report.passes) == (1024, 1) and host.tobytes() == got["mean"].tobytes()


# ---------------------------------------------------------------- 11. the tick
CPP_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "rusty_marcher.hpp"
using namespace rusty_marcher;
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    scene::Scene sc = scene::Scene::create_default();
    framebuffer::FrameBuffer fb = framebuffer::create_frame_buffer(32, 32);
    renderer::Renderer r = renderer::create_renderer(1.5, 32., 32.);
    r.max_depth = 3;
    std::vector<Vec3f> v;
    for (int k = 0; k < argc - 2; k += 3) v.push_back(Vec3f{std::atof(argv[2 + k]), std::atof(argv[3 + k]), std::atof(argv[4 + k])});
    const rm_converge c{0.1, 16u, 256u};
    rm_converge_report rep = r.render_converging_moving(fb, sc, v, 1., c, 8u, {}, 0.4, 5., true);
    std::printf("first %u %u\n", rep.listed, rep.passes);
    while (rep.listed > 0u) rep = r.render_converging_moving(fb, sc, v, 1., c, 8u, {}, 0.4, 5.);
    std::printf("done %u %llu %u %u\n", rep.passes, (unsigned long long)rep.samples_cast, rep.max_count, r.last_samples);
    std::FILE *f = std::fopen(argv[1], "wb");
    if (!f) return 3;
    for (const auto &row : fb.buffer) std::fwrite(row.data(), sizeof(Vec3f), row.size(), f);
    std::fclose(f);
    rep = r.render_converging_moving(fb, sc, v, 1., c, 8u, {}, 0.4, 5.);
    std::printf("again %u %u\n", rep.listed, rep.passes);
    rep = r.render_converging(fb, sc, c, 8u, {}, 0.4, 5.);
    std::printf("still %u %u\n", rep.listed, rep.passes);
    return 0;
}
"""


def test_the_tick_through_c_python_and_the_cpp_mirror(pkg, entry, ctx, Y, capsys, tmp_path):
    assert workloads.FOV == 1.5 and (LR.APERTURE, LR.FOCUS, MV.SHUTTER) == (0.4, 5., 1.)
    L, B = pkg.lib(), pkg._lib
    name = "demo-moving-8"
    scene_name, depth, aperture, radii, ns, tol, lo, hi = CMV.CASES[name]
    n_passes, cast, _ = CMV.FOUND[name]
    scene = Y.scene(scene_name)[0]
    GL.upload(ctx, scene)
    kinds = Y.kinds(scene_name)
    v = velocities_of(Y, scene_name, CMV.SPEED[name])
    only = MR.velocities(kinds)                                        # the spheres' velocities, zero for every other shape
    polygon = kinds.index(MV.ORC_POLYGON)
    assert v[polygon].any() and not only[polygon].any()
    device = run_case(pkg, ctx, Y, name)
    assert len(device) == n_passes
    p = pkg.backend.make_params(workloads.FOV, 32., 32., depth)
    host, host8 = np.full((32, 32, 3), -3.5), np.full((32, 32, 3), 7, np.uint8)

    def tick(restart=False, vel=v, shutter=MV.SHUTTER, t=tol, r=None, n=ns, most=hi, **kw):
        return ctx.render_converging_moving(p, vel, shutter, aperture, LR.FOCUS, n, t, lo, most, radii=r, restart=restart, **kw)

    def motion(restart=False, vel=only, **kw):
        return ctx.render_converging_motion(p, vel, MV.SHUTTER, aperture, LR.FOCUS, ns, tol, lo, hi, restart=restart, **kw)

    def still(restart=False, **kw):
        return ctx.render_converging(p, aperture, LR.FOCUS, ns, tol, lo, hi, restart=restart, **kw)

    before = (ctx.uploads(), ctx.launch_stats())
    # tick by tick the device call's frame, to the end: the three resident prefixes grow as the frame does
    seen = 0
    for k in range(n_passes):
        timing, rep = tick(restart=(k == 0), host_rgb=host, host_rgb8=host8)
        seen += device[k]["listed"]
        assert (rep.listed, rep.passes, rep.samples_cast) == (device[k]["listed"], k + 1, seen * ns), k
        assert rep.max_count == int(device[k]["count"].max())
        assert host.tobytes() == device[k]["mean"].tobytes() and host8.tobytes() == device[k]["rgb8"].tobytes(), k
        assert timing.kernel_ms > 0. and timing.total_ms >= timing.kernel_ms
    assert rep.listed == 0 and rep.samples_cast == cast
    # a finished picture: nothing is launched, the report says 0, the frame stands
    for _ in range(2):
        again, again8 = np.full((32, 32, 3), NAN), np.full((32, 32, 3), BYTE, np.uint8)
        timing, rep = tick(host_rgb=again, host_rgb8=again8)
        assert timing.kernel_ms == 0. and (rep.listed, rep.passes, rep.samples_cast) == (0, n_passes, cast)
        assert again.tobytes() == host.tobytes() and again8.tobytes() == host8.tobytes()
    assert (ctx.uploads(), ctx.launch_stats()) == before              # the counters of renders and uploads were left alone
    # a tightened tolerance continues: the yardstick's next pass on the finished state, not a fresh frame
    s = CMV.case_samples(Y, name)
    recs, _ = CR.run(s, 32, 32, ns, tol, lo, hi)
    st = recs[-1][1].copy()
    listed, near = CR.one_pass(st, s, ns, 0.05, lo, hi, False, float(np.abs(CR.y_of(s)).max()))
    assert 0 < int(listed.sum()) < 1024
    timing, rep = tick(t=0.05, host_rgb=again)
    assert (rep.listed, rep.passes, rep.samples_cast) == (int(listed.sum()), n_passes + 1, cast + int(listed.sum()) * ns)
    assert GL.worst(again, st.mean.reshape(32, 32, 3)) < TIGHT and timing.kernel_ms > 0.
    # ... and another n_samples or cap continues too
    assert tick(t=0.05, n=4)[1].passes == n_passes + 2 and tick(t=0.05, most=512)[1].passes == n_passes + 3
    # what begins the frame again, one at a time, each followed by a tick that goes on: restart; a changed velocity of a polygon,
    # and back; a changed shutter, and back; radii, and none
    pushed = v.copy()
    pushed[polygon] = v[polygon] * 1.5
    for kw in (dict(restart=True), dict(vel=pushed), dict(), dict(shutter=0.5), dict(), dict(r=(1.5, 3.)), dict()):
        first = tick(**kw)[1]
        assert (first.listed, first.passes, first.samples_cast, first.max_count) == (1024, 1, 1024 * ns, ns), kw
        kw.pop("restart", None)
        assert tick(**kw)[1].passes == 2
    # a switch to and from render_converging_motion with equal sphere-only velocities: the ticks share one state, not one frame
    moved, spheres = np.full((32, 32, 3), NAN), np.full((32, 32, 3), NAN)
    assert tick(vel=only)[1].passes == 1 and tick(vel=only, host_rgb=moved)[1].passes == 2
    assert motion()[1].passes == 1 and motion(host_rgb=spheres)[1].passes == 2     # moving -> motion
    assert moved.tobytes() == spheres.tobytes() and not np.isnan(moved).any()      # (zero rows but the spheres': the same bytes)
    assert tick(vel=only)[1].passes == 1                               # motion -> moving
    # ... and to and from render_converging
    assert still()[1].passes == 1 and still()[1].passes == 2           # moving -> plain
    assert tick()[1].passes == 1                                       # plain -> moving
    first = tick(restart=True, host_rgb=again)[1]
    assert first.passes == 1 and again.tobytes() == device[0]["mean"].tobytes()
    # the C entry point itself
    lens, conv, report = B.rm_lens(aperture, LR.FOCUS, ns, 0), B.rm_converge(tol, lo, hi), B.rm_converge_report()
    D, V3 = C.POINTER(C.c_double), C.POINTER(B.rm_vec3)
    vc = np.ascontiguousarray(v)
    for k in range(3):
        st_ = L.rm_render_converging_moving(ctx.ptr, C.byref(p), C.byref(lens), C.byref(conv), None, 0, vc.ctypes.data_as(V3), len(vc), MV.SHUTTER,
                                            1 if k == 0 else 0, again.ctypes.data_as(D), None, C.byref(report), None)
        assert st_ == 0 and (report.listed, report.passes) == (device[k]["listed"], k + 1)
    assert again.tobytes() == device[2]["mean"].tobytes()
    # refused calls in between change nothing of the frame: a wrong count; a velocity that is not finite, on a polygon; the
    # shutter; the rule
    for bad, n_shapes, shutter, c, word in ((v[:-1], len(v) - 1, 1., conv, "n_shapes"),
                                            (np.where(np.arange(len(v))[:, None] == polygon, NAN, v), len(v), 1., conv, "velocities[%d]" % polygon),
                                            (v, len(v), -1e-9, conv, "shutter"), (v, len(v), NAN, conv, "shutter"),
                                            (v, len(v), 1., B.rm_converge(NAN, lo, hi), "tolerance")):
        bad = np.ascontiguousarray(bad)
        report.passes, held = 77, again.copy()
        st_ = L.rm_render_converging_moving(ctx.ptr, C.byref(p), C.byref(lens), C.byref(c), None, 0, bad.ctypes.data_as(V3), n_shapes, shutter, 0,
                                            again.ctypes.data_as(D), None, C.byref(report), None)
        msg = L.rm_last_error(ctx.ptr).decode()
        assert st_ == B.RM_ERR_INVALID_ARG and report.passes == 77 and again.tobytes() == held.tobytes(), msg
        assert word in msg and "rm_render_converging_moving" in msg, msg
    # the moving spheres' tick keeps its refusal, word for word, and leaves this frame alone
    with pytest.raises(B.BackendError, match=r"rm_render_converging_motion: velocities\[%d\] is not zero and shape %d is not a sphere \(only spheres move\)"
                       % (polygon, polygon)):
        motion(vel=v)
    assert tick(host_rgb=again)[1].passes == 4 and again.tobytes() == device[3]["mean"].tobytes()   # the frame went through all that untouched
    fresh = pkg.backend.Context(0)
    try:
        report.passes = 77
        assert L.rm_render_converging_moving(fresh.ptr, C.byref(p), C.byref(lens), C.byref(conv), None, 0, vc.ctypes.data_as(V3), len(vc), 1., 0, None,
                                             None, C.byref(report), None) == B.RM_ERR_NO_SCENE and report.passes == 77
    finally:
        fresh.close()
    # a frame without a whole patch row: RM_OK with a report of zeros
    tiny = pkg.backend.make_params(workloads.FOV, 31., 64., depth)
    rep = ctx.render_converging_moving(tiny, v, MV.SHUTTER, aperture, LR.FOCUS, ns, tol, lo, hi)[1]
    assert (rep.listed, rep.passes, rep.samples_cast, rep.max_count) == (0, 0, 0, 0)
    # area lights and moving shapes through the tick: the device call's frame with all three sequences, three ticks
    soft = run_case(pkg, ctx, Y, "demo-moving-soft-64", passes=3)
    sd = CMV.CASES["demo-moving-soft-64"]
    for k in range(3):
        rep = ctx.render_converging_moving(p, v, MV.SHUTTER, sd[2], LR.FOCUS, sd[4], sd[5], sd[6], sd[7], radii=sd[3], restart=(k == 0), host_rgb=host)[1]
        assert rep.listed == soft[k]["listed"] and host.tobytes() == soft[k]["mean"].tobytes()
    # the two converging ticks alternating on one context -- every switch begins the frame again -- equal contexts that make one
    # kind of call
    a, b = pkg.backend.Context(0), pkg.backend.Context(0)
    try:
        a.upload(scene.flatten())
        b.upload(scene.flatten())
        alt_moving, alt_motion, one_moving, one_motion = (np.full((32, 32, 3), NAN) for _ in range(4))
        for k in range(2):
            assert tick(host_rgb=alt_moving)[1].passes == 1 and motion(host_rgb=alt_motion)[1].passes == 1
        assert a.render_converging_moving(p, v, MV.SHUTTER, aperture, LR.FOCUS, ns, tol, lo, hi, host_rgb=one_moving)[1].passes == 1
        assert b.render_converging_motion(p, only, MV.SHUTTER, aperture, LR.FOCUS, ns, tol, lo, hi, host_rgb=one_motion)[1].passes == 1
        assert alt_moving.tobytes() == one_moving.tobytes() and alt_motion.tobytes() == one_motion.tobytes()
        assert alt_moving.tobytes() != alt_motion.tobytes() and not np.isnan(alt_moving).any()
    finally:
        a.close()
        b.close()
    # Renderer.render_converging_moving and render_converged_moving: the prints of render(), the report returned
    r = pkg.create_renderer(workloads.FOV, 32., 32.)
    r.max_depth = depth
    fb = pkg.create_frame_buffer(32, 32)
    vel = [pkg.Vec3f(*e) for e in v]
    capsys.readouterr()
    rep = r.render_converging_moving(fb, scene, vel, MV.SHUTTER, tol, ns, lo, hi, aperture=aperture, focus=LR.FOCUS, restart=True)
    out = capsys.readouterr().out
    assert "Scene rendered in " in out and "compute units used" in out
    assert (rep.listed, rep.passes) == (1024, 1) and r.last_samples == ns and r.last_report is rep and r.last_timing.kernel_ms > 0.
    assert fb.buffer.tobytes() == device[0]["mean"].tobytes()
    rep = r.render_converged_moving(fb, scene, vel, MV.SHUTTER, tol, ns, lo, hi, aperture=aperture, focus=LR.FOCUS)
    assert (rep.listed, rep.passes, rep.samples_cast) == (0, n_passes, cast) and fb.buffer.tobytes() == device[-1]["mean"].tobytes()
    # the C++ mirror, from compiled code
    src, exe, dump = tmp_path / "tick.cpp", tmp_path / "tick", tmp_path / "tick.f64"
    src.write_text(CPP_MAIN)
    lib_dir = os.path.join(entry.PKG_DIR, "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(entry.ROOT, "include"), "-I", os.path.join(entry.PKG_DIR, "host"),
                           str(src), "-o", str(exe), "-L", lib_dir, "-lrusty_marcher_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath," + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")])
    log = subprocess.check_output([str(exe), str(dump)] + [repr(float(x)) for x in v.reshape(-1)]).decode()
    top = int(device[-1]["count"].max())
    assert [l for l in log.splitlines() if l.split()[0] in ("first", "done", "again", "still")] == \
        ["first 1024 1", "done %d %d %d %d" % (n_passes, cast, top, top), "again 0 %d" % n_passes, "still 1024 1"]
    assert np.fromfile(str(dump)).tobytes() == device[-1]["mean"].tobytes()


def test_the_cornell_box_ticks_without_a_sphere(pkg, ctx, Y):
    """The staging rule: the Cornell box holds meshes and no sphere; the converging tick of the moving spheres keeps no shape
    table for such a scene, this one must -- three ticks are the device call's three passes over the library's tables."""
    name = "cornell-moving-8"
    scene_name, depth, aperture, radii, ns, tol, lo, hi = CMV.CASES[name]
    GL.upload(ctx, Y.scene(scene_name)[0])
    assert MV.ORC_SPHERE not in Y.kinds(scene_name)
    v = velocities_of(Y, scene_name, CMV.SPEED[name])
    p = pkg.backend.make_params(workloads.FOV, 32., 32., depth)
    device = run_case(pkg, ctx, Y, name, passes=4)
    host = np.full((32, 32, 3), NAN)
    for k in range(4):
        rep = ctx.render_converging_moving(p, v, MV.SHUTTER, aperture, LR.FOCUS, ns, tol, lo, hi, restart=(k == 0), host_rgb=host)[1]
        assert (rep.listed, rep.passes) == (device[k]["listed"], k + 1) and host.tobytes() == device[k]["mean"].tobytes(), k
    assert 0 < rep.listed < 1024
    # the meshes did move: zero velocities through the moving spheres' tick, which obeys them on a scene without spheres, give
    # another picture after the same four ticks
    still = np.full((32, 32, 3), NAN)
    for k in range(4):
        ctx.render_converging_motion(p, v * 0., MV.SHUTTER, aperture, LR.FOCUS, ns, tol, lo, hi, restart=(k == 0), host_rgb=still)
    assert int((np.abs(still - host) > 0.05).any(axis=2).sum()) > VM.SHARE * 1024


# ---------------------------------------------------------------- 12. the two ticks beside each other
def moving_ticks(pkg, Y, steps):
    """The ticks `steps` names -- "p" rm_render_progressive_moving, "c" rm_render_converging_moving with a negative tolerance,
    so every pixel is listed -- on a context of their own, 4 samples each, none with `restart` -> every tick's host_rgb."""
    demo = workloads.product_scene(pkg, "demo")
    v = velocities_of(Y, "demo")
    p = pkg.backend.make_params(workloads.FOV, 32., 32., 2)
    c = pkg.backend.Context(0)
    try:
        c.upload(demo.flatten())
        out = []
        for kind in steps:
            host = np.full((32, 32, 3), NAN)
            if kind == "p":
                c.render_progressive_moving(p, v, MV.SHUTTER, LR.APERTURE, LR.FOCUS, 4, host_rgb=host)
            else:
                rep = c.render_converging_moving(p, v, MV.SHUTTER, LR.APERTURE, LR.FOCUS, 4, -1., 0, 64, host_rgb=host)[1]
                assert rep.listed == 1024
            assert np.isfinite(host).all() and host.any()
            out.append(host)
        return out
    finally:
        c.close()


def test_the_two_moving_ticks_alternating_on_one_context_are_each_kinds_own_frames(pkg, Y):
    """rm_ctx::progressive and rm_ctx::converging share nothing: three ticks of each, alternating on one context, give byte for
    byte what the same three ticks give on a context that makes only that kind of call -- and, a negative tolerance being the
    plain run, both kinds give the same three frames."""
    mixed = moving_ticks(pkg, Y, "pcpcpc")
    for at, kind in enumerate("pc"):
        alone = moving_ticks(pkg, Y, kind * 3)
        assert alone[0].tobytes() != alone[2].tobytes()                 # (the frame goes on from tick to tick)
        for k in range(3):
            assert mixed[2 * k + at].tobytes() == alone[k].tobytes(), "tick %d of kind %s" % (k + 1, kind)
    for k in range(3):
        assert mixed[2 * k].tobytes() == mixed[2 * k + 1].tobytes()
