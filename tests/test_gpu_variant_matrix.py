"""Every instantiation of the sample-shading kernels against the oracle (-m gpu).  Eight kernel families run
radiance_steps<BVH, POW, STACK, LIGHTS> (csrc/rm_radiance_step.inc), and each launcher picks the instantiation by the scene
image (a hierarchy or none; integer exponents or not) and by max_depth <= 5; the converging frames also by whether light
offsets are given.  The cells of tests/variant_matrix.py are scenes and depths at which every one of these facts matters:
tests/test_variant_matrix.py pins on the CPU that a cell takes the kernel it claims, that the oracle alone tells it from its
neighbours (12.5 against 12; one level less deep) on more than 5 % of the rays and pixels, and that a ray fills the stack.

Which test launches which instantiation -- R test_radiance, F test_refine, L test_lens, P test_progressive, S test_soft,
C test_converging[stored], O test_converging[offsets], B test_bounce, CB test_converging_bounce[stored], OB
test_converging_bounce[offsets], each at the cell named on the left (`mesh-integer-5` runs the fifth line's kernels once
more, over a triangle hierarchy):

    cell                  BVH  POW      STACK  radiance refine lens accum soft converge converge+offsets bounce converge-bounce +offsets
    flat-integer-5        no   INTEGER   4        R       F     L    P     S     C         O               B       CB            OB
    flat-integer-6        no   INTEGER  32        R       F     L    P     S     C         O               B       CB            OB
    flat-generic-5        no   GENERIC   4        R       F     L    P     S     C         O               B       CB            OB
    flat-generic-6        no   GENERIC  32        R       F     L    P     S     C         O               B       CB            OB
    spheres-integer-5     yes  INTEGER   4        R       F     L    P     S     C         O               B       CB            OB
    spheres-integer-6     yes  INTEGER  32        R       F     L    P     S     C         O               B       CB            OB
    spheres-generic-5     yes  GENERIC   4        R       F     L    P     S     C         O               B       CB            OB
    spheres-generic-6     yes  GENERIC  32        R       F     L    P     S     C         O               B       CB            OB

8 x 5 + 8 x 2 = 56, and 8 + 8 x 2 = 24 of the diffuse bounce (rm_bounce.hip, rm_converge_bounce.hip): 80.  (C and O also
launch the accum and the soft kernels of their line, CB and OB the bounce kernel: the plain runs beside them.)

Every channel of every ray or pixel within TIGHT = 1e-9 of the oracle, nothing left out and nothing NaN; what leaves the scene
is exactly +0; every output holds a sentinel beforehand; what the header calls byte for byte is demanded byte for byte.  The
largest deviations observed on an MI355X are recorded in DESIGN.md section 6k."""
import os

import numpy as np
import pytest

import antialias_reference as AR
import bounce_reference as BR
import converge_reference as CR
import lens_reference as LR
import progressive_reference as PR
import radiance_reference as RR
import soft_reference as SR
import test_gpu_antialias as GA
import test_gpu_bounce as GB
import test_gpu_converge as GC
import test_gpu_converge_bounce as GCB
import test_gpu_lens as GL
import test_gpu_parity as GPAR
import test_gpu_progressive as GP
import test_gpu_query as GQ
import test_gpu_soft as GS
import variant_matrix as VM
import workloads

pytestmark = pytest.mark.gpu

TIGHT = VM.TIGHT
W, H = VM.W, VM.H
NAN = float("nan")
cells = pytest.mark.parametrize("cell", VM.CELLS, ids=VM.cell_id)


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_variant_matrix_gpu"))


@pytest.fixture(scope="module")
def matrix(pkg, O, orc):
    return VM.Matrix(pkg, O, orc)


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return CR.Yardstick(pkg, O, orc)                                   # (with the lens, progressive and soft references' frames)


@pytest.fixture(scope="module")
def A(pkg, O, orc):
    return AR.Yardstick(pkg, O, orc)


@pytest.fixture(scope="module")
def B(pkg, O, entry, orc, tmp_path_factory):
    return BR.Yardstick(pkg, O, orc, BR.compile_helper(O, entry, tmp_path_factory.mktemp("orb_variant_matrix_gpu")))


def load(ctx, matrix, yardstick, cell):
    """Uploads the cell's scene -> its name in `yardstick` (where one is given)."""
    bvh, generic, _ = cell
    pair = matrix.pair(bvh, generic)
    GL.upload(ctx, pair[0])
    return VM.register(yardstick, matrix.name(bvh, generic), pair) if yardstick is not None else None


def held(got, ref, what, bound=TIGHT):
    """Every channel within `bound`, nothing NaN, and exactly +0 wherever the reference is exactly zero in every channel --
    which must happen somewhere.  -> the worst deviation."""
    got, ref = got.reshape(-1, 3), ref.reshape(-1, 3)
    assert got.shape == ref.shape and not np.isnan(got).any(), what
    delta = float(np.abs(got - ref).max())
    gone = ~(ref != 0.).any(axis=1)
    assert gone.any() and not got[gone].view(np.uint64).any(), "%s: %d of %d rays or pixels into the sky are not +0" % (
        what, int(got[gone].view(np.uint64).any(axis=1).sum()), int(gone.sum()))
    assert delta < bound, "%s: max |delta| %.3e" % (what, delta)
    return delta


# ---------------------------------------------------------------- radiance queries
@cells
def test_radiance(pkg, ctx, matrix, cell):
    import torch
    bvh, generic, depth = cell
    load(ctx, matrix, None, cell)
    got = ctx.radiance(matrix.o, matrix.d, max_depth=depth, background=RR.BACKGROUND)
    d_rays = held(got, matrix.rays(bvh, generic, depth), "rays")
    p = pkg.backend.make_params(workloads.FOV, float(H), float(W), depth)
    d_samples = held(ctx.radiance_samples(p, matrix.xy), matrix.samples(bvh, generic, depth), "samples")
    # the device variant into a tensor of its own
    dev = ctx.radiance_device(torch.from_numpy(np.array(matrix.o)).to("cuda:0"), torch.from_numpy(np.array(matrix.d)).to("cuda:0"),
                              max_depth=depth, background=RR.BACKGROUND)
    assert dev.cpu().numpy().tobytes() == got.tobytes()
    print("%s radiance: max |delta| rays %.3e, samples %.3e" % (VM.cell_id(cell), d_rays, d_samples))


# ---------------------------------------------------------------- adaptive refinement
@cells
def test_refine(pkg, ctx, matrix, A, cell):
    bvh, generic, depth = cell
    name = load(ctx, matrix, A, cell)
    run = GA.Run(pkg, ctx, W, H, depth, VM.REFINE_N, VM.REFINE_THRESHOLD, frame_fill=NAN)
    assert GA.worst(run.rendered, A.frame(name, W, H, depth)) < TIGHT
    m_ref, f_ref = A.refined(name, W, H, depth, VM.REFINE_N, VM.REFINE_THRESHOLD)
    assert 0 < int(m_ref.sum()) < W * H                                # a proper subset
    GA.check_against(run, m_ref, f_ref, H, "%s refine" % VM.cell_id(cell))
    assert not np.isnan(run.frame).any()
    # ... and with every pixel refined, the sky's among them
    every = GA.Run(pkg, ctx, W, H, depth, VM.REFINE_N, -1., frame_fill=NAN)
    m_all, f_all = A.refined(name, W, H, depth, VM.REFINE_N, -1.)
    assert every.count == W * H and m_all.all()
    print("%s refine: max |delta| over every pixel %.3e" % (VM.cell_id(cell), held(every.frame, f_all, "refine, every pixel")))


# ---------------------------------------------------------------- lens frames
@cells
def test_lens(pkg, ctx, matrix, Y, cell):
    bvh, generic, depth = cell
    name = load(ctx, matrix, Y, cell)
    table = ctx.lens_table(VM.LENS_SAMPLES)
    got = GL.lens_frame(pkg, ctx, W, H, depth, VM.APERTURE, VM.FOCUS, table, fill=NAN)
    ref = Y.frame(name, W, H, depth, VM.APERTURE, VM.FOCUS, table)
    sharp = Y.frame(name, W, H, depth, 0., VM.FOCUS, table)
    assert int((np.abs(ref - sharp) > 0.05).any(axis=2).sum()) > 50    # the lens does blur
    print("%s lens: max |delta| %.3e" % (VM.cell_id(cell), held(got, ref, "lens")))


# ---------------------------------------------------------------- progressive frames
@cells
def test_progressive(pkg, ctx, matrix, Y, cell):
    bvh, generic, depth = cell
    name = load(ctx, matrix, Y, cell)
    table = ctx.lens_sequence(0, 10)
    total, mean, rgb8 = GP.run_passes(pkg, ctx, W, H, depth, VM.APERTURE, VM.FOCUS, table, (5, 5))
    ref_sum, ref_mean = Y.progressive(name, W, H, depth, VM.APERTURE, VM.FOCUS, table, (5, 5))
    d_mean, d_sum = held(mean, ref_mean, "mean"), held(total, ref_sum, "sum", 10 * TIGHT)
    assert rgb8.tobytes() == PR.to_bytes(mean).tobytes()
    one = GP.run_passes(pkg, ctx, W, H, depth, VM.APERTURE, VM.FOCUS, table, (10,))
    for a, b, what in zip((total, mean, rgb8), one, ("sum", "mean", "bytes")):
        assert a.tobytes() == b.tobytes(), "%s after two passes of 5 is not the one pass of 10's" % what
    print("%s progressive: max |delta| mean %.3e, sum %.3e" % (VM.cell_id(cell), d_mean, d_sum))


# ---------------------------------------------------------------- soft-shadow frames
@cells
def test_soft(pkg, ctx, matrix, Y, cell):
    bvh, generic, depth = cell
    name = load(ctx, matrix, Y, cell)
    table, offsets = ctx.lens_sequence(0, 10), ctx.light_sequence(0, 10, VM.RADII)
    assert offsets.tobytes() == SR.light_sequence(0, 10, VM.RADII).tobytes()
    total, mean, rgb8 = GS.run_soft(pkg, ctx, W, H, depth, VM.APERTURE, VM.FOCUS, table, offsets, (5, 5))
    ref_sum, ref_mean = Y.soft(name, W, H, depth, VM.APERTURE, VM.FOCUS, table, offsets, (5, 5))
    d_mean, d_sum = held(mean, ref_mean, "mean"), held(total, ref_sum, "sum", 10 * TIGHT)
    assert rgb8.tobytes() == PR.to_bytes(mean).tobytes()
    one = GS.run_soft(pkg, ctx, W, H, depth, VM.APERTURE, VM.FOCUS, table, offsets, (10,))
    for a, b, what in zip((total, mean, rgb8), one, ("sum", "mean", "bytes")):
        assert a.tobytes() == b.tobytes(), "%s after two passes of 5 is not the one pass of 10's" % what
    hard = Y.progressive(name, W, H, depth, VM.APERTURE, VM.FOCUS, table, (5, 5))[1]
    assert int((np.abs(ref_mean - hard) > 0.05).any(axis=2).sum()) > 20      # the lights did move
    # zero offsets: the progressive frame
    zeros = np.zeros((10, len(VM.RADII), 3))
    zeros[5:] = -0.
    plain = GP.run_passes(pkg, ctx, W, H, depth, VM.APERTURE, VM.FOCUS, table, (5, 5))
    still = GS.run_soft(pkg, ctx, W, H, depth, VM.APERTURE, VM.FOCUS, table, zeros, (5, 5))
    for a, b, what in zip(still, plain, ("sum", "mean", "bytes")):
        assert a.tobytes() == b.tobytes(), "%s with zero offsets is not the progressive frame's" % what
    print("%s soft: max |delta| mean %.3e, sum %.3e" % (VM.cell_id(cell), d_mean, d_sum))


# ---------------------------------------------------------------- converging frames
@pytest.mark.parametrize("offsets", [False, True], ids=["stored", "offsets"])
@cells
def test_converging(pkg, ctx, matrix, Y, cell, offsets):
    bvh, generic, depth = cell
    ns, tol, lo, hi = VM.CONVERGE
    radii = VM.RADII if offsets else None
    name = load(ctx, matrix, Y, cell)
    s = Y.samples(name, W, H, depth, VM.APERTURE, VM.FOCUS, hi, radii)
    ymax = float(np.abs(CR.y_of(s)).max())
    recs, nearest = CR.run(s, W, H, ns, tol, lo, hi)
    f, tables = GC.Frame(pkg, H, W), GC.device_tables(ctx, hi, radii)
    worst = np.zeros(4)
    for k, (listed, st) in enumerate(recs):
        GC.converge_pass(pkg, ctx, f, depth, VM.APERTURE, VM.FOCUS, ns, tol, lo, hi, tables, k == 0)
        got = f.snapshot()
        assert got["listed"] == int(listed.sum()), "pass %d" % k
        worst = np.maximum(worst, GC.compare(VM.cell_id(cell), k, got, listed, st, ymax))
    assert got["listed"] == 0                                          # the last pass of the reference lists nothing
    held(got["mean"], recs[-1][1].mean, "mean")
    # tolerance < 0: the plain run -- progressive with stored lights, soft with offset lights -- byte for byte
    plain = GC.plain_snapshots(pkg, ctx, depth, VM.APERTURE, VM.FOCUS, ns, 2, radii)
    g = GC.Frame(pkg, H, W)
    for k in range(2):
        GC.converge_pass(pkg, ctx, g, depth, VM.APERTURE, VM.FOCUS, ns, -1., lo, hi, tables, k == 0)
        got = g.snapshot()
        assert got["listed"] == W * H and np.all(got["count"] == ns * (k + 1))
        for key, ref in zip(("sum", "mean", "rgb8"), plain[ns * (k + 1)]):
            assert got[key].tobytes() == ref.tobytes(), "%s after %d samples is not the plain run's" % (key, ns * (k + 1))
    print("%s converging, %s lights: %d passes; max |delta| mean %.3e, sum / n %.3e, Y / n %.3e, Q / n %.3e (nearest decision %.3g x its margin)"
          % (VM.cell_id(cell), "offset" if offsets else "stored", len(recs), worst[0], worst[1], worst[2], worst[3], nearest))


# ---------------------------------------------------------------- the diffuse bounce
@cells
def test_bounce(pkg, ctx, matrix, B, cell):
    """rm_accumulate_bounce_device through the lens, under the area lights, rows from BOUNCE_FIRST on, strength 1."""
    bvh, generic, depth = cell
    name = load(ctx, matrix, B, cell)
    first, n = VM.BOUNCE_FIRST, VM.BOUNCE_ROWS
    table, offsets, bounce = ctx.lens_sequence(first, n), ctx.light_sequence(first, n, VM.RADII), pkg.backend.bounce_sequence(first, n)
    assert bounce.tobytes() == BR.bounce_sequence(first, n).tobytes() and offsets.tobytes() == SR.light_sequence(first, n, VM.RADII).tobytes()
    assert np.asarray(table).tobytes() == PR.lens_sequence(first, n).tobytes()     # the rows tests/test_variant_matrix.py pins
    total, mean, rgb8 = GB.run_bounce(pkg, ctx, W, H, depth, VM.APERTURE, VM.FOCUS, table, offsets, bounce, 1., (5, 5))
    ref_sum, ref_mean = B.bounce(name, W, H, depth, VM.APERTURE, VM.FOCUS, table, offsets, bounce, 1., (5, 5))
    d_mean, d_sum = held(mean, ref_mean, "mean"), held(total, ref_sum, "sum", n * TIGHT)
    assert rgb8.tobytes() == PR.to_bytes(mean).tobytes()
    one = GB.run_bounce(pkg, ctx, W, H, depth, VM.APERTURE, VM.FOCUS, table, offsets, bounce, 1., (n,))
    for a, b, what in zip((total, mean, rgb8), one, ("sum", "mean", "bytes")):
        assert a.tobytes() == b.tobytes(), "%s after two passes of 5 is not the one pass of 10's" % what
    soft = B.soft(name, W, H, depth, VM.APERTURE, VM.FOCUS, table, offsets, (5, 5))[1]
    assert int((np.abs(ref_mean - soft) > 0.05).any(axis=2).sum()) > 50      # light did come back
    # strength 0: the area lights' frame
    still = GB.run_bounce(pkg, ctx, W, H, depth, VM.APERTURE, VM.FOCUS, table, offsets, bounce, 0., (5, 5))
    plain = GS.run_soft(pkg, ctx, W, H, depth, VM.APERTURE, VM.FOCUS, table, offsets, (5, 5))
    for a, b, what in zip(still, plain, ("sum", "mean", "bytes")):
        assert a.tobytes() == b.tobytes(), "%s with strength 0 is not the soft frame's" % what
    print("%s bounce: max |delta| mean %.3e, sum %.3e" % (VM.cell_id(cell), d_mean, d_sum))


@pytest.mark.parametrize("offsets", [False, True], ids=["stored", "offsets"])
@cells
def test_converging_bounce(pkg, ctx, matrix, B, cell, offsets):
    """rm_accumulate_converging_bounce_device with stored and with offset lights against the plain bounce run of the same cell
    (which test_bounce holds to the oracle): tolerance < 0 byte for byte, and a real tolerance pixel by pixel at its own count."""
    bvh, generic, depth = cell
    ns, tol, lo, hi = VM.CONVERGE
    radii = VM.RADII if offsets else None
    name = load(ctx, matrix, B, cell)
    tables = GCB.bounce_tables(pkg, ctx, hi, radii)
    plain = GCB.plain_bounce_snapshots(pkg, ctx, B, name, depth, VM.APERTURE, VM.FOCUS, ns, hi // ns, radii, 1.)
    f = GC.Frame(pkg, H, W)
    for k in range(2):
        GCB.bounce_pass(pkg, ctx, f, depth, VM.APERTURE, VM.FOCUS, ns, -1., lo, hi, tables, 1., k == 0)
        got = f.snapshot()
        assert got["listed"] == W * H and np.all(got["count"] == ns * (k + 1))
        for key, ref in zip(("sum", "mean", "rgb8"), plain[ns * (k + 1)]):
            assert not (key != "rgb8" and np.isnan(got[key]).any())
            assert got[key].tobytes() == ref.tobytes(), "%s after %d samples is not the plain bounce run's" % (key, ns * (k + 1))
    assert int((np.abs(got["mean"] - GC.plain_snapshots(pkg, ctx, depth, VM.APERTURE, VM.FOCUS, ns, 2, radii)[2 * ns][1]) > 0.05).any(axis=2).sum()) > 20
    # a real tolerance: every pixel is the plain bounce run at its own count
    g = GC.Frame(pkg, H, W)
    for k in range(8 * (hi // ns + 2)):                                # (converge_reference.run's stop: a pixel listed late, as a neighbour, outlasts hi / ns passes)
        GCB.bounce_pass(pkg, ctx, g, depth, VM.APERTURE, VM.FOCUS, ns, tol, lo, hi, tables, 1., k == 0)
        last = g.snapshot()
        if last["listed"] == 0:
            break
    counts = last["count"]
    assert last["listed"] == 0 and len(np.unique(counts)) >= 3 and counts.max() <= hi and counts.min() >= lo
    for c in np.unique(counts):
        at = counts == c
        for key, ref in zip(("sum", "mean", "rgb8"), plain[int(c)]):
            assert last[key][at].tobytes() == ref[at].tobytes(), "%s of the pixels with %d samples" % (key, c)
    print("%s converging bounce, %s lights: %d distinct counts, %d .. %d; every pixel is the plain bounce run at its own count"
          % (VM.cell_id(cell), "offset" if offsets else "stored", len(np.unique(counts)), counts.min(), counts.max()))


# ---------------------------------------------------------------- random scenes
@pytest.mark.parametrize("seed", range(int(os.environ.get("RM_MATRIX_FUZZ_SEEDS", "6"))))   # RM_MATRIX_FUZZ_SEEDS=300: a longer hunt
def test_fuzz_random_scenes(pkg, O, ctx, orc, seed):
    """The render fuzz's seeded scenes (tests/test_gpu_parity.py: spheres, polygons, a mesh, 1-3 lights, every third with an
    exponent of 12.5, every other with a hierarchy, depth caps 1..6) through the radiance rays and a lens frame whose aperture
    and focus come from the scene's bounds."""
    scene, oscene, cam, _, _, depth = GPAR._fuzz_scene(pkg, O, seed)
    GL.upload(ctx, scene)
    desc = scene.flatten().desc()
    o, d = RR.rays_for("fuzz", desc, np.random.default_rng(20261400 + seed), VM.N_RAYS)
    got = ctx.radiance(o, d, max_depth=depth)
    ref = orc.cast(oscene, o, d, depth)
    d_rays = GL.worst(got, ref)
    gone = ~(ref != 0.).any(axis=1)
    assert not np.isnan(got).any() and d_rays < TIGHT and not got[gone].view(np.uint64).any()
    lo, hi = GQ.bounds_of(desc)
    focus, aperture = float(np.linalg.norm((lo + hi) / 2. - np.array(cam))), 0.01 * float(np.linalg.norm(hi - lo))
    table = ctx.lens_table(VM.LENS_SAMPLES)
    frame = GL.lens_frame(pkg, ctx, W, H, depth, aperture, focus, table, fill=NAN)
    ref_frame = LR.frame(orc, oscene, cam, None, W, H, depth, aperture, focus, table)
    d_lens = GL.worst(frame, ref_frame)
    print("fuzz %d (depth %d, %d primitives): max |delta| rays %.3e (%d lit), lens %.3e (%d lit)" % (
        seed, depth, desc.n_spheres + desc.n_polygons + desc.n_triangles, d_rays, int((~gone).sum()), d_lens, int((ref_frame != 0.).any(axis=2).sum())))
    assert not np.isnan(frame).any() and d_lens < TIGHT
