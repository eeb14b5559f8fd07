"""Converging frames with a moving camera on the GPU (-m gpu): rm_accumulate_converging_camera_device and
rm_render_converging_camera through the C ABI and the Python bindings, against the frames of rm_accumulate_camera_device,
rm_accumulate_converging_device and rm_accumulate_converging_moving_device and against tests/camera_motion_reference.py's samples
under converge_reference's select and fold.

What the header calls byte for byte is demanded byte for byte.  Against the yardstick the bounds are tests/test_gpu_converge.py's:
masks, lists (as sets) and counts exactly, every channel of the mean within TIGHT = 1e-9, of the sum within n TIGHT, Y within
3 n TIGHT and Q within 6 n (ymax + 1.5 TIGHT) TIGHT, no pixel left out; converge_reference.run asserts that no free decision of
a case lies within the margin of its bound.  Frames are 32 x 32, caps of 32 and 40 rows."""
import numpy as np
import pytest

import camera_motion_reference as CM
import converge_reference as CR
import lens_reference as LR
import moving_reference as MV
import progressive_reference as PR
import radiance_reference as RR
import soft_reference as SR
import test_gpu_camera_motion as GK
import test_gpu_converge as GC
import test_gpu_converge_moving as GCM
import test_gpu_lens as GL
import test_gpu_progressive as GP
import workloads

pytestmark = pytest.mark.gpu

TIGHT = CR.TIGHT
NAN, BYTE = GP.NAN, GP.BYTE
Frame, compare, on_device = GC.Frame, GC.compare, GCM.on_device
KEYS = ("sum", "stats", "count", "mean", "rgb8", "mask", "list")
# case of camera_motion_reference.MOTIONS -> (radii or None, aperture, shapes move as well, n_samples, tolerance, min, max samples)
CASES = {"demo-both": ((1.5, 3.), LR.APERTURE, False, 8, 0.1, 8, 32), "cornell": (None, 0., False, 8, 0.1, 8, 32),
         "synthetic256": (None, LR.APERTURE, False, 8, 0.1, 8, 32), "pool": (SR.PENUMBRA_RADII, LR.APERTURE, True, 5, 0.1, 10, 40)}


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_converge_camera"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return CM.Yardstick(pkg, O, orc)


def camera_pass(pkg, c, f, depth, aperture, focus, ns, tol, lo, hi, tables, fresh, outputs=True):
    p = pkg.backend.make_params(workloads.FOV, float(f.h), float(f.w), depth)
    table, camera, lights, shapes = tables
    c.accumulate_converging_camera_device(p, f.sum, f.stats, f.count, aperture, focus, ns, table, camera, lights, shapes, tol, lo, hi, fresh,
                                          mean=f.mean if outputs else None, rgb8=f.rgb8 if outputs else None, mask=f.mask if outputs else None,
                                          workspace=f.ws[:f.ws_words])


def run_passes(pkg, c, depth, aperture, focus, ns, tol, lo, hi, tables, passes=None):
    f, out, k = Frame(pkg, 32, 32), [], 0
    while passes is None or k < passes:
        camera_pass(pkg, c, f, depth, aperture, focus, ns, tol, lo, hi, tables, k == 0)
        k += 1
        out.append(f.snapshot())
        if passes is None and out[-1]["listed"] == 0:
            break
        assert k <= 8 * (hi // ns + 2)
    return out


def case_tables(ctx, Y, case, random=None):
    """The four tables of a case, max_samples rows, as numpy (shapes None where no shape moves): the library's, or with `random`
    a generator tables that are not -- another camera and other offsets for every row."""
    name, depth, velocity, turn = CM.MOTIONS[case]
    radii, aperture, moving, ns, tol, lo, hi = CASES[case]
    if random is None:
        assert (GK.CASES[case][0], GK.CASES[case][2]) == (radii, moving)
        return GK.library_tables(ctx, Y, case, 0, hi)
    shapes = MV.random_offsets(random, hi, Y.kinds(name), MV.SPEED[name] / 3.) if moving else None
    return PR.lens_sequence(0, hi), CM.random_rows(random, hi, MV.SPEED[name] / 6.), SR.random_offsets(random, hi, Y.n_lights(name)), shapes


def device(tables):
    return tuple(None if t is None else on_device(t)[0] for t in tables)


def plain_snapshots(pkg, c, depth, aperture, focus, ns, n_passes, tables):
    """rm_accumulate_camera_device over consecutive slices of the four tables in passes of ns: count -> (sum, mean, bytes)."""
    table, camera, lights, shapes = tables
    out = {}
    for k in range(1, n_passes + 1):
        out[k * ns] = GK.run_camera(pkg, c, 32, 32, depth, aperture, focus, table[:k * ns], camera[:k * ns], lights[:k * ns],
                                    None if shapes is None else shapes[:k * ns], (ns,) * k)
    return out


# ---------------------------------------------------------------- 1. parity with the yardstick, pass by pass
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("tables_are", ["the library's", "random"])
def test_converging_camera_frames_match_the_yardstick_pass_by_pass(pkg, ctx, Y, case, tables_are):
    name, depth, velocity, turn = CM.MOTIONS[case]
    radii, aperture, moving, ns, tol, lo, hi = CASES[case]
    GL.upload(ctx, Y.scene(name)[0])
    tables = case_tables(ctx, Y, case, None if tables_are == "the library's" else np.random.default_rng(20261021))
    s = Y.camera_samples(name, 32, 32, depth, aperture, LR.FOCUS, *tables)
    ymax = float(np.abs(CR.y_of(s)).max())
    recs, nearest = CR.run(s, 32, 32, ns, tol, lo, hi)
    got = run_passes(pkg, ctx, depth, aperture, LR.FOCUS, ns, tol, lo, hi, device(tables))
    assert len(got) == len(recs)
    worst = np.zeros(4)
    for k, (g, (listed, st)) in enumerate(zip(got, recs)):
        assert g["listed"] == int(listed.sum())
        worst = np.maximum(worst, compare(case, k, g, listed, st, ymax))
    print("%s, %s tables: %d passes, %d samples cast; max |delta| mean %.3e, sum / n %.3e, Y / n %.3e, Q / n %.3e (nearest decision %.3g x its margin)"
          % (case, tables_are, len(got), sum(g["listed"] for g in got) * ns, worst[0], worst[1], worst[2], worst[3], nearest))
    assert len(np.unique(got[-1]["count"])) >= 2 and any(0 < g["listed"] < 1024 for g in got)


# ---------------------------------------------------------------- 2. standing rows are the underlying passes
@pytest.mark.parametrize("name,depth", [("demo", 3), ("synthetic256", 6)])
def test_standing_rows_are_the_underlying_passes_byte_for_byte(pkg, ctx, Y, name, depth):
    """An oriented context, every row its basis and an offset of zero (+0. in the first half of the table, -0. in the second),
    seven passes of 5 samples under a cap of 40: rm_accumulate_converging_device's bytes without a shape table (the hierarchy
    cell on the 256 spheres), rm_accumulate_converging_moving_device's with one."""
    scene = Y.scene(name)[0]
    GL.upload(ctx, scene)
    try:
        eye, basis, focus = GK.side_view(ctx, scene)
        ns, tol, lo, hi = 5, 0.1, 10, 40
        camera = CM.standing_rows(hi, basis)
        camera[hi // 2:, :3] = -0.
        lights = SR.light_sequence(0, hi, (1.5,) * Y.n_lights(name))
        shapes = ctx.motion_sequence(0, hi, MV.velocities(Y.kinds(name), MV.SPEED[name]), CM.SHUTTER)
        for g in (None, shapes):
            table, cam, lo_t, sh = device((PR.lens_sequence(0, hi), camera, lights, g))
            a, b = Frame(pkg, 32, 32), Frame(pkg, 32, 32)
            partial = 0
            for k in range(7):
                if g is None:
                    GC.converge_pass(pkg, ctx, a, depth, LR.APERTURE, focus, ns, tol, lo, hi, (table, lo_t), k == 0)
                else:
                    GCM.moving_pass(pkg, ctx, a, depth, LR.APERTURE, focus, ns, tol, lo, hi, (table, lo_t, sh), k == 0)
                camera_pass(pkg, ctx, b, depth, LR.APERTURE, focus, ns, tol, lo, hi, (table, cam, lo_t, sh), k == 0)
                under, got = a.snapshot(), b.snapshot()
                partial += 0 < under["listed"] < 1024
                for key in KEYS:
                    assert not (key in ("sum", "stats", "mean") and np.isnan(got[key]).any())
                    assert got[key].tobytes() == under[key].tobytes(), "%s, %s, pass %d: %s" % (name, "static" if g is None else "moving", k, key)
            assert partial >= 1 and len(np.unique(under["count"])) >= 2
    finally:
        ctx.orient(None)


# ---------------------------------------------------------------- 3. own count, a negative tolerance, unlisted pixels
@pytest.mark.parametrize("case", ["demo-both", "pool"])
def test_every_pixel_holds_the_plain_camera_run_at_its_own_count(pkg, ctx, Y, case):
    name, depth, velocity, turn = CM.MOTIONS[case]
    radii, aperture, moving, ns, tol, lo, hi = CASES[case]
    GL.upload(ctx, Y.scene(name)[0])
    tables = case_tables(ctx, Y, case)
    last = run_passes(pkg, ctx, depth, aperture, LR.FOCUS, ns, tol, lo, hi, device(tables))[-1]
    counts = last["count"]
    assert last["listed"] == 0 and len(np.unique(counts)) >= 2 and counts.max() <= hi and counts.min() >= lo
    plain = plain_snapshots(pkg, ctx, depth, aperture, LR.FOCUS, ns, int(counts.max()) // ns, tables)
    for c in np.unique(counts):
        at = counts == c
        for key, ref in zip(("sum", "mean", "rgb8"), plain[int(c)]):
            assert last[key][at].tobytes() == ref[at].tobytes(), "%s: %s of the pixels with %d samples" % (case, key, c)


@pytest.mark.parametrize("moving", [False, True])
def test_a_negative_tolerance_is_the_plain_run_and_unlisted_pixels_keep_every_byte(pkg, ctx, Y, moving):
    """A fresh pass and two continued ones of 5 samples under a cap of 16 on the pool scene with tables that are not the library's;
    the fourth pass finds every pixel capped, lists nothing and touches nothing -- NaN planted in every buffer stays."""
    GL.upload(ctx, Y.scene("pool")[0])
    rng = np.random.default_rng(20261022)
    tables = (PR.lens_sequence(0, 16), CM.random_rows(rng, 16, MV.SPEED["pool"] / 6.), SR.random_offsets(rng, 16, Y.n_lights("pool")),
              MV.random_offsets(rng, 16, Y.kinds("pool"), MV.SPEED["pool"] / 3.) if moving else None)
    plain = plain_snapshots(pkg, ctx, 3, LR.APERTURE, LR.FOCUS, 5, 3, tables)
    dev = device(tables)
    f = Frame(pkg, 32, 32)
    for k in range(3):
        camera_pass(pkg, ctx, f, 3, LR.APERTURE, LR.FOCUS, 5, -1., 16, 16, dev, k == 0)
        got = f.snapshot()
        assert got["listed"] == 1024 and (got["count"] == 5 * (k + 1)).all()
        for key, ref in zip(("sum", "mean", "rgb8"), plain[5 * (k + 1)]):
            assert got[key].tobytes() == ref.tobytes(), "pass %d: %s" % (k, key)
    before = f.snapshot()
    camera_pass(pkg, ctx, f, 3, LR.APERTURE, LR.FOCUS, 5, -1., 16, 16, dev, False)       # 15 + 5 > 16: capped
    after = f.snapshot()
    assert after["listed"] == 0 and not after["mask"].any()
    for key in ("sum", "stats", "count", "mean", "rgb8"):
        assert after[key].tobytes() == before[key].tobytes(), key
    # ... and a pass that lists some pixels leaves the others alone: settle everything but what the widened rule keeps
    g = Frame(pkg, 32, 32)
    camera_pass(pkg, ctx, g, 3, LR.APERTURE, LR.FOCUS, 5, 0.1, 5, 16, dev, True)
    first = g.snapshot()
    camera_pass(pkg, ctx, g, 3, LR.APERTURE, LR.FOCUS, 5, 0.1, 5, 16, dev, False)
    second = g.snapshot()
    off = ~second["mask"].astype(bool)
    assert 0 < second["listed"] < 1024
    for key in ("sum", "stats", "count", "mean", "rgb8"):
        assert second[key][off].tobytes() == first[key][off].tobytes(), key


# ---------------------------------------------------------------- 4. the tick
def test_the_tick_is_the_device_call_finishes_begins_again_and_refuses(pkg, ctx, Y):
    import ctypes as C
    L, B = pkg.lib(), pkg._lib
    scene = Y.scene("demo")[0]
    GL.upload(ctx, scene)
    kinds = Y.kinds("demo")
    v = MV.velocities(kinds, MV.SPEED["demo"])
    radii, vel, turn = (1.5, 3.), (4., 0., -2.), (0.2, 0.1, 0.)
    ns, tol, lo, hi = 8, 0.1, 8, 32
    p = pkg.backend.make_params(workloads.FOV, 32., 32., 3)

    def tick(velocity=vel, t=turn, shutter=CM.SHUTTER, vs=None, restart=False, tolerance=tol, **kw):
        return ctx.render_converging_camera(p, velocity, shutter, LR.APERTURE, LR.FOCUS, ns, tolerance, lo, hi, t, vs, radii, restart, **kw)[1]

    def moving(restart=False):
        return ctx.render_converging_moving(p, v, CM.SHUTTER, LR.APERTURE, LR.FOCUS, ns, tol, lo, hi, radii, restart)[1]

    for vs in (None, v):
        tables = (ctx.lens_sequence(0, hi), ctx.camera_sequence(0, hi, vel, CM.SHUTTER, turn), ctx.light_sequence(0, hi, radii),
                  None if vs is None else ctx.motion_sequence(0, hi, v, CM.SHUTTER))
        want = run_passes(pkg, ctx, 3, LR.APERTURE, LR.FOCUS, ns, tol, lo, hi, device(tables))
        host, host8 = np.full((32, 32, 3), -3.5), np.full((32, 32, 3), 7, np.uint8)
        cast = 0
        for k, w in enumerate(want):
            rep = tick(vs=vs, restart=k == 0, host_rgb=host, host_rgb8=host8)
            cast += w["listed"] * ns
            assert (rep.listed, rep.passes, rep.samples_cast) == (w["listed"], k + 1, cast)
            assert host.tobytes() == w["mean"].tobytes() and host8.tobytes() == w["rgb8"].tobytes()
        # a finished frame launches nothing
        timing, rep = ctx.render_converging_camera(p, vel, CM.SHUTTER, LR.APERTURE, LR.FOCUS, ns, tol, lo, hi, turn, vs, radii, host_rgb=host)
        assert rep.listed == 0 and rep.passes == len(want) and timing.kernel_ms == 0. and host.tobytes() == want[-1]["mean"].tobytes()
    # what begins the frame again
    assert tick(restart=True).passes == 1 and tick().passes == 2
    assert tick(velocity=(4., 0., -2.5)).passes == 1 and tick(velocity=(4., 0., -2.5)).passes == 2
    assert tick(t=(0.2, 0.1, 0.01)).passes == 1
    assert tick(shutter=0.5).passes == 1 and tick(shutter=0.5).passes == 2
    assert tick().passes == 1 and tick(tolerance=0.05).passes == 2                          # the rule stays outside the key
    assert tick(vs=v).passes == 1
    assert moving().passes == 1 and moving().passes == 2                                    # camera -> moving shapes
    assert tick(vs=v).passes == 1 and tick(vs=v).passes == 2                                # ... and back
    assert tick(velocity=(0., 0., 0.), t=(0., 0., 0.), vs=v).passes == 1                    # a motion of zero is a motion
    assert moving().passes == 1
    assert ctx.render_converging(p, LR.APERTURE, LR.FOCUS, ns, tol, lo, hi, radii)[1].passes == 1
    assert tick().passes == 1 and tick().passes == 2
    # rows == 0: RM_OK and a report of zeros; the frame stands
    short = pkg.backend.make_params(workloads.FOV, 31., 32., 3)
    rep = ctx.render_converging_camera(short, vel, CM.SHUTTER, LR.APERTURE, LR.FOCUS, ns, tol, lo, hi, turn, None, radii)[1]
    assert (rep.listed, rep.passes, rep.max_count, rep.samples_cast) == (0, 0, 0, 0)
    assert tick().passes == 3
    # refusals change nothing of the state
    lens, conv = B.rm_lens(LR.APERTURE, LR.FOCUS, ns, 0), B.rm_converge(tol, lo, hi)
    r64 = np.ascontiguousarray(radii)
    nan = float("nan")

    def raw(motion, shutter=CM.SHUTTER, c=conv):
        m = B.rm_camera_motion(B.vec3(motion[:3]), *motion[3:]) if motion is not None else None
        rep = B.rm_converge_report(5, 6, 7, 8, 0)
        st = L.rm_render_converging_camera(ctx.ptr, C.byref(p), C.byref(lens), C.byref(c), r64.ctypes.data_as(C.POINTER(C.c_double)), 2, None, 0,
                                           shutter, C.byref(m) if m is not None else None, 0, None, None, C.byref(rep), None)
        assert (rep.samples_cast, rep.listed, rep.passes) == (5, 6, 7)
        return st, L.rm_last_error(ctx.ptr)

    good = vel + turn
    for args, text in (((None,), b"NULL motion"), (((nan, 0., 0., 0., 0., 0.),), b"not finite"), ((good, -1.), b"shutter"),
                       ((good, CM.SHUTTER, B.rm_converge(nan, lo, hi)), b"tolerance"), ((good, CM.SHUTTER, B.rm_converge(tol, lo, 4)), b"max_samples")):
        st, err = raw(*args)
        assert st != 0 and text in err and b"rm_render_converging_camera" in err, err
    assert tick().passes == 4


def test_the_converged_one_shot(pkg, ctx, Y, capsys):
    scene = Y.scene("demo")[0]
    r, fb = pkg.create_renderer(workloads.FOV, 32., 32.), pkg.create_frame_buffer(32, 32)
    rep = r.render_converged_camera(fb, scene, (4., 0., -2.), CM.SHUTTER, 0.1, 8, (0.2, 0.1, 0.), min_samples=8, max_samples=32)
    assert rep.listed == 0 and rep.passes >= 2 and 8 <= rep.max_count <= 32 and r.last_report is rep
    c = pkg.backend.default_context(0)
    tables = (c.lens_sequence(0, 32), c.camera_sequence(0, 32, (4., 0., -2.), CM.SHUTTER, (0.2, 0.1, 0.)), np.zeros((32, Y.n_lights("demo"), 3)), None)
    want = run_passes(pkg, c, 3, 0., 1., 8, 0.1, 8, 32, device(tables))
    assert len(want) == rep.passes and np.asarray(fb.buffer).reshape(32, 32, 3).tobytes() == want[-1]["mean"].tobytes()
    capsys.readouterr()
