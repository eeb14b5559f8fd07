"""History in the converging tick on the GPU (-m gpu): rm_converge_history, rm_converge_history_info and what rm_render_converging
does with them, through the Python binding.

The tick's buffers are handed out by no call.  But the converging tick is, byte for byte, the device call over the library's
own sequences (tests/test_gpu_converge.py holds it to that), and rm_reproject_device is held to the yardstick by
tests/test_gpu_reproject.py; so a reprojected tick is rebuilt here by hand -- the previous frame with
rm_accumulate_converging_device, primary hits at both views, rm_reproject_device, one more pass with fresh = 0 -- and the tick
must write those bytes."""
import numpy as np
import pytest

import test_gpu_reproject as GR
import workloads

pytestmark = pytest.mark.gpu

NAN, BYTE = float("nan"), 0xA5
H, W, ROWS = 72, 64, 64                                                # 72 % 32 = 8 rows the tick leaves alone
NS, TOL, LO, HI, RADIUS = GR.NS, GR.TOL, GR.LO, GR.HI, GR.RADIUS
SETTINGS = dict(sigma_z=.1, min_normal_dot=.9, max_history=32)
STEP = (.25, 0., 0.)


class Demo:
    def __init__(self, pkg):
        self.pkg = pkg
        self.c = pkg.backend.Context(0)
        self.scene = workloads.product_scene(pkg, "demo")
        self.radii = (RADIUS,) * len(self.scene.lights)
        self.c.upload(self.scene.flatten())
        self.c.orient(None)
        pos = self.c.camera()[0]
        self.base = (pos.x, pos.y, pos.z)

    def at(self, step=(0., 0., 0.), yaw=0.):
        GR.move(self.pkg, self.c, self.base, step, yaw)

    def tick(self, p, restart=False, tol=TOL, lo=LO, hi=HI, ns=NS, radii=None, aperture=0., host_rgb=None, host_rgb8=None):
        return self.c.render_converging(p, aperture, 5., ns, tol, lo, hi, radii=self.radii if radii is None else radii, restart=restart,
                                        host_rgb=host_rgb, host_rgb8=host_rgb8)[1]


@pytest.fixture()
def demo(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    d = Demo(pkg)
    yield d
    d.c.close()


def params(pkg, h=H, w=W):
    return GR.params(pkg, h, w)


def report_of(rep):
    return (rep.samples_cast, rep.listed, rep.passes, rep.max_count)


def test_a_camera_move_with_history_is_the_composition_by_hand(pkg, demo):
    import torch
    c, p = demo.c, params(pkg)
    assert c.history_info() == {"reprojections": 0, "last_reprojected": 0, "carried": 0, "without": 0}
    c.converge_history(SETTINGS)
    demo.at()
    for k in range(3):
        demo.tick(p, restart=(k == 0))
    assert c.history_info()["last_reprojected"] == 0 and c.history_info()["reprojections"] == 0
    demo.at(STEP)
    host, host8 = np.full((H, W, 3), NAN), np.full((H, W, 3), BYTE, np.uint8)
    timing, rep = c.render_converging(p, 0., 5., NS, TOL, LO, HI, radii=demo.radii, host_rgb=host, host_rgb8=host8)
    info = c.history_info()
    assert info["last_reprojected"] == 1 and info["reprojections"] == 1
    assert info["carried"] > 0 and info["carried"] + info["without"] == ROWS * W
    assert timing.kernel_ms > 0. and np.isnan(host[ROWS:]).all() and (host8[ROWS:] == BYTE).all()
    # by hand: the previous frame, the hits of both views, the reprojection, one pass that continues
    demo.at()
    view = c.camera()
    total, stats, count, _ = GR.converging_frame(c, p, len(demo.radii))
    prev_hits = c.primary_hits_device(p)
    demo.at(STEP)
    cur_hits = c.primary_hits_device(p)
    dev = "cuda:0"
    total2, stats2 = torch.full((H, W, 3), NAN, dtype=torch.float64, device=dev), torch.full((H, W, 2), NAN, dtype=torch.float64, device=dev)
    count2, carried = torch.full((H, W), 7, dtype=torch.int32, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev)
    c.reproject_device(p, total, stats, count, prev_hits, cur_hits, view, total2, stats2, count2, carried_total=carried, **SETTINGS)
    table = torch.from_numpy(c.lens_sequence(0, HI)).to(dev)
    offsets = torch.from_numpy(c.light_sequence(0, HI, demo.radii)).to(dev)
    ws = c.accumulate_converging_device(p, total2, stats2, count2, 0., 5., NS, table, TOL, LO, HI, False, offsets=offsets)
    torch.cuda.synchronize()
    assert info["carried"] == int(carried.cpu()[0])
    listed = int(ws.cpu()[0])
    assert 0 < listed < ROWS * W                                         # carried pixels that are settled are not sampled again
    assert report_of(rep) == (listed * NS, listed, 1, 32)                # N = min(24, 32) + 8
    S, n = total2.cpu().numpy()[:ROWS], count2.cpu().numpy()[:ROWS]
    assert n.min() >= 8                                                  # every pixel holds samples: carried, sampled or both
    want = S / n.astype(np.float64)[..., None]                           # the mean of every pixel, sampled by the pass or not
    assert host[:ROWS].tobytes() == want.tobytes()
    with np.errstate(invalid="ignore"):
        assert host8[:ROWS].tobytes() == (255. * np.minimum(np.maximum(want, 0.), 1.)).astype(np.uint8).tobytes()
    # the next tick continues the reprojected frame, and is no reprojection itself
    rep2 = demo.tick(p, host_rgb=host)
    c.accumulate_converging_device(p, total2, stats2, count2, 0., 5., NS, table, TOL, LO, HI, False, offsets=offsets, workspace=ws)
    torch.cuda.synchronize()
    assert rep2.passes == 2 and rep2.listed == int(ws.cpu()[0])
    S, n = total2.cpu().numpy()[:ROWS], count2.cpu().numpy()[:ROWS]
    assert host[:ROWS].tobytes() == (S / n.astype(np.float64)[..., None]).tobytes()
    info = c.history_info()
    assert info["last_reprojected"] == 0 and info["reprojections"] == 1 and info["carried"] + info["without"] == ROWS * W


def test_without_history_the_ticks_are_what_they_were(pkg, demo):
    c, p = demo.c, params(pkg)

    def two_views(restart_second):
        demo.at()
        for k in range(3):
            demo.tick(p, restart=(k == 0))
        demo.at(STEP)
        mean, rgb8 = np.full((H, W, 3), NAN), np.full((H, W, 3), BYTE, np.uint8)
        rep = demo.tick(p, restart=restart_second, host_rgb=mean, host_rgb8=rgb8)
        return mean.tobytes(), rgb8.tobytes(), report_of(rep)

    moved, restarted = two_views(False), two_views(True)
    assert moved == restarted and moved[2] == (ROWS * W * NS, ROWS * W, 1, NS)
    assert c.history_info() == {"reprojections": 0, "last_reprojected": 0, "carried": 0, "without": 0}
    # ... and after history was on and is off again
    c.converge_history(SETTINGS)
    assert two_views(False) != restarted and c.history_info()["reprojections"] == 1
    c.converge_history(None)
    assert two_views(False) == restarted
    info = c.history_info()
    assert info["reprojections"] == 1 and info["last_reprojected"] == 0
    c.converge_history(None)                                             # off twice is off


def test_everything_else_still_begins_the_frame_again(pkg, demo):
    c, p = demo.c, params(pkg)
    c.converge_history(SETTINGS)
    every = ROWS * W

    def settle():
        demo.at()
        for k in range(3):
            rep = demo.tick(p, restart=(k == 0))
        assert rep.passes == 3
        return c.history_info()["reprojections"]

    # a changed tolerance continues the frame
    before = settle()
    rep = demo.tick(p, tol=TOL / 2.)
    assert rep.passes == 4 and c.history_info() == dict(c.history_info(), reprojections=before, last_reprojected=0)
    # each of these, together with a camera move, begins it again: every pixel is listed, and nothing counts as a reprojection
    begun = []
    before = settle()
    demo.at(STEP)
    begun.append(("radius", demo.tick(p, radii=(RADIUS * 2.,) * len(demo.radii))))
    before_lens = settle()
    demo.at(STEP)
    begun.append(("lens", demo.tick(p, aperture=.05)))
    settle()
    demo.at(STEP)
    begun.append(("restart", demo.tick(p, restart=True)))
    settle()
    demo.at(STEP)
    zero = np.zeros((len(demo.scene.shapes), 3))
    begun.append(("motion", c.render_converging_motion(p, zero, 0., 0., 5., NS, TOL, LO, HI, radii=demo.radii)[1]))
    settle()
    c.upload(workloads.product_scene(pkg, "cornell").flatten())
    c.upload(demo.scene.flatten())                                       # the same scene, uploaded again: another copy on the device
    demo.at(STEP)
    begun.append(("scene", demo.tick(p)))
    for name, rep in begun:
        assert (rep.passes, rep.listed, rep.max_count) == (1, every, NS), name
    info = c.history_info()
    assert info["reprojections"] == before == before_lens == 0 and info["last_reprojected"] == 0
    # ... while the move alone does not
    settle()
    demo.at(STEP)
    rep = demo.tick(p)
    assert rep.passes == 1 and rep.listed < every and c.history_info()["reprojections"] == 1
    # a yaw turns the oriented state on: still only the view
    demo.at(STEP, yaw=.05)
    rep = demo.tick(p)
    assert rep.passes == 1 and rep.listed < every and c.history_info()["reprojections"] == 2 and c.history_info()["last_reprojected"] == 1
    # a refused call changes nothing of the state
    demo.at()
    with pytest.raises(pkg._lib.BackendError, match="frame width is not a multiple of 32"):
        c.render_converging(params(pkg, H, 48), 0., 5., NS, TOL, LO, HI, radii=demo.radii)
    demo.at(STEP, yaw=.05)
    assert c.history_info()["reprojections"] == 2 and c.history_info()["last_reprojected"] == 1
    assert demo.tick(p).passes == 2


def test_the_filter_after_a_reprojected_tick_filters_that_frame(pkg, demo):
    c, p = demo.c, params(pkg)
    c.converge_history(SETTINGS)

    def run(filtered):
        out = []
        demo.at()
        for k in range(3):
            demo.tick(p, restart=(k == 0))
        demo.at(STEP)
        for k in range(3):
            mean, rgb8 = np.full((H, W, 3), NAN), np.full((H, W, 3), BYTE, np.uint8)
            rep = demo.tick(p, host_rgb=mean, host_rgb8=rgb8)
            out.append((mean.tobytes(), rgb8.tobytes(), report_of(rep)))
            if filtered:
                plain = np.full((H, W, 3), NAN)
                c.render_denoised(p, iterations=0, host_rgb=plain)
                assert plain.tobytes() == mean.tobytes()                 # no iterations: the reprojected frame's own mean
                smooth = np.full((H, W, 3), NAN)
                c.render_denoised(p, iterations=3, guides=(k % 2 == 0), host_rgb=smooth)
                assert np.isfinite(smooth[:ROWS]).all() and smooth.tobytes() != mean.tobytes()
        return out

    before = c.history_info()["reprojections"]
    plain, filtered = run(False), run(True)
    assert plain == filtered and plain[0][2][2] == 1 and plain[2][2][2] == 3
    assert c.history_info()["reprojections"] == before + 2


def test_history_turned_on_in_the_middle_of_a_frame(pkg, demo):
    c, p = demo.c, params(pkg)
    demo.at()
    for k in range(2):
        demo.tick(p, restart=(k == 0))
    c.converge_history(SETTINGS)
    # moved at once: the kept frame has no hit buffer, so this frame begins again -- and keeps one
    demo.at(STEP)
    rep = demo.tick(p)
    assert rep.passes == 1 and rep.listed == ROWS * W and c.history_info()["last_reprojected"] == 0
    demo.at((2. * STEP[0], 0., 0.))
    rep = demo.tick(p)
    assert rep.passes == 1 and rep.listed < ROWS * W
    assert c.history_info()["last_reprojected"] == 1 and c.history_info()["reprojections"] == 1
    # ... and with a tick between turning it on and the move, the first move is carried: that tick found the frame without a hit
    # buffer and filled it.  A finished frame's tick launches no pass, but fills it all the same
    c.converge_history(None)
    for finish in (False, True):
        demo.at()
        rep = demo.tick(p, restart=True)
        while finish and rep.listed > 0:
            rep = demo.tick(p)
        passes = rep.passes
        c.converge_history(SETTINGS)
        again = demo.tick(p)
        assert again.passes == (passes if finish else passes + 1)
        demo.at(STEP)
        before = c.history_info()["reprojections"]
        assert demo.tick(p).passes == 1 and c.history_info()["reprojections"] == before + 1, finish
        c.converge_history(None)


def test_history_gains_what_a_restart_loses(pkg, demo):
    """The demo at 64 x 64, area lights of radius 1.5, a pinhole; the view settled to 64 samples a pixel, then a sideways step of
    0.25.  Against the plain progressive frame of the new view at 1,024 samples, one tick of 8 from history must be nearer than one
    tick of 8 of a restarted frame, and the tick after it must list no more pixels.  (profiles/reproject_figures.txt has the figures.)"""
    c, p = demo.c, params(pkg, 64, 64)
    demo.at(STEP)
    truth = np.zeros((64, 64, 3))
    for k in range(16):
        total = c.render_progressive_soft(p, demo.radii, 0., 5., 64, restart=(k == 0), host_rgb=truth)[1]
    assert total == 1024

    def after_the_step(history):
        c.converge_history(SETTINGS if history else None)
        demo.at()
        for k in range(8):
            rep = demo.tick(p, restart=(k == 0), tol=-1., hi=64)          # a tolerance below 0: every pixel, until it holds 64
        assert rep.max_count == 64
        demo.at(STEP)
        mean = np.zeros((64, 64, 3))
        first = demo.tick(p, hi=1024, host_rgb=mean)
        following = demo.tick(p, hi=1024)
        return float(np.abs(mean - truth).mean()), first, following

    kept, first, following = after_the_step(True)
    assert c.history_info()["last_reprojected"] == 0 and c.history_info()["reprojections"] == 1
    lost, first0, following0 = after_the_step(False)
    print("mean absolute error after one tick of 8: with history %.6g, restarted %.6g; listed by the following tick: %d and %d"
          % (kept, lost, following.listed, following0.listed))
    assert first0.listed == 64 * 64 and first.listed <= first0.listed
    assert kept < lost
    assert following.listed <= following0.listed
