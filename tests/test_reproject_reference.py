"""The temporal reprojection's yardstick held to its own properties (tests/reproject_reference.py): no GPU, no product code.

The frames are synthetic: a plane one unit in front of a camera whose numbers are powers of two (32 x 32 or 64 x 32 pixels,
half_fov 0.5), so that the hit points and, for the identical view, the sample positions are exact."""
import numpy as np
import pytest

import reproject_reference as R

H, W = 32, 32
FRAME = R.Frame(width=W, height=H, ratio=1., half_fov=.5)


def halves(P):
    """Two shapes: 0 left of x = 0, 1 right of it"""
    return (P[..., 0] >= 0.).astype(np.uint32)


def picture(hits, n, values=(1., 0.)):
    """A frame that holds exactly n * values[shape] in every channel and in both moments (no picture has such moments: what
    is carried is carried whatever it means)"""
    v = np.where(hits["shape"] == 0, values[0], values[1])
    nd = n.astype(np.float64)
    S = np.repeat((nd * v)[..., None], 3, axis=-1)
    return S, np.stack([nd * v, nd * v], axis=-1)


def counts(seed, h=H, w=W, lo=1, hi=40):
    return np.random.default_rng(seed).integers(lo, hi, size=(h, w)).astype(np.uint32)


def test_a_two_shape_picture_comes_back_exact():
    prev_view = R.View()
    prev_hits = R.plane_hits(prev_view, FRAME, H, W, 1., halves)
    n = counts(1)
    S, stats = picture(prev_hits, n)
    for step in ((.0371, 0., 0.), (-.013, .021, 0.), (0., 0., .3), (.11, -.07, -.2)):
        view = R.View(position=step)
        # the new view sees the same plane z = -1: its points by its own rays, pushed onto the plane
        cur = R.plane_hits(view, FRAME, H, W, 1. + step[2], halves)
        taps = []
        gS, gstats, gn, carried = R.reproject(S, stats, n, prev_hits, cur, prev_view, FRAME, R.Control(max_history=16), taps)
        assert carried.sum() > H * W // 3 and (taps[0] >= 2).sum() > H * W // 4, step   # fractional positions: the taps do blend
        nd = gn.astype(np.float64)
        want = np.where(cur["shape"] == 0, 1., 0.) * nd
        assert (gS == want[..., None]).all(), step                       # exactly n' * 1. and n' * 0.: nothing crossed x = 0
        assert (gstats[..., 0] == want).all() and (gstats[..., 1] == want).all()
        assert (gn[carried == 0] == 0).all() and (gn[carried == 1] >= 1).all() and gn.max() <= 16
        assert (gS[carried == 0] == 0.).all() and not np.signbit(gS[carried == 0]).any()


def test_an_identical_view_on_integer_positions_takes_exactly_one_tap():
    view = R.View()
    hits = R.plane_hits(view, FRAME, H, W, 1., halves)
    sx, sy, ok = R.sample_positions(hits, view, FRAME, W, H)
    yy, xx = np.mgrid[0:H, 0:W]
    assert ok.all() and (sx == xx).all() and (sy == yy).all()            # the inverse of the sample-ray formula, exactly
    r = np.random.default_rng(2)
    n = counts(2)
    S, stats = r.random((H, W, 3)) * n[..., None], r.random((H, W, 2)) * n[..., None]
    taps = []
    gS, gstats, gn, carried = R.reproject(S, stats, n, hits, hits, view, FRAME, R.Control(max_history=65536), taps)
    assert (taps[0] == 1).all() and carried.all() and (gn == n).all()
    nd = n.astype(np.float64)
    assert (gS == ((1. * (S / nd[..., None])) / 1.) * nd[..., None]).all()   # the pixel's own mean times its own count
    assert np.allclose(gS, S, rtol=4e-16, atol=0.) and np.allclose(gstats, stats, rtol=4e-16, atol=0.)


def test_behind_the_camera_outside_the_frustum_and_nan_carry_nothing():
    prev_view = R.View()
    prev_hits = R.plane_hits(prev_view, FRAME, H, W, 1., halves)
    n = counts(3)
    S, stats = picture(prev_hits, n, (.5, .25))
    cur = prev_hits.copy()
    cur["point"][0, :, 2] = .5                                           # behind the previous camera: zf < 0
    cur["point"][1, :, 2] = 0.                                           # in its plane: zf == 0
    cur["point"][2, :, 0] = 40.                                          # far to the right of the frustum
    cur["point"][3, :, 1] = -40.                                         # far below it
    cur["point"][4, :8, 0] = np.nan
    cur["point"][4, 8:16, 2] = np.inf
    cur["point"][4, 16:24, 1] = -np.inf
    cur["point"][4, 24:, 0] = 1e300
    cur["hit"][5] = 0                                                    # the sky
    cur["shape"][6] = 7                                                  # a shape the previous view never saw
    cur["normal"][7] = (0., 1., 0.)                                      # a surface that faces another way
    cur["point"][8, :, 2] -= 1.                                          # one unit off the tangent plane, at the same sample position
    cur["point"][8, :, :2] *= 2.
    gS, gstats, gn, carried = R.reproject(S, stats, n, prev_hits, cur, prev_view, FRAME, R.Control())
    assert not carried[:9].any() and (gn[:9] == 0).all() and (gS[:9] == 0.).all() and (gstats[:9] == 0.).all()
    assert carried[9:].all()
    # ... and NaN or garbage in the previous frame never reaches an index: the call ends, and pixels elsewhere are what they were
    bad_hits = prev_hits.copy()
    bad_hits["point"][20:] = np.nan
    bad_hits["normal"][24:] = np.inf
    bad_n = n.copy()
    bad_n[20:] = 0xdeadbeef
    g2 = R.reproject(S, stats, bad_n, bad_hits, cur, prev_view, FRAME, R.Control())
    assert (g2[0][9:19] == gS[9:19]).all() and (g2[2][9:19] == gn[9:19]).all()
    assert not g2[3][20:].any()                                          # e is NaN there: e*e <= dz is false


def test_the_clamp_and_the_minimum_of_counts():
    prev_view, view = R.View(), R.View(position=(1. / 64., 1. / 64., 0.))   # a quarter of a pixel each way: four taps
    prev_hits = R.plane_hits(prev_view, FRAME, H, W, 1., lambda P: np.zeros(P.shape[:2], np.uint32))
    cur = R.plane_hits(view, FRAME, H, W, 1., lambda P: np.zeros(P.shape[:2], np.uint32))
    n = counts(4, lo=1, hi=200)
    S, stats = picture(prev_hits, n, (.5, .5))
    taps = []
    _, _, gn, carried = R.reproject(S, stats, n, prev_hits, cur, prev_view, FRAME, R.Control(max_history=65536), taps)
    inner = np.zeros((H, W), bool)
    inner[1:-1, 1:-1] = True
    assert (taps[0][inner] == 4).all() and carried[inner].all()
    sx, sy, _ = R.sample_positions(cur, prev_view, FRAME, W, H)
    x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
    for y, x in ((5, 5), (17, 9), (30, 30), (1, 20)):
        assert gn[y, x] == n[y0[y, x]:y0[y, x] + 2, x0[y, x]:x0[y, x] + 2].min()
    for most in (1, 8, 50):
        _, _, clamped, _ = R.reproject(S, stats, n, prev_hits, cur, prev_view, FRAME, R.Control(max_history=most))
        assert (clamped == np.minimum(gn, most)).all() and clamped.max() == most
    # a tap without samples takes no part, in the minimum either
    holes = n.copy()
    holes[::2, ::2] = 0
    taps = []
    _, _, hn, hc = R.reproject(S, stats, holes, prev_hits, cur, prev_view, FRAME, R.Control(max_history=65536), taps)
    assert (taps[0][inner] == 3).all() and (hn[inner] >= 1).all() and hc[inner].all()


def test_the_carried_second_moment_is_at_least_the_square_of_the_first():
    r = np.random.default_rng(5)
    prev_view, view = R.View(), R.View(position=(.031, -.017, .05))
    prev_hits = R.plane_hits(prev_view, FRAME, H, W, 1., halves)
    cur = R.plane_hits(view, FRAME, H, W, 1.05, halves)
    n = counts(5, lo=2, hi=64)
    nd = n.astype(np.float64)
    # real moments: sums of y and y*y over n samples a pixel
    ys = [r.random((H, W)) * (1. + 3. * (k % 3)) for k in range(64)]
    Y, Q = np.zeros((H, W)), np.zeros((H, W))
    for k, y in enumerate(ys):
        Y, Q = np.where(k < n, Y + y, Y), np.where(k < n, Q + y * y, Q)
    S = np.repeat((Y / 3.)[..., None], 3, axis=-1)
    _, gstats, gn, carried = R.reproject(S, np.stack([Y, Q], axis=-1), n, prev_hits, cur, prev_view, FRAME, R.Control(max_history=24))
    assert carried.sum() > H * W // 2
    gd = gn.astype(np.float64)[carried == 1]
    Y2, Q2 = gstats[..., 0][carried == 1], gstats[..., 1][carried == 1]
    m2 = Q2 - (Y2 * Y2) / gd                                             # what the converging rule forms: n' times the variance
    assert (m2 >= -1e-12 * Q2).all() and (m2 > 0.).any()


def test_rows_from_rows_on_are_untouched():
    h = 40                                                               # 8 rows below the last whole patch row
    frame = R.Frame(width=W, height=32., ratio=1., half_fov=.5)
    prev_view, view = R.View(), R.View(position=(0., -3. / 64., 0.))     # the new view looks 1.5 pixels lower
    zero = lambda P: np.zeros(P.shape[:2], np.uint32)
    prev_hits, cur = R.plane_hits(prev_view, frame, h, W, 1., zero), R.plane_hits(view, frame, h, W, 1., zero)
    n = counts(6, h=h)
    S, stats = picture(prev_hits, n, (.5, .5))
    S[32:], stats[32:], n[32:] = np.nan, np.nan, 0xffffffff              # what lies there is no part of the frame
    prev_hits["point"][32:] = np.nan
    gS, gstats, gn, carried = R.reproject(S, stats, n, prev_hits, cur, prev_view, frame, R.Control(max_history=65536))
    assert gS.shape == (32, W, 3) and gstats.shape == (32, W, 2) and gn.shape == carried.shape == (32, W)
    sx, sy, ok = R.sample_positions(cur[:32], prev_view, frame, W, 32)
    assert (sy[30] == 31.5).all() and (sy[31] == 32.5).all()
    assert carried[:31].all() and not carried[31].any()                  # sy = 32.5 is not < rows: nothing of row 32 is read
    assert np.isfinite(gS).all() and (gn[30] == n[31]).all()             # row 30 took row 31 alone: the tap on row 32 is skipped
