"""Properties of the variance-guided filter's yardstick itself (tests/denoise_reference.py): no GPU, no product code.  They pin
what the header's "So ..." paragraph promises of the rule, on the restatement the GPU is then held to byte for byte."""
import numpy as np

import denoise_reference as DR


def frame(h, w, value=.25, n=8, spread=.01):
    """A flat frame: every pixel `n` samples of colour `value`, y's sample variance spread^2."""
    S = np.full((h, w, 3), value * n)
    y = 3. * value
    stats = np.zeros((h, w, 2))
    stats[..., 0] = y * n
    stats[..., 1] = n * y * y + (n - 1) * spread * spread
    return S, stats, np.full((h, w), n, np.uint32)


def test_the_synthetic_frames_hold_every_branch_of_the_rule():
    for seed, (h, w) in enumerate(((96, 96), (32, 32), (40, 64))):
        S, stats, n, hits = DR.synthetic(seed, h, w)
        assert (n == 0).any() and (n == 1).any() and (n >= 2).any()
        assert (hits["hit"] == 1).any() and (hits["hit"] == 0).any()
        assert len(np.unique(hits["shape"][hits["hit"] == 1])) >= 3
        assert np.all(hits[hits["hit"] == 0] == np.zeros((), DR.HIT_DTYPE))
        nd = np.maximum(n, 1).astype(np.float64)
        m2 = stats[..., 1] - stats[..., 0] * stats[..., 0] / nd
        assert (m2[n >= 2] < 0.).any() and (m2[n >= 2] > 0.).any()     # the clamp of m2 bites somewhere, and not everywhere
        d = (hits["normal"][:, 1:] * hits["normal"][:, :-1]).sum(-1)
        both = (hits["hit"][:, 1:] == 1) & (hits["hit"][:, :-1] == 1) & (hits["shape"][:, 1:] == hits["shape"][:, :-1])
        assert (d[both] <= 0.).any() and (d[both] > 0.).any()          # ... and so does the test of the normals


def test_no_iterations_is_the_mean_and_the_start_variance():
    S, stats, n, hits = DR.synthetic(3, 40, 64)
    ctl = DR.Control(iterations=0, fallback_variance=.5)
    C, V, B = DR.denoise(S, stats, n, hits, ctl)
    assert C.shape == (32, 64, 3) and V.shape == (32, 64) and B.shape == (32, 64, 3)     # rows = 40 - 40 % 32
    n, S, stats = n[:32], S[:32], stats[:32]
    some = n > 0
    assert np.array_equal(C[some], S[some] / n[some].astype(np.float64)[:, None])
    assert np.all(C[~some] == 0.) and np.all(V[n < 2] == .5)
    two = n >= 2
    nd = n[two].astype(np.float64)
    m2 = np.maximum(stats[two][:, 1] - (stats[two][:, 0] * stats[two][:, 0]) / nd, 0.)
    assert np.array_equal(V[two], m2 / (nd * (nd - 1.)))
    assert np.array_equal(B, DR.to_bytes(C))


def test_two_shapes_come_back_exactly():
    h = w = 64
    yy, xx = np.mgrid[0:h, 0:w]
    left = xx + yy // 3 < 40                                             # a slanted edge: taps of every step straddle it
    S, stats, n = frame(h, w, spread=.3)                                 # a large variance: the luminance stop is wide open
    S[left], S[~left] = 8., 0.
    stats[..., 0] = np.where(left, 24., 0.)
    stats[..., 1] = stats[..., 0] * stats[..., 0] / 8. + 7. * .09
    hits = np.zeros((h, w), DR.HIT_DTYPE)
    hits["hit"], hits["shape"], hits["t"], hits["normal"] = 1, np.where(left, 2, 5), 3., (0., 0., 1.)
    hits["point"] = np.stack([xx * .01, yy * .01, np.full((h, w), -3.)], axis=-1)
    hits["element"] = xx % 7                                             # (not compared: a mesh is one surface)
    C, V, _ = DR.denoise(S, stats, n, hits, DR.Control())
    assert np.all(C[left] == 1.) and np.all(C[~left] == 0.)
    unguided, _, _ = DR.denoise(S, stats, n, None, DR.Control())
    assert ((unguided > 0.) & (unguided < 1.)).any()                     # without the guide the edge does blur: the case is no tautology


def test_a_constant_picture_stays_within_an_ulp_and_its_variance_does_not_grow():
    S, stats, n = frame(64, 64, value=.3, n=7, spread=.05)
    C0, V0, _ = DR.denoise(S, stats, n, None, DR.Control(iterations=0))
    v0 = V0[0, 0]
    assert np.all(V0 == v0) and v0 > 0.
    for it in range(1, 6):
        C, V, _ = DR.denoise(S, stats, n, None, DR.Control(iterations=it))
        assert np.all(np.abs(C - C0) <= np.spacing(C0))
        assert np.all(V >= 0.) and np.all(V <= v0 * (1. + 1e-12))
    assert V.max() < .2 * v0                                             # five iterations of averaging do bring it down


def test_variance_is_never_negative():
    S, stats, n, hits = DR.synthetic(5, 96, 96)
    for guide in (None, hits):
        C, V, _ = DR.denoise(S, stats, n, guide, DR.Control())
        assert np.isfinite(C).all() and np.isfinite(V).all() and np.all(V >= 0.)


def test_a_hole_is_filled_from_its_neighbours_and_is_no_tap():
    S, stats, n = frame(32, 32, value=.25)
    n[10, 12] = 0
    S[10, 12] = 1e6                                                      # (what a pixel without samples holds is not looked at)
    stats[10, 12] = (1e6, -1e6)
    C, V, _ = DR.denoise(S, stats, n, None, DR.Control(iterations=1))
    assert np.all(np.abs(C - .25) <= np.spacing(.25))                    # the hole took its neighbours' value and gave them nothing
    C0, _, _ = DR.denoise(S, stats, n, None, DR.Control(iterations=0))
    assert np.all(C0[10, 12] == 0.)
    # a hole whose every tap is rejected keeps C0, V0
    hits = np.zeros((32, 32), DR.HIT_DTYPE)
    hits["hit"], hits["normal"] = 1, (0., 0., 1.)
    hits["shape"][10, 12] = 9
    C, V, _ = DR.denoise(S, stats, n, hits, DR.Control(iterations=3, fallback_variance=.125))
    assert np.all(C[10, 12] == 0.) and V[10, 12] == .125




def test_at_step_16_a_frame_of_32_sees_the_centre_and_its_three_partners_alone():
    """In a frame of 32 x 32 at step 16 every tap with |dx| = 2 or |dy| = 2 lies 32 pixels away, out of bounds for every pixel, and
    of dx = +-1 exactly one lies inside: 16 pixels towards the frame's middle.  So a pixel folds at most four taps -- itself, its
    horizontal, its vertical and its diagonal partner, in tap order -- restated here by hand, with rolls by 16 instead of the
    yardstick's shifts.  (The centre tap ALONE is what remains one step further, at step 32, which no call reaches.)"""
    S, stats, n, _ = DR.synthetic(7, 32, 32)
    ctl = DR.Control()
    C, V = DR.start(S, stats, n, 1.)
    got_C, got_V = DR.iteration(C, V, n, None, ctl, 16)
    y = DR.y_of(C)
    den = (np.float64(ctl.sigma_l) * np.float64(ctl.sigma_l)) * DR.prefilter(V) + np.float64(ctl.epsilon)
    yy, xx = np.mgrid[0:32, 0:32]
    want_C, want_V = np.full_like(C, np.nan), np.full_like(V, np.nan)
    for ys in (1, -1):
        for xs in (1, -1):
            quadrant = ((yy < 16) == (ys == 1)) & ((xx < 16) == (xs == 1))
            sw, sv, sc = np.zeros_like(V), np.zeros_like(V), np.zeros_like(C)
            for dy, dx in sorted([(0, 0), (0, xs), (ys, 0), (ys, xs)]):
                roll = lambda a: np.roll(np.roll(a, -16 * dy, axis=0), -16 * dx, axis=1)   # q = p + 16 (dx, dy), inside by the quadrant
                a = y - roll(y)
                w = (DR.H5[dx + 2] * DR.H5[dy + 2]) * np.where(n > 0, den / (den + a * a), 1.)
                use = roll(n) > 0
                sw = np.where(use, sw + w, sw)
                sc = np.where(use[..., None], sc + w[..., None] * roll(C), sc)
                sv = np.where(use, sv + (w * w) * roll(V), sv)
            with np.errstate(all="ignore"):
                qC, qV = np.where((sw > 0.)[..., None], sc / sw[..., None], C), np.where(sw > 0., sv / (sw * sw), V)
            want_C[quadrant], want_V[quadrant] = qC[quadrant], qV[quadrant]
    assert np.array_equal(got_C, want_C) and np.array_equal(got_V, want_V)
    assert not np.array_equal(got_C, C)                                  # (the partners do count)
    # one step further only the centre is left: C' = (w C) / w, V' = (w w V) / (w w) with w = h(0) h(0), and a hole stays a hole
    C3, V3 = DR.iteration(C, V, n, None, ctl, 32)
    w, some = 9. / 64., n > 0
    assert np.array_equal(C3[some], (w * C[some]) / w) and np.array_equal(V3[some], ((w * w) * V[some]) / (w * w))
    assert np.array_equal(C3[~some], C[~some]) and np.array_equal(V3[~some], V[~some])
