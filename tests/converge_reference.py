"""The yardstick of the converging frames' tests (include/rusty_marcher_amd.h, "converging frames"): the select rule and the fold
restated in numpy, operation for operation as the header states them, over progressive_reference.samples / soft_reference.samples,
which hold every row of the sequences for every pixel on the CPU.  No GPU, no product code.

The tests demand masks, lists and counts exactly, no pixel left out.  That is legitimate only where no decision is close: the
GPU's samples differ from the oracle's by up to TIGHT a channel, so its (Y, Q) differ a little and a pixel whose m2 sits on the
bound could fall either way.  So `run` asserts, for every decision that is not forced (by tolerance < 0, min_samples or the cap),
    |m2 - bound| > 12 n ymax TIGHT,
ymax the case's largest |y|: a deviation of TIGHT a channel moves y by at most 3 TIGHT, Y by 3 n TIGHT, y y by 6 ymax TIGHT
(+ 9 TIGHT^2), Q by 6 n ymax TIGHT, (Y Y) / n by 2 |Y| 3 n TIGHT / n <= 6 n ymax TIGHT: m2 by at most 12 n ymax TIGHT.  The
cases the tests use were chosen so that the reference alone satisfies this (tests/test_converge_abi.py prints the nearest one).

tests/test_converge_abi.py pins this file's properties and shows the cases are not vacuous; tests/test_gpu_converge.py holds the
GPU to it."""
import numpy as np

import lens_reference as LR
import progressive_reference as PR
import soft_reference as SR

TIGHT = PR.TIGHT                     # the project's parity bound, per channel, no pixel left out
MAX_SAMPLES = PR.MAX_SAMPLES


def y_of(c):
    """y = (r + g) + b of samples [..., 3]."""
    c = np.asarray(c, dtype=np.float64)
    return (c[..., 0] + c[..., 1]) + c[..., 2]


def capped(n, ns, max_samples):
    return n.astype(np.int64) + ns > max_samples


def unsettled(n, Y, Q, tolerance, min_samples):
    """The header's rule per pixel, every operation rounded once; a NaN leaves the pixel unsettled."""
    n = np.asarray(n)
    if tolerance < 0.:
        return np.ones(n.shape, bool)
    few = n < max(min_samples, 2)
    nd = n.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        m2 = Q - (Y * Y) / nd
        bound = (np.float64(tolerance) * np.float64(tolerance)) * (nd * (nd - 1.))
        return few | ~(m2 <= bound)


def dilate(noisy, width, rows):
    """noisy, or a noisy neighbour among left, right, above, below inside [0, width) x [0, rows)."""
    g = noisy.reshape(rows, width)
    out = g.copy()
    out[:, 1:] |= g[:, :-1]
    out[:, :-1] |= g[:, 1:]
    out[1:] |= g[:-1]
    out[:-1] |= g[1:]
    return out.reshape(-1)


def select(n, Y, Q, width, rows, ns, tolerance, min_samples, max_samples):
    """-> (listed, noisy): bool per pixel of [0, rows) x [0, width), row-major."""
    cap = capped(n, ns, max_samples)
    noisy = ~cap & unsettled(n, Y, Q, tolerance, min_samples)
    return ~cap & dilate(noisy, width, rows), noisy


def nearest_decision(n, Y, Q, ns, tolerance, min_samples, max_samples, ymax):
    """The smallest (|m2 - bound| / (12 n ymax TIGHT)) over the decisions that are not forced; inf where every one is."""
    if tolerance < 0.:
        return np.inf
    free = ~capped(n, ns, max_samples) & ~(n < max(min_samples, 2))
    if not free.any():
        return np.inf
    nd = n[free].astype(np.float64)
    m2 = Q[free] - (Y[free] * Y[free]) / nd
    bound = (np.float64(tolerance) * np.float64(tolerance)) * (nd * (nd - 1.))
    assert np.isfinite(m2).all()
    return float((np.abs(m2 - bound) / (12. * nd * ymax * TIGHT)).min())


class State:
    """sum [pixels][3], stats (Y, Q) [pixels], count [pixels] of a converging frame; pixels = rows x width, row-major."""

    def __init__(self, width, rows):
        self.width, self.rows = width, rows
        p = width * rows
        self.S, self.Y, self.Q = np.zeros((p, 3)), np.zeros(p), np.zeros(p)
        self.n = np.zeros(p, dtype=np.uint32)
        self.mean = np.zeros((p, 3))

    def copy(self):
        c = State(self.width, self.rows)
        c.S, c.Y, c.Q, c.n, c.mean = self.S.copy(), self.Y.copy(), self.Q.copy(), self.n.copy(), self.mean.copy()
        return c


def one_pass(state, samples, ns, tolerance, min_samples, max_samples, fresh, ymax=None):
    """One call of rm_accumulate_converging_device on `state` (changed in place) over samples [pixel][row][3] ->
    (listed bool per pixel, nearest decision).  With ymax given the margin of every free decision is asserted."""
    if fresh:
        state.n[:] = 0
    listed, _ = select(state.n, state.Y, state.Q, state.width, state.rows, ns, tolerance, min_samples, max_samples)
    near = np.inf
    if ymax is not None:
        near = nearest_decision(state.n, state.Y, state.Q, ns, tolerance, min_samples, max_samples, ymax)
        assert near > 1., "a decision lies within 12 n ymax TIGHT of its bound (%.3g of it): not a case for exact masks" % near
    idx = np.flatnonzero(listed)
    n = state.n[idx].astype(np.int64)
    assert (n + ns <= samples.shape[1]).all()
    first = n == 0
    S, Y, Q = state.S[idx].copy(), state.Y[idx].copy(), state.Q[idx].copy()
    for t in range(ns):
        c = samples[idx, n + t]
        y = y_of(c)
        if t == 0:
            S = np.where(first[:, None], c, S + c)
            Y = np.where(first, y, Y + y)
            Q = np.where(first, y * y, Q + y * y)
        else:
            S, Y, Q = S + c, Y + y, Q + y * y
    state.S[idx], state.Y[idx], state.Q[idx] = S, Y, Q
    state.n[idx] = (n + ns).astype(np.uint32)
    state.mean[idx] = S / (n + ns).astype(np.float64)[:, None]
    return listed, near


def run(samples, width, rows, ns, tolerance, min_samples, max_samples, passes=None, check=True):
    """Passes of a frame, the first fresh, until nothing is listed (or `passes` of them) -> (records, nearest decision): a
    record a pass, (listed, the State after it)."""
    ymax = float(np.abs(y_of(samples[:, :max_samples])).max()) if check else None
    state, out, nearest, k = State(width, rows), [], np.inf, 0
    while passes is None or k < passes:
        listed, near = one_pass(state, samples, ns, tolerance, min_samples, max_samples, k == 0, ymax)
        nearest = min(nearest, near)
        out.append((listed, state.copy()))
        k += 1
        if passes is None and not listed.any():
            break
        assert k <= 8 * (max_samples // ns + 2)                          # (a safety stop: a pixel listed late, as a neighbour, can outlast max_samples / ns passes)
    return out, nearest


def prefix_sums(samples, counts):
    """The plain run's (sum, mean) [pixel][3] at a count per pixel: the left fold of the first counts[p] rows of pixel p."""
    out_s, out_m = np.zeros((samples.shape[0], 3)), np.zeros((samples.shape[0], 3))
    acc = samples[:, 0].copy()
    for c in range(1, int(counts.max()) + 1):
        if c > 1:
            acc = acc + samples[:, c - 1]
        at = counts == c
        out_s[at], out_m[at] = acc[at], acc[at] / float(c)
    return out_s, out_m


class Yardstick(SR.Yardstick):
    """SR.Yardstick with every row of the sequences for every pixel, made once a case and shared (never written to)."""

    def __init__(self, pkg, O, orc):
        super().__init__(pkg, O, orc)
        self._rows = {}

    def samples(self, name, w, h, depth, aperture, focus, n_rows, radii=None, view=None):
        """[pixel][row][3] over rows [0, n_rows) of rm_lens_sequence (and of rm_light_sequence for `radii`)."""
        key = (name, w, h, depth, float(aperture), float(focus), n_rows, None if radii is None else tuple(radii), view)
        if key not in self._rows:
            eye, basis = (self.eye(name), None) if view is None else view
            table = PR.lens_sequence(0, n_rows)
            oscene = self.scene(name)[1]
            if radii is None:
                s = PR.samples(self.orc, oscene, eye, basis, w, h, depth, aperture, focus, table)
            else:
                s = SR.samples(self.O, self.orc, oscene, eye, basis, w, h, depth, aperture, focus, table, SR.light_sequence(0, n_rows, radii))
            s.setflags(write=False)
            self._rows[key] = s
        return self._rows[key]


# The cases both test files use, 32 x 32: name -> (scene, depth, aperture, radii or None, n_samples, tolerance, min_samples,
# max_samples).  Depth 6 takes the kernels with STACK = 32, the 256 spheres those with the hierarchy; with 5 samples a wave has
# idle lanes; "demo-capped", "demo-soft-64" and "penumbra-1" run into the cap, the others finish before it.
CASES = {
    "demo-8": ("demo", 3, LR.APERTURE, None, 8, 0.1, 16, 256),
    "penumbra-8": ("penumbra", 3, 0., SR.PENUMBRA_RADII, 8, 0.1, 16, 256),
    "demo-5": ("demo", 3, LR.APERTURE, None, 5, 0.1, 16, 256),
    "spheres-8": ("synthetic256", 6, LR.APERTURE, None, 8, 0.1, 16, 256),
    "demo-soft-64": ("demo", 3, LR.APERTURE, (1.5, 3.), 64, 0.05, 16, 256),
    "penumbra-1": ("penumbra", 3, LR.APERTURE, SR.PENUMBRA_RADII, 1, 0.1, 16, 40),
    "demo-capped": ("demo", 3, LR.APERTURE, None, 8, 0.05, 16, 256),
}
# What the reference alone finds for them (tests/test_converge_abi.py): name -> (passes until nothing is listed, samples cast,
# distinct final counts)
FOUND = {"demo-8": (24, 30672, 20), "penumbra-8": (21, 33808, 18), "demo-5": (38, 32580, 25), "spheres-8": (29, 55040, 25),
         "demo-soft-64": (5, 121984, 4), "penumbra-1": (41, 22273, 22), "demo-capped": (33, 74328, 30)}


def case_samples(Y, name, w=32, h=32, view=None):
    scene, depth, aperture, radii, ns, tol, lo, hi = CASES[name]
    return Y.samples(scene, w, h, depth, aperture, LR.FOCUS, hi, radii, view)
