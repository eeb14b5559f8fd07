"""The yardstick of the progressive frames' tests (include/rusty_marcher_amd.h, "progressive frames"): rm_lens_sequence, the
continued sum, its mean and its display bytes restated in numpy, operation for operation as the header states them.  No GPU,
no product code.  The rays are lens_reference.lens_rays', cast by radiance_reference.OracleRadiance.cast(..., normalize=True);
tests/test_progressive_abi.py pins this file on the library's sequence and shows it is not vacuous,
tests/test_gpu_progressive.py holds the GPU to it."""
import numpy as np

import lens_reference as LR

TIGHT = LR.TIGHT                     # the project's parity bound, per channel, no pixel left out
MAX_SAMPLES = 65536                  # RM_PROGRESSIVE_MAX_SAMPLES
# pixels of the demo's 32 x 32 frame (depth 3, LR.APERTURE / LR.FOCUS) whose mean after 192 samples of the sequence differs from
# the mean after the first 4 by more than 0.05 in some channel (tests/test_progressive_abi.py)
REFINED = 318


def digit_reversed(s, b):
    """The digits of s in base b mirrored at the point, as the integer pair (r, q): phi_b(s) = r / q."""
    r, q = 0, 1
    while s > 0:
        r, q, s = r * b + s % b, q * b, s // b
    return r, q


def lens_sequence(first, count):
    """rm_lens_sequence: rows first .. first + count - 1, (count, 4) rows (dx, dy, u, v), every operation rounded once in the
    header's order."""
    assert first >= 0 and count >= 0 and first + count <= MAX_SAMPLES
    t = np.empty((count, 4))
    for k in range(count):
        phi = []
        for base in (2, 3, 5, 7):
            r, q = digit_reversed(first + k, base)
            phi.append(np.float64(r) / np.float64(q))                # (r, q < 2^53: exact before the one division)
        a = 2. * phi[2] - 1.
        b = 2. * phi[3] - 1.
        t[k, 0] = phi[0]
        t[k, 1] = phi[1]
        t[k, 2] = a * np.sqrt(1. - b * b / 2.)
        t[k, 3] = b * np.sqrt(1. - a * a / 2.)
    return t


def accumulate(prev_sum, samples, n_before):
    """One pass: samples [pixel][s][3] added to prev_sum [pixel][3] (not read when n_before == 0: the sum starts as the first
    sample itself) in table order by plain additions -> (sum, mean = sum / (n_before + n))."""
    s = np.asarray(samples, dtype=np.float64)
    if n_before > 0:
        acc, t0 = np.array(prev_sum, dtype=np.float64), 0
    else:
        acc, t0 = s[:, 0].copy(), 1
    for t in range(t0, s.shape[1]):
        acc = acc + s[:, t]
    return acc, acc / float(n_before + s.shape[1])


def to_bytes(mean):
    """to_vec: (uint8_t)(255. * fmin(fmax(mean, 0.), 1.)) per channel."""
    return (255. * np.fmin(np.fmax(np.asarray(mean, dtype=np.float64), 0.), 1.)).astype(np.uint8)


def samples(orc, oscene, eye, basis, width, height, depth, aperture, focus, table):
    """The radiance of every lens ray of the rows a frame writes: [pixel][s][3], pixels row-major."""
    rows = LR.rows_of(height)
    n = np.asarray(table).shape[0]
    o, d = LR.lens_rays(width, rows, orc.renderer(width, height), eye, basis, aperture, focus, table)
    return orc.cast(oscene, o, d, depth, normalize=True).reshape(rows * width, n, 3)


def frames(orc, oscene, eye, basis, width, height, depth, aperture, focus, table, passes):
    """The passes `passes` (their sizes, in order) over consecutive slices of `table`, begun with n_before = 0 ->
    (sum, mean) after the last, each [height][width][3] with zero rows from rows_of(height) on."""
    rows = LR.rows_of(height)
    assert sum(passes) == np.asarray(table).shape[0]
    s = samples(orc, oscene, eye, basis, width, height, depth, aperture, focus, table)
    acc, mean, done = None, None, 0
    for n in passes:
        acc, mean = accumulate(acc, s[:, done:done + n], done)
        done += n
    out_sum, out_mean = np.zeros((height, width, 3)), np.zeros((height, width, 3))
    out_sum[:rows], out_mean[:rows] = acc.reshape(rows, width, 3), mean.reshape(rows, width, 3)
    return out_sum, out_mean


class Yardstick(LR.Yardstick):
    """LR.Yardstick with reference progressive frames, each made once and shared (never written to)."""

    def __init__(self, pkg, O, orc):
        super().__init__(pkg, O, orc)
        self._progressive = {}

    def progressive(self, name, w, h, depth, aperture, focus, table, passes, view=None):
        """(sum, mean) after the passes over `table`; view = (eye, basis) of an oriented context, None: the fixed view."""
        t = np.ascontiguousarray(table, dtype=np.float64)
        key = (name, w, h, depth, float(aperture), float(focus), t.tobytes(), tuple(passes), view)
        if key not in self._progressive:
            eye, basis = (self.eye(name), None) if view is None else view
            pair = frames(self.orc, self.scene(name)[1], eye, basis, w, h, depth, aperture, focus, t, passes)
            for f in pair:
                f.setflags(write=False)
            self._progressive[key] = pair
        return self._progressive[key]
