"""The yardstick of the thin-lens camera's tests (include/rusty_marcher_amd.h, "thin-lens camera"): rm_lens_table and the
lens rays restated in numpy, operation for operation as the header states them, and the resolve in table order.  No GPU, no
product code.  The rays are cast by radiance_reference.OracleRadiance.cast(..., normalize=True) -- orc_cast_ray with an
origin per ray, the yardstick of the radiance tests; tests/test_lens_abi.py pins this file on orc_render and on the
library's table, tests/test_gpu_lens.py holds the GPU to it."""
import numpy as np

import radiance_reference as RR
import workloads

TIGHT = RR.TIGHT                     # the project's parity bound, per channel, no pixel left out
# The settings the non-vacuity pin and the GPU tests share: the demo scene's glass sphere (centre z = -5, radius 2) lies in
# the plane in focus, the mirror sphere (z = -18) and the far floor do not.
APERTURE, FOCUS = 0.4, 5.
# pixels of the demo's 64 x 64 lens frame (16 samples, depth 3) that differ from the aperture-0 frame of the same table by more
# than 0.05 in some channel (tests/test_lens_abi.py)
BLURRED = 788


def rows_of(height):
    """The rows a lens frame writes."""
    return height - height % 32


def lens_table(n):
    """rm_lens_table: (n, 4) rows (dx, dy, u, v), every operation rounded once in the header's order."""
    assert 1 <= n <= 64
    m = 1
    while m * m < n:
        m += 1                                                   # ceil(sqrt(n)) in integers
    dm = np.float64(m)
    t = np.empty((n, 4))
    for s in range(n):
        i, j = s % m, s // m
        a = np.float64(2 * j + 1) / dm - 1.
        b = np.float64(2 * (m - 1 - i) + 1) / dm - 1.
        t[s, 0] = np.float64(i) / dm
        t[s, 1] = np.float64(j) / dm
        t[s, 2] = a * np.sqrt(1. - b * b / 2.)
        t[s, 3] = b * np.sqrt(1. - a * a / 2.)
    return t


def supersample_table(n):
    """(i / n, j / n, 0, 0), j outer and i inner: with aperture 0 the supersampled frame."""
    t = np.zeros((n * n, 4))
    for s in range(n * n):
        t[s, 0] = np.float64(s % n) / np.float64(n)
        t[s, 1] = np.float64(s // n) / np.float64(n)
    return t


def random_table(rng, n):
    """A valid table that is not the library's: offsets in [0, 1), lens points in the unit disc (the rim included: row 0)."""
    t = np.empty((n, 4))
    t[:, :2] = rng.uniform(0., 1., (n, 2))
    r, phi = np.sqrt(rng.uniform(0., 1., n)) * 0.999, rng.uniform(0., 2. * np.pi, n)
    t[:, 2], t[:, 3] = r * np.cos(phi), r * np.sin(phi)
    t[0, 2:] = (1., 0.)
    assert table_ok(t)
    return t


def table_ok(t):
    """The conditions rm_render_lens checks of a table."""
    t = np.asarray(t, dtype=np.float64)
    return bool(t.ndim == 2 and t.shape[1] == 4 and np.isfinite(t).all() and (t[:, :2] >= 0.).all() and (t[:, :2] < 1.).all()
                and (t[:, 2] * t[:, 2] + t[:, 3] * t[:, 3] <= 1. + 1e-12).all())


def lens_rays(width, rows, r, eye, basis, aperture, focus, table):
    """Steps 1-4 for every pixel of [0, rows) and every table row: (origins, un-normalised directions), each
    (rows * width * n, 3) in the order [y][x][s].  r: the Renderer (width, height, half_fov, ratio); basis: (right, up,
    forward) of an oriented context, None for the fixed view."""
    table = np.asarray(table, dtype=np.float64)
    n = table.shape[0]
    pix = RR.pixel_positions(width, rows)                                     # (x, y), row-major
    xy = np.empty((rows * width, n, 2))
    xy[..., 0] = pix[:, 0][:, None] + table[:, 0][None, :]                    # sx = x + dx
    xy[..., 1] = pix[:, 1][:, None] + table[:, 1][None, :]                    # sy = y + dy
    D = RR.sample_directions(xy.reshape(-1, 2), r, basis)                     # 1. (bx * right + by * up) + forward, or (bx, by, -1)
    eye = np.asarray(eye, dtype=np.float64)
    if aperture == 0.:                                                        # 4., the exception: the sample ray itself
        return np.ascontiguousarray(np.broadcast_to(eye, D.shape)), D
    right, up, _ = basis if basis is not None else RR.FIXED_VIEW
    aperture, focus = np.float64(aperture), np.float64(focus)
    au, av = aperture * table[:, 2], aperture * table[:, 3]                   # 3.
    F, O = np.empty_like(D), np.empty((n, 3))
    for c in range(3):
        F[:, c] = eye[c] + D[:, c] * focus                                    # 2. one product, one sum
        O[:, c] = eye[c] + ((au * right[c]) + (av * up[c]))
    O = np.ascontiguousarray(np.broadcast_to(O[None], (rows * width, n, 3))).reshape(-1, 3)
    return O, F - O                                                           # 4. normalised by the oracle's own normalized()


def resolve(samples):
    """[pixel][s][3] -> [pixel][3]: summed per channel in table order by plain additions, divided once by n."""
    s = np.asarray(samples, dtype=np.float64)
    acc = s[:, 0].copy()
    for t in range(1, s.shape[1]):
        acc = acc + s[:, t]
    return acc / float(s.shape[1])


def frame(orc, oscene, eye, basis, width, height, depth, aperture, focus, table):
    """The reference lens frame, [height][width][3]; rows from rows_of(height) on are zero."""
    rows = rows_of(height)
    out = np.zeros((height, width, 3))
    if rows:
        n = np.asarray(table).shape[0]
        o, d = lens_rays(width, rows, orc.renderer(width, height), eye, basis, aperture, focus, table)
        rgb = orc.cast(oscene, o, d, depth, normalize=True)
        out[:rows] = resolve(rgb.reshape(rows * width, n, 3)).reshape(rows, width, 3)
    return out


class Yardstick:
    """Oracle scenes and reference lens frames, each made once and shared (never written to)."""

    def __init__(self, pkg, O, orc):
        self.pkg, self.O, self.orc = pkg, O, orc
        self._scene, self._frame = {}, {}

    def scene(self, name):
        if name not in self._scene:
            self._scene[name] = (workloads.product_scene(self.pkg, name), workloads.oracle_scene(self.O, name))
        return self._scene[name]

    def eye(self, name):
        return self.scene(name)[1].c.camera.tup()

    def frame(self, name, w, h, depth, aperture, focus, table, view=None):
        """view = (eye, basis) of an oriented context; None: the scene's camera and the fixed view."""
        t = np.ascontiguousarray(table, dtype=np.float64)
        key = (name, w, h, depth, float(aperture), float(focus), t.tobytes(), view)
        if key not in self._frame:
            eye, basis = (self.eye(name), None) if view is None else view
            f = frame(self.orc, self.scene(name)[1], eye, basis, w, h, depth, aperture, focus, t)
            f.setflags(write=False)
            self._frame[key] = f
        return self._frame[key]
