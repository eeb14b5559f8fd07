"""The yardstick of the adaptive anti-aliasing's tests (include/rusty_marcher_amd.h, "adaptive anti-aliasing"): contrast,
mask and refined frame restated in numpy as the header states them.  No GPU, no product code.  The samples a refined
pixel averages come from radiance_reference.OracleRadiance.cast over radiance_reference.sample_directions, the yardstick
of the radiance tests; tests/test_antialias_abi.py pins this file on the oracle's frames, tests/test_gpu_antialias.py
holds the GPU to it."""
import numpy as np

import radiance_reference as RR
import workloads

TIGHT = RR.TIGHT                     # the project's parity bound, per channel, no pixel left out
THRESHOLD = 0.125
MARGIN = 1e-6                        # no contrast of a tested frame lies this near the threshold: the masks can be demanded exactly
# (scene, frame width, frame height, max_depth) -> pixels refined at THRESHOLD, counted on the oracle's frame
FRAMES = {("demo", 64, 64, 3): 1073, ("demo", 96, 64, 5): 1280, ("cornell", 64, 64, 3): 198,
          ("synthetic256", 64, 64, 6): 1738, ("demo", 32, 32, 3): 436}


def rows_of(height):
    """The rows a render writes."""
    return height - height % 32


def _take(c, a, b):
    """c = max(c, |a - b|) per channel; a NaN makes its comparison false."""
    with np.errstate(invalid="ignore"):
        for k in range(3):
            d = np.abs(a[..., k] - b[..., k])
            np.copyto(c, d, where=d > c)


def contrast(frame, rows):
    """[rows][width]: the largest |f[y][x][c] - f[q][c]| over the channels and the up-to-four neighbours q of (x, y) inside
    [0, width) x [0, rows), on the frame as it is; 0 for a pixel without a neighbour."""
    f = np.asarray(frame, dtype=np.float64)[:rows]
    c = np.zeros(f.shape[:2])
    _take(c[:, 1:], f[:, 1:], f[:, :-1])      # left
    _take(c[:, :-1], f[:, :-1], f[:, 1:])     # right
    _take(c[1:], f[1:], f[:-1])               # above
    _take(c[:-1], f[:-1], f[1:])              # below: row rows - 1 never looks at row rows
    return c


def mask(frame, rows, threshold):
    """[rows][width] bool: the pixels refined, contrast > threshold."""
    return contrast(frame, rows) > threshold


def nearest_to(frame, rows, threshold):
    """How near the threshold the nearest contrast lies (what decides whether a mask may be demanded exactly)."""
    return float(np.abs(contrast(frame, rows) - threshold).min())


def positions(m, n):
    """The n * n sample positions (x + i / n, y + j / n) of the pixels of the mask m, pixels row-major, [pixel][j][i]: the
    rows radiance_reference.supersample_positions holds for them."""
    rows, width = m.shape
    return RR.supersample_positions(width, rows, n).reshape(rows * width, n * n, 2)[m.ravel()].reshape(-1, 2)


def refined(frame, m, samples):
    """The frame with every pixel of the mask m replaced by the mean of its samples: samples is [pixel][j * n + i][3] -- the
    listed pixels' in row-major order, or every pixel's of the rows, the [y][x][j][i] order of supersample_positions --
    summed one after the other in that order and divided once by n * n.  Everything else keeps its bytes."""
    out = np.array(frame, dtype=np.float64)
    rows, width = m.shape
    s = np.asarray(samples, dtype=np.float64)
    if s.shape[0] == rows * width and not m.all():
        s = s[m.ravel()]
    assert s.ndim == 3 and s.shape[0] == int(m.sum()) and s.shape[2] == 3, s.shape
    acc = s[:, 0].copy()
    for t in range(1, s.shape[1]):
        acc = acc + s[:, t]
    out[:rows][m] = acc / float(s.shape[1])
    return out


class Yardstick:
    """Oracle frames, masks and refined frames, each made once and shared (never written to)."""

    def __init__(self, pkg, O, orc):
        self.pkg, self.O, self.orc = pkg, O, orc
        self._scene, self._frame, self._refined = {}, {}, {}

    def scene(self, name):
        if name not in self._scene:
            self._scene[name] = (workloads.product_scene(self.pkg, name), workloads.oracle_scene(self.O, name))
        return self._scene[name]

    def eye(self, name):
        return self.scene(name)[1].c.camera.tup()

    def frame(self, name, w, h, depth, view=None):
        """The oracle's frame: orc_render, or -- view = (eye, basis) -- its cast_ray along the oriented context's pixel rays.
        Rows from rows_of(h) on are zero."""
        key = (name, w, h, depth, view)
        if key not in self._frame:
            oscene = self.scene(name)[1]
            if view is None:
                f = self.O.render(oscene, w, h, fov=workloads.FOV, max_depth=depth)
            else:
                rows = rows_of(h)
                d = RR.sample_directions(RR.pixel_positions(w, rows), self.orc.renderer(w, h), view[1])
                f = np.zeros((h, w, 3))
                f[:rows] = self.orc.cast(oscene, view[0], d, depth, normalize=True).reshape(rows, w, 3)
            f.setflags(write=False)
            self._frame[key] = f
        return self._frame[key]

    def refined(self, name, w, h, depth, n, threshold, view=None):
        """(mask, refined frame) of the oracle's frame."""
        key = (name, w, h, depth, n, threshold, view)
        if key not in self._refined:
            f = self.frame(name, w, h, depth, view)
            m = mask(f, rows_of(h), threshold)
            xy = positions(m, n)
            eye, basis = (self.eye(name), None) if view is None else view
            s = self.orc.cast(self.scene(name)[1], eye, RR.sample_directions(xy, self.orc.renderer(w, h), basis), depth, normalize=True)
            out = refined(f, m, s.reshape(-1, n * n, 3))
            m.setflags(write=False)
            out.setflags(write=False)
            self._refined[key] = (m, out)
        return self._refined[key]
