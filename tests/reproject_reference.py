"""The yardstick of the temporal reprojection's tests (include/rusty_marcher_amd.h, "temporal reprojection"): the rule restated in
numpy, float64, operation for operation as the header states it.  No GPU, no product code.

The rule uses + - * /, floor, comparisons and integer-to-double conversions alone, every one rounded once, and numpy's elementwise
operations on float64 arrays are exactly those; so the device is held to this file byte for byte.  One Python loop runs over the
four taps, and every sum is a whole-array left fold from +0. in tap order.

tests/test_reproject_reference.py pins this file's own properties; tests/test_gpu_reproject.py holds the GPU to it."""
import numpy as np

from denoise_reference import HIT_DTYPE, rows_of

FIXED_BASIS = ((1., 0., 0.), (0., 1., 0.), (0., 0., -1.))


class Control:
    """rm_reproject"""

    def __init__(self, sigma_z=.1, min_normal_dot=.9, max_history=32):
        self.sigma_z, self.min_normal_dot, self.max_history = float(sigma_z), float(min_normal_dot), int(max_history)


class View:
    """rm_view: position and (right, up, forward)"""

    def __init__(self, position=(0., 0., 0.), basis=FIXED_BASIS):
        self.position = np.array(position, np.float64)
        self.right, self.up, self.forward = (np.array(v, np.float64) for v in basis)


class Frame:
    """What the rule reads of rm_params: the Renderer's four numbers"""

    def __init__(self, width, height, ratio, half_fov):
        self.width, self.height, self.ratio, self.half_fov = float(width), float(height), float(ratio), float(half_fov)

    @staticmethod
    def of(fov, height, width):
        """create_renderer(fov, height, width) (renderer.rs:25-33)"""
        return Frame(width, height, float(width) / float(height), np.tan(np.float64(fov) / 2.))


def dot3(v, a):
    """(v.x*a.x + v.y*a.y) + v.z*a.z"""
    return (v[..., 0] * a[..., 0] + v[..., 1] * a[..., 1]) + v[..., 2] * a[..., 2]


def sample_positions(cur_hits, view, frame, W, rows):
    """Steps a to d for every pixel -> (sx, sy, ok): ok where the pixel may carry something"""
    P = cur_hits["point"]
    with np.errstate(all="ignore"):
        v = P - view.position
        zf, xr, yu = dot3(v, view.forward), dot3(v, view.right), dot3(v, view.up)
        sx = (((xr / zf) / frame.ratio) / frame.half_fov / 2. + 0.5) * frame.width
        sy = (((yu / zf) / frame.half_fov) / -2. + 0.5) * frame.height
        ok = (cur_hits["hit"] != 0) & (zf > 0.)
        ok = ok & (sx > -1.) & (sx < np.float64(W)) & (sy > -1.) & (sy < np.float64(rows))
    return sx, sy, ok


def reproject(prev_S, prev_stats, prev_n, prev_hits, cur_hits, view, frame, ctl, taps_out=None):
    """The rule over whole buffers [H][W][...] -> (S [rows][W][3], stats [rows][W][2], n [rows][W] uint32, carried [rows][W] uint8)
    of the rows the call writes, rows = H - H % 32.  taps_out: optionally a list that receives the number of admitted taps a pixel."""
    rows, W = rows_of(prev_S.shape[0]), prev_S.shape[1]
    prev_S, prev_stats = np.asarray(prev_S, np.float64)[:rows], np.asarray(prev_stats, np.float64)[:rows]
    prev_n, prev_hits, cur_hits = np.asarray(prev_n).view(np.uint32)[:rows], np.asarray(prev_hits)[:rows], np.asarray(cur_hits)[:rows]
    sx, sy, ok = sample_positions(cur_hits, view, frame, W, rows)
    with np.errstate(all="ignore"):
        sx, sy = np.where(ok, sx, 0.), np.where(ok, sy, 0.)                  # (no conversion of what failed the check)
        fx0, fy0 = np.floor(sx), np.floor(sy)
        fx, fy = sx - fx0, sy - fy0
        x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
        N, P, t, shape = cur_hits["normal"], cur_hits["point"], cur_hits["t"], cur_hits["shape"]
        sz = np.float64(ctl.sigma_z) * (1. + t)
        dz = sz * sz
        sw, s1, s2 = np.zeros((rows, W)), np.zeros((rows, W)), np.zeros((rows, W))
        sc = np.zeros((rows, W, 3))
        nmin = np.full((rows, W), 0xffffffff, np.uint32)
        taps = np.zeros((rows, W), np.int64)
        for j in (0, 1):
            for i in (0, 1):
                wb = (fx if i else 1. - fx) * (fy if j else 1. - fy)
                qx, qy = x0 + i, y0 + j
                use = ok & (wb > 0.) & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < rows)
                cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, rows - 1)
                n_q, h_q = prev_n[cy, cx], prev_hits[cy, cx]
                use = use & (n_q != 0) & (h_q["hit"] != 0) & (h_q["shape"] == shape)
                d = dot3(N, h_q["normal"])
                use = use & (d > np.float64(ctl.min_normal_dot))
                Pq = h_q["point"]
                e = (N[..., 0] * (Pq[..., 0] - P[..., 0]) + N[..., 1] * (Pq[..., 1] - P[..., 1])) + N[..., 2] * (Pq[..., 2] - P[..., 2])
                use = use & (e * e <= dz)
                nq = n_q.astype(np.float64)
                sw = np.where(use, sw + wb, sw)
                sc = np.where(use[..., None], sc + wb[..., None] * (prev_S[cy, cx] / nq[..., None]), sc)
                s1 = np.where(use, s1 + wb * (prev_stats[cy, cx, 0] / nq), s1)
                s2 = np.where(use, s2 + wb * (prev_stats[cy, cx, 1] / nq), s2)
                nmin = np.where(use, np.minimum(nmin, n_q), nmin)
                taps += use
        carried = sw > 0.
        n = np.where(carried, np.minimum(nmin, np.uint32(ctl.max_history)), 0).astype(np.uint32)
        nd = n.astype(np.float64)
        S = np.where(carried[..., None], (sc / sw[..., None]) * nd[..., None], 0.)
        stats = np.where(carried[..., None], (np.stack([s1, s2], axis=-1) / sw[..., None]) * nd[..., None], 0.)
    if taps_out is not None:
        taps_out.append(taps)
    return S, stats, n, carried.astype(np.uint8)


def plane_hits(view, frame, h, w, depth, shape_of):
    """The hits a view has of the plane `depth` in front of it along its forward, facing it: pixel (x, y) sees the point
    E + depth (bx R + by U + F) with the radiance section's bx and by -- for power-of-two numbers every coordinate is exact.
    shape_of(P) -> the shape ids of points [h][w][3].  -> [h][w] of HIT_DTYPE"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    bx = 2. * (xx / frame.width - 0.5) * frame.half_fov * frame.ratio
    by = -2. * (yy / frame.height - 0.5) * frame.half_fov
    D = bx[..., None] * view.right + by[..., None] * view.up + view.forward
    hits = np.zeros((h, w), HIT_DTYPE)
    hits["point"] = view.position + depth * D
    hits["t"] = depth * np.sqrt((D * D).sum(-1))
    hits["normal"] = -view.forward
    hits["shape"], hits["hit"] = shape_of(hits["point"]), 1
    return hits
