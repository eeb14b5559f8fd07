"""The yardstick of the variance-guided filter's tests (include/rusty_marcher_amd.h, "variance-guided filter"): the rule restated in
numpy, float64, operation for operation as the header states it.  No GPU, no product code.

The rule uses + - * / and comparisons alone, every one rounded once, and numpy's elementwise operations on float64 arrays are
exactly those; so the device is held to this file byte for byte.  One Python loop runs over the iterations, the 9 prefilter
taps and the 25 taps, and every sum is a whole-array left fold from +0. in tap order -- no np.sum or einsum over taps, whose
pairwise order is not the rule's.

tests/test_denoise_reference.py pins this file's own properties; tests/test_gpu_denoise.py holds the GPU to it."""
import numpy as np

H5 = (1. / 16., 1. / 4., 3. / 8., 1. / 4., 1. / 16.)                    # the 5-tap B3 spline, all exact in binary
K3 = (1. / 4., 1. / 2., 1. / 4.)

# numpy mirror of rm_hit (72 bytes)
HIT_DTYPE = np.dtype([("t", "<f8"), ("point", "<f8", 3), ("normal", "<f8", 3), ("shape", "<u4"), ("element", "<u4"), ("hit", "<i4"),
                      ("_pad", "<u4")])
assert HIT_DTYPE.itemsize == 72


class Control:
    """rm_denoise"""

    def __init__(self, sigma_l=4., sigma_z=.1, epsilon=1e-10, fallback_variance=1., iterations=5, normal_squarings=5):
        self.sigma_l, self.sigma_z, self.epsilon, self.fallback_variance = float(sigma_l), float(sigma_z), float(epsilon), float(fallback_variance)
        self.iterations, self.normal_squarings = int(iterations), int(normal_squarings)


def rows_of(h):
    return h - h % 32


def y_of(c):
    return (c[..., 0] + c[..., 1]) + c[..., 2]


def start(S, stats, n, fallback_variance):
    """C0 [rows][W][3], V0 [rows][W] of sum, (Y, Q) and count over the rows handed in."""
    nd = n.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        C0 = np.where((n > 0)[..., None], S / nd[..., None], 0.)
        Y, Q = stats[..., 0], stats[..., 1]
        m2 = Q - (Y * Y) / nd
        m2 = np.where(m2 < 0., 0., m2)
        V0 = np.where(n >= 2, m2 / (nd * (nd - 1.)), np.float64(fallback_variance))
    return C0, V0


def shifted(a, dy, dx, fill=0):
    """b[y, x] = a[y + dy, x + dx] where that is inside a, `fill` elsewhere; and the mask of where it is."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    inside = np.zeros((h, w), bool)
    y0, y1 = max(0, -dy), min(h, h - dy)
    x0, x1 = max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        inside[y0:y1, x0:x1] = True
    return b, inside


def prefilter(V):
    """g: the 3x3 prefilter of V, in-bounds taps only, normalised by the weights met."""
    sv, sk = np.zeros_like(V), np.zeros_like(V)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            k = K3[dx + 1] * K3[dy + 1]
            Vq, inside = shifted(V, dy, dx)
            sv = np.where(inside, sv + k * Vq, sv)
            sk = np.where(inside, sk + k, sk)
    return sv / sk


def iteration(C, V, n, hits, ctl, step):
    """One iteration with step `step` over C [rows][W][3], V, n [rows][W], hits [rows][W] of HIT_DTYPE or None -> (C', V')."""
    sl, sz_, eps = np.float64(ctl.sigma_l), np.float64(ctl.sigma_z), np.float64(ctl.epsilon)
    y = y_of(C)
    den = (sl * sl) * prefilter(V) + eps
    sw, sv = np.zeros_like(V), np.zeros_like(V)
    sc = np.zeros_like(C)
    have_p = n > 0
    if hits is not None:
        hit_p, shape_p = hits["hit"] != 0, hits["shape"]
        N_p, P_p, t_p = hits["normal"], hits["point"], hits["t"]
        sz = sz_ * (1. + t_p)
        dz = sz * sz
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                Cq, inside = shifted(C, step * dy, step * dx)
                Vq, _ = shifted(V, step * dy, step * dx)
                nq, _ = shifted(n, step * dy, step * dx)
                yq, _ = shifted(y, step * dy, step * dx)
                use = inside & (nq > 0)
                a = y - yq
                wl = np.where(have_p, den / (den + a * a), 1.)
                w = (H5[dx + 2] * H5[dy + 2]) * wl
                if hits is not None:
                    hq, _ = shifted(hits, step * dy, step * dx)
                    hit_q = hq["hit"] != 0
                    N_q, P_q = hq["normal"], hq["point"]
                    d = (N_p[..., 0] * N_q[..., 0] + N_p[..., 1] * N_q[..., 1]) + N_p[..., 2] * N_q[..., 2]
                    wn = d
                    for _ in range(ctl.normal_squarings):
                        wn = wn * wn
                    e = (N_p[..., 0] * (P_q[..., 0] - P_p[..., 0]) + N_p[..., 1] * (P_q[..., 1] - P_p[..., 1])) \
                        + N_p[..., 2] * (P_q[..., 2] - P_p[..., 2])
                    wz = dz / (dz + e * e)
                    both_hit, both_miss = hit_p & hit_q, ~hit_p & ~hit_q
                    admitted = both_miss | (both_hit & (shape_p == hq["shape"]) & (d > 0.))
                    use = use & admitted
                    w = np.where(both_miss, w, w * wn * wz)              # (both missed: wn = wz = 1.)
                sw = np.where(use, sw + w, sw)
                sc = np.where(use[..., None], sc + w[..., None] * Cq, sc)
                sv = np.where(use, sv + (w * w) * Vq, sv)
        some = sw > 0.
        C2 = np.where(some[..., None], sc / sw[..., None], C)
        V2 = np.where(some, sv / (sw * sw), V)
    return C2, V2


def to_bytes(mean):
    """The progressive frames' byte rule: (uint8_t)(255. * fmin(fmax(m, 0.), 1.)), a NaN -> 0."""
    with np.errstate(invalid="ignore"):
        m = np.where(np.isnan(mean), 0., mean)
        return (255. * np.minimum(np.maximum(m, 0.), 1.)).astype(np.uint8)


def denoise(S, stats, n, hits, ctl):
    """The filter over whole buffers [H][W][...] (hits: [H][W] of HIT_DTYPE, or None) -> (C [rows][W][3], V [rows][W],
    bytes [rows][W][3]) of the rows the filter writes, rows = H - H % 32."""
    rows = rows_of(S.shape[0])
    S, stats, n = np.asarray(S, np.float64)[:rows], np.asarray(stats, np.float64)[:rows], np.asarray(n, np.uint32)[:rows]
    hits = None if hits is None else np.asarray(hits)[:rows]
    C, V = start(S, stats, n, ctl.fallback_variance)
    for i in range(ctl.iterations):
        C, V = iteration(C, V, n, hits, ctl, 1 << i)
    return C, V, to_bytes(C)


def synthetic(seed, h, w, n_shapes=4):
    """A seeded frame with everything the rule branches on: counts 0, 1 and >= 2, hits and misses, `n_shapes` shape ids in
    patches with slowly varying normals and points, noise of very different size from pixel to pixel.
    -> (S [h][w][3], stats [h][w][2], n [h][w] uint32, hits [h][w] of HIT_DTYPE)"""
    r = np.random.default_rng(seed)
    n = r.integers(2, 40, size=(h, w)).astype(np.uint32)
    n[r.random((h, w)) < .06] = 0
    n[r.random((h, w)) < .06] = 1
    yy, xx = np.mgrid[0:h, 0:w]
    shape = ((xx // 11 + 2 * (yy // 9)) % n_shapes).astype(np.uint32)
    miss = ((xx + 2 * yy) % 29 < 5) | (r.random((h, w)) < .03)
    base = .15 + .2 * shape[..., None] + .05 * np.sin(xx / 7.)[..., None] * np.array([1., .5, .25])
    noise = r.normal(size=(h, w, 3)) * (.002 + .2 * r.random((h, w, 1)) ** 3)
    nd = np.maximum(n, 1).astype(np.float64)
    S = (base + noise) * nd[..., None]
    S[n == 0] = r.normal(size=(int((n == 0).sum()), 3))                  # (what a pixel without samples holds is not looked at)
    ymean = y_of(S) / nd
    spread = (.002 + .3 * r.random((h, w)) ** 2)
    stats = np.stack([ymean * nd, nd * (ymean * ymean) + spread * spread * nd * (.5 + r.random((h, w)))], axis=-1)
    stats[r.random((h, w)) < .02, 1] *= .5                               # (some m2 < 0: clamped)
    hits = np.zeros((h, w), HIT_DTYPE)
    normal = np.stack([.3 * np.sin(xx / 9. + shape), .3 * np.cos(yy / 8.), np.ones((h, w))], axis=-1) + .03 * r.normal(size=(h, w, 3))
    normal[(shape == 1) & (xx % 22 > 15)] *= -1.                         # (some neighbours of one shape face the other way: d <= 0)
    normal /= np.sqrt((normal * normal).sum(-1))[..., None]
    t = 4. + shape + .01 * xx + .02 * yy + .002 * r.normal(size=(h, w))
    hits["t"], hits["normal"] = t, normal
    hits["point"] = np.stack([(xx - w / 2.) * .01 * t, (yy - h / 2.) * .01 * t, -t], axis=-1)
    hits["shape"], hits["element"], hits["hit"] = shape, r.integers(0, 5, size=(h, w)), 1
    blank = np.zeros((), HIT_DTYPE)
    hits[miss] = blank                                                   # (every other field is 0 on a miss)
    return S, stats, n, hits
