"""The ranged ray queries restated in numpy (include/rusty_marcher_amd.h, "ranged ray queries"): the CPU yardstick of
tests/test_gpu_ranged_queries.py, itself pinned to the oracle by tests/test_ranged_abi.py.

float64 throughout, one numpy operation per rounding, in the reference's order (numpy evaluates a * b + c * d as two
products and a sum: nothing is fused).  Each primitive offers the candidates the reference forms -- a sphere its two
roots (sphere.rs:43-45), a polygon or triangle its one dist (polygon.rs:71-76, triangle.rs:62-67) -- and the closed range
[t_min, t_max] decides which are accepted; accepted candidates are ordered by |p - o|^2 (shapes.rs:128), exact ties
going to the first in list order.  Built from an rm_scene_desc (scene.flatten().desc()); vectorised over the rays, a
Python loop over the primitives in list order."""
import numpy as np

NEAR = 1e-9     # a candidate this close (relative) to an end of its range marks the ray `near_end`


def _v(v):
    return np.array([v.x, v.y, v.z], dtype=np.float64)


def dot(a, b):
    """geometry.rs:180-182: (x x' + y y') + z z'"""
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def normalized(a):
    """geometry.rs:104-109: sqrt, the reciprocal of the rounded norm, three products -> (unit vector, norm)"""
    norm = np.sqrt(dot(a, a))
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(norm > 0., 1. / norm, 1.)
    return a * inv[..., None], norm


def in_range(t, lo, hi):
    """closed; not-a-number lies in every range, as it passes the reference's `t < 0`"""
    return ~(t < lo) & ~(t > hi)


class Scene:
    """The primitives of an rm_scene_desc in list order: (kind, shape index, element, data)."""

    def __init__(self, desc):
        self.prims = []
        for si in range(desc.n_shapes):
            sh = desc.shapes[si]
            if sh.kind == 0:
                s = desc.spheres[sh.first]
                self.prims.append(("sphere", si, 0, (_v(s.center), float(s.radius_square))))
            elif sh.kind == 1:
                p = desc.polygons[sh.first]
                verts = np.array([_v(desc.polygon_vertices[p.first_vertex + k]) for k in range(p.n_vertices)])
                self.prims.append(("planar", si, 0, (_v(p.plane_normal), _v(p.plane_point), verts, None)))
            else:
                for e in range(sh.count):
                    t = desc.triangles[sh.first + e]
                    verts = np.array([_v(v) for v in t.vertices])
                    self.prims.append(("planar", si, e, (_v(t.normal), _v(t.center), verts, 1e-6)))
        self.lights = np.array([_v(desc.lights[i].position) for i in range(desc.n_lights)]).reshape(-1, 3)

    # ---- candidates ----
    @staticmethod
    def _sphere(data, o, d):
        """-> (inside the silhouette, t0, t1)"""
        c, r2 = data
        line = c - o
        tca = dot(line, d)
        d2 = dot(line, line) - tca * tca
        alive = ~(d2 > r2)                                              # sphere.rs:37
        with np.errstate(invalid="ignore"):
            thc = np.sqrt(r2 - d2)
        return alive, tca - thc, tca + thc

    @staticmethod
    def _planar(data, o, d):
        """-> (plane met in front and inside every edge, dist)"""
        n, pp, verts, eps = data
        dotprod = dot(d, n)
        alive = ~(np.abs(dotprod) < eps) if eps is not None else ~(dotprod == 0.)      # triangle.rs:57 / polygon.rs:66
        with np.errstate(divide="ignore", invalid="ignore"):
            dist = dot(pp - o, n) / dotprod
        with np.errstate(all="ignore"):
            alive &= ~(dist < 0.)
            p = o + d * dist[:, None]
            k = len(verts)
            for i in range(k):                                          # polygon.rs:54-56: z of (v_i - p) x (v_i+1 - p)
                a, b = verts[i] - p, verts[(i + 1) % k] - p
                alive &= (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]) > 0.
        return alive, dist

    def _accepted(self, o, d, lo, hi):
        """For every primitive in list order: (kind, shape, element, data, accepted, t, near_end)."""
        def near(t, ok):
            with np.errstate(all="ignore"):
                e = np.abs(t - lo) <= NEAR * np.abs(lo)
                e |= np.isfinite(hi) & (np.abs(t - hi) <= NEAR * np.abs(hi))
            return ok & e

        for kind, si, el, data in self.prims:
            if kind == "sphere":
                alive, t0, t1 = self._sphere(data, o, d)
                first = in_range(t0, lo, hi)
                t = np.where(first, t0, t1)
                yield kind, si, el, data, alive & (first | in_range(t1, lo, hi)), t, near(t0, alive) | near(t1, alive)
            else:
                alive, dist = self._planar(data, o, d)
                yield kind, si, el, data, alive & in_range(dist, lo, hi), dist, near(dist, alive)

    # ---- the queries ----
    def closest(self, o, d, ranges):
        """-> dict of hit (int32), shape, element (int64; -1 on a miss), t, point, normal, near_end (bool)"""
        o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
        lo, hi = _lo_hi(ranges, len(o))
        n = len(o)
        hit = np.zeros(n, bool)
        best = np.zeros(n)
        out = dict(shape=np.full(n, -1, np.int64), element=np.full(n, -1, np.int64), t=np.zeros(n), point=np.zeros((n, 3)),
                   normal=np.zeros((n, 3)), near_end=np.zeros(n, bool))
        for kind, si, el, data, ok, t, near in self._accepted(o, d, lo, hi):
            out["near_end"] |= near
            with np.errstate(all="ignore"):                             # (a far root may be inf or nan where nothing is accepted)
                p = o + d * t[:, None]
                dp = p - o
                dist = dot(dp, dp)                                      # shapes.rs:128
                take = ok & (~hit | (dist < best))                      # shapes.rs:130 / obj.rs:198: strict, first wins
            if not take.any():
                continue
            best[take] = dist[take]
            hit |= take
            out["shape"][take], out["element"][take], out["t"][take] = si, el, t[take]
            out["point"][take] = p[take]
            if kind == "sphere":
                out["normal"][take] = normalized(p[take] - data[0])[0]  # sphere.rs:58
            else:
                out["normal"][take] = data[0]
        out["hit"] = hit.astype(np.int32)
        return out

    def occluded(self, o, d, ranges):
        """-> (occluded, near_end)"""
        o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
        lo, hi = _lo_hi(ranges, len(o))
        occ, near_end = np.zeros(len(o), bool), np.zeros(len(o), bool)
        for _, _, _, _, ok, _, near in self._accepted(o, d, lo, hi):
            occ |= ok
            near_end |= near
        return occ, near_end

    def visible(self, a, b, skin):
        """rm_visible_segments -> (visible, near_end)"""
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        d, length = normalized(b - a)
        lo, hi = np.full(len(a), float(skin)), length - skin
        empty = hi < lo
        occ, near = self.occluded(a, d, np.stack([lo, hi], axis=1))
        return empty | ~occ, near & ~empty

    def shadow_rays(self, points, normals):
        """renderer.rs:166-172 for every (point, light): origins and directions (N, n_lights, 3), norms (N, n_lights)"""
        p, n = np.asarray(points, np.float64)[:, None, :], np.asarray(normals, np.float64)[:, None, :]
        d, norm = normalized(self.lights[None, :, :] - p)
        side = np.where(dot(d, n) < 0., -1e-3, 1e-3)
        return p + n * side[..., None], d, norm

    def lights_visible(self, points, normals, clipped):
        """rm_lights_visible -> (lit (N, n_lights), near_end)"""
        o, d, norm = self.shadow_rays(points, normals)
        shape = norm.shape
        hi = norm.reshape(-1) if clipped else np.full(norm.size, np.inf)
        occ, near = self.occluded(o.reshape(-1, 3), d.reshape(-1, 3), np.stack([np.zeros(norm.size), hi], axis=1))
        return ~occ.reshape(shape), near.reshape(shape)


def _lo_hi(ranges, n):
    r = np.asarray(ranges, np.float64)
    if r.shape == (2,):
        r = np.broadcast_to(r, (n, 2))
    assert r.shape == (n, 2)
    return r[:, 0].copy(), r[:, 1].copy()
