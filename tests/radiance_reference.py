"""The yardstick of the radiance queries' tests (include/rusty_marcher_amd.h, "radiance queries"): the oracle's own
orc_cast_ray(o, d, scene, background, 1, max_depth), driven for many rays -- each with an origin of its own -- by a few
lines of C compiled here, and the sample rays restated in numpy, operation for operation as the header states them.
No GPU, no product code: tests/test_radiance_abi.py pins this file to orc_backproject and orc_render on the CPU, and
asserts there that the ray sets below are not vacuous; tests/test_gpu_radiance.py holds the GPU to it."""
import ctypes as C
import os
import subprocess

import numpy as np

import test_gpu_query as GQ
import workloads

TIGHT = 1e-9                         # the project's render parity bound, per channel, no ray left out
N_RAYS = 4097                        # 64 waves and one: the last wave has one live lane
SEEDS = {"demo": 20261101, "cornell": 20261102, "synthetic256": 20261103, "panes": 20261104, "samples": 20261105}
BACKGROUND = (0.1, 0.1, 0.1)

RADIANCE_C = r"""
#include <pthread.h>
#include <stdint.h>
#include <stddef.h>
#include "rm_oracle.h"
typedef orc_vec3 (*cast_t)(orc_vec3, orc_vec3, const orc_scene *, orc_vec3, unsigned, unsigned);
typedef orc_vec3 (*norm_t)(orc_vec3);
typedef orc_vec3 (*bp_t)(const orc_renderer *, size_t, size_t);
typedef int (*fci_t)(orc_vec3, orc_vec3, const orc_shape *, size_t, orc_intersection *, uint8_t *);
typedef struct {
    cast_t cast; norm_t norm; fci_t fci; const orc_scene *s; const double *o, *d; int normalize; orc_vec3 bg; unsigned depth;
    double *rgb; int32_t *first, *shape;
    size_t begin, end;
} job_t;
static void *run(void *p) {
    job_t *j = (job_t *)p;
    for (size_t i = j->begin; i < j->end; i++) {
        const orc_vec3 o = {j->o[3 * i], j->o[3 * i + 1], j->o[3 * i + 2]};
        orc_vec3 d = {j->d[3 * i], j->d[3 * i + 1], j->d[3 * i + 2]};
        if (j->normalize) d = j->norm(d);
        const orc_vec3 c = j->cast(o, d, j->s, j->bg, 1, j->depth);
        j->rgb[3 * i] = c.x; j->rgb[3 * i + 1] = c.y; j->rgb[3 * i + 2] = c.z;
        if (j->first) {
            orc_intersection is;
            uint8_t sh = 0;
            const int h = j->fci(o, d, j->s->shapes, j->s->n_shapes, &is, &sh);
            j->first[i] = !h ? -1 : is.reflectance.is_glass_like ? 1 : 0;
            j->shape[i] = h ? (int32_t)sh : -1;
        }
    }
    return NULL;
}
/* rgb[i] = cast_ray(o[i], d[i] (normalize: orc_normalized(d[i])), scene, bg, 1, depth); first[i] (optional): -1 the ray leaves
   the scene, 1 its first hit is glass, 0 it is not, and shape[i]: -1 or the index of the first hit in Scene.shapes (wrapped to u8) */
void radiance_rays(cast_t cast, norm_t norm, fci_t fci, const orc_scene *s, size_t n, const double *o, const double *d, int normalize,
                   const double *bg, unsigned depth, double *rgb, int32_t *first, int32_t *shape, int n_threads) {
    pthread_t th[64];
    job_t jobs[64];
    if (n_threads < 1) n_threads = 1;
    if (n_threads > 64) n_threads = 64;
    const size_t per = (n + (size_t)n_threads - 1) / (size_t)n_threads;
    for (int t = 0; t < n_threads; t++) {
        job_t j = {cast, norm, fci, s, o, d, normalize, {bg[0], bg[1], bg[2]}, depth, rgb, first, shape, 0, 0};
        j.begin = per * (size_t)t < n ? per * (size_t)t : n;
        j.end = j.begin + per < n ? j.begin + per : n;
        jobs[t] = j;
        pthread_create(&th[t], NULL, run, &jobs[t]);
    }
    for (int t = 0; t < n_threads; t++) pthread_join(th[t], NULL);
}
void normalize_all(norm_t norm, size_t n, const double *d, double *out) {
    for (size_t i = 0; i < n; i++) {
        const orc_vec3 v = {d[3 * i], d[3 * i + 1], d[3 * i + 2]};
        const orc_vec3 u = norm(v);
        out[3 * i] = u.x; out[3 * i + 1] = u.y; out[3 * i + 2] = u.z;
    }
}
/* renderer.rs:128-135 for every pixel: out[y][x] = backproject(x, y) */
void backproject_all(bp_t bp, const orc_renderer *r, size_t w, size_t h, double *out) {
    for (size_t y = 0; y < h; y++)
        for (size_t x = 0; x < w; x++) {
            const orc_vec3 u = bp(r, x, y);
            double *q = out + 3 * (y * w + x);
            q[0] = u.x; q[1] = u.y; q[2] = u.z;
        }
}
"""


def compile_helper(O, entry, directory):
    src, so = directory / "orc_radiance.c", directory / "orc_radiance.so"
    src.write_text(RADIANCE_C)
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-shared", "-fPIC", "-pthread",
                           "-I", os.path.join(entry.ROOT, "oracle"), str(src), "-o", str(so)])
    return OracleRadiance(O, C.CDLL(str(so)))


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


class OracleRadiance:
    def __init__(self, O, L):
        self.O, self.OL, self.L = O, O.lib(), L
        P, V = C.POINTER, C.c_void_p
        L.radiance_rays.argtypes = [V, V, V, V, C.c_size_t, P(C.c_double), P(C.c_double), C.c_int, P(C.c_double), C.c_uint,
                                    P(C.c_double), P(C.c_int32), P(C.c_int32), C.c_int]
        L.normalize_all.argtypes = [V, C.c_size_t, P(C.c_double), P(C.c_double)]
        L.backproject_all.argtypes = [V, V, C.c_size_t, C.c_size_t, P(C.c_double)]
        self._cast = C.cast(self.OL.orc_cast_ray, V)
        self._norm = C.cast(self.OL.orc_normalized, V)
        self._fci = C.cast(self.OL.orc_find_closest_intersect, V)
        self._bp = C.cast(self.OL.orc_backproject, V)
        self.threads = max(1, min(16, len(os.sched_getaffinity(0))))

    def cast(self, oscene, o, d, depth, background=BACKGROUND, normalize=False, want_first=False):
        """orc_cast_ray along rays (o[i], d[i]) -- d taken as it is, or through orc_normalized first -> (N, 3) radiance
        (and, want_first, per ray -1 / 0 / 1: leaves the scene / first hit not glass / glass, and the shape first hit or -1)."""
        o = np.ascontiguousarray(np.broadcast_to(np.asarray(o, dtype=np.float64), np.shape(d)))
        d = np.ascontiguousarray(d, dtype=np.float64)
        n = d.shape[0]
        rgb = np.zeros((n, 3))
        first = np.zeros(n, np.int32) if want_first else None
        shape = np.zeros(n, np.int32) if want_first else None
        bg = np.ascontiguousarray(background, dtype=np.float64)
        self.L.radiance_rays(self._cast, self._norm, self._fci, C.cast(oscene.ptr, C.c_void_p), n, _p(o), _p(d), 1 if normalize else 0,
                             _p(bg), int(depth), _p(rgb), _p(first, C.c_int32), _p(shape, C.c_int32), self.threads)
        return (rgb, first, shape) if want_first else rgb

    def normalized(self, d):
        d = np.ascontiguousarray(d, dtype=np.float64).reshape(-1, 3)
        out = np.empty_like(d)
        self.L.normalize_all(self._norm, d.shape[0], _p(d), _p(out))
        return out

    def renderer(self, w, h, fov=workloads.FOV):
        """create_renderer(fov, height, width), renderer.rs:25-33"""
        return self.OL.orc_create_renderer(float(fov), float(h), float(w))

    def backproject(self, w, h, fov=workloads.FOV):
        r = self.renderer(w, h, fov)
        out = np.empty((h, w, 3))
        self.L.backproject_all(self._bp, C.cast(C.pointer(r), C.c_void_p), w, h, _p(out))
        return out


# ---------------------------------------------------------------- sample rays, as the header states them
FIXED_VIEW = ((1., 0., 0.), (0., 1., 0.), (0., 0., -1.))


def sample_directions(xy, r, basis=None):
    """Un-normalised direction of every sample (sx, sy) under the Renderer `r` (anything with width, height, half_fov and
    ratio: the oracle's orc_create_renderer, an rm_params): bx = 2 * (sx / width - 0.5) * half_fov * ratio,
    by = -2 * (sy / height - 0.5) * half_fov, z = -1, every operation rounded once in this order; under a basis (right, up,
    forward) per component (bx * right + by * up) + forward."""
    xy = np.asarray(xy, dtype=np.float64)
    width, height, half_fov, ratio = np.float64(r.width), np.float64(r.height), np.float64(r.half_fov), np.float64(r.ratio)
    bx = 2. * (xy[:, 0] / width - 0.5) * half_fov * ratio
    by = -2. * (xy[:, 1] / height - 0.5) * half_fov
    d = np.empty((xy.shape[0], 3))
    if basis is None:
        d[:, 0], d[:, 1], d[:, 2] = bx, by, -1.
    else:
        right, up, forward = basis
        for c in range(3):
            d[:, c] = (bx * right[c] + by * up[c]) + forward[c]
    return d


def pixel_positions(width, rows):
    """(sx, sy) of every integer pixel of the rows [0, rows), row-major."""
    y, x = np.mgrid[0:rows, 0:width]
    return np.stack([x.ravel(), y.ravel()], axis=1).astype(np.float64)


def supersample_positions(width, rows, n):
    """(x + i / n, y + j / n) for every pixel of the rows [0, rows): [y][x][j][i] pairs, as Renderer.render_supersampled orders them."""
    sub = np.arange(n, dtype=np.float64) / n
    xy = np.empty((rows, width, n, n, 2))
    xy[..., 0] = (np.arange(width, dtype=np.float64)[:, None] + sub[None, :])[None, :, None, :]
    xy[..., 1] = (np.arange(rows, dtype=np.float64)[:, None] + sub[None, :])[:, None, :, None]
    return xy.reshape(-1, 2)


def basis_tuple(b):
    """((x, y, z) of right, up, forward) of an rm_camera_basis."""
    return tuple((v.x, v.y, v.z) for v in (b.right, b.up, b.forward))


# ---------------------------------------------------------------- scenes and ray sets
def rays_for(name, desc, rng, n=N_RAYS):
    """n rays with origins in the padded bounds of the scene.  Half of them aim at a point of a random primitive (a point
    inside a sphere, on a polygon or a triangle), so most rays shade something; the demo's first quarter starts inside a sphere."""
    lo, hi = GQ.bounds_of(desc)
    o, d = GQ.random_rays(rng, n, lo, hi)
    targets = []
    for i in range(desc.n_spheres):
        s = desc.spheres[i]
        targets.append(("s", np.array([s.center.x, s.center.y, s.center.z]), np.sqrt(s.radius_square)))
    for i in range(desc.n_polygons):
        p = desc.polygons[i]
        targets.append(("p", np.array([[desc.polygon_vertices[p.first_vertex + k].x, desc.polygon_vertices[p.first_vertex + k].y,
                                        desc.polygon_vertices[p.first_vertex + k].z] for k in range(p.n_vertices)]), 0.))
    for i in range(desc.n_triangles):
        targets.append(("p", np.array([[v.x, v.y, v.z] for v in desc.triangles[i].vertices]), 0.))
    k = n // 2
    pick = rng.integers(0, len(targets), k)
    for j in range(k):
        kind, geom, r = targets[pick[j]]
        if kind == "s":
            aim = geom + GQ.unit(rng.normal(size=3)) * (0.8 * r * rng.uniform())
        else:
            aim = (geom * rng.dirichlet(np.ones(len(geom)))[:, None]).sum(axis=0)
        d[j] = GQ.unit(aim - o[j])
    if name == "demo":
        o[:n // 4] = GQ.inside_spheres(rng, desc, n // 4)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


GLASS = dict(diffusion=0.3, diffuse_color=(0.9, 0.8, 0.7), specular=0.9, specular_exponent=20.,
             is_glass_like=True, reflection=0.4, refractive_index=1.5)


def pane_stack(pkg, O):
    """A stack of 13 glass panes in front of a glass sphere (tests/test_gpu_parity.py test_deep_recursion_needs_the_stack):
    every pane adds a level and, at oblique incidence, a sibling.  -> (product Scene, oracle scene)"""
    panes = []
    for k in range(13):
        z = -4. - 1.25 * k
        tilt = 0.05 * k
        panes.append([(-12., -9., z - tilt), (12., -9., z + tilt), (12., 9., z + tilt), (-12., 9., z - tilt)])
    s, o = pkg.Scene.new(), O.OracleScene()
    R, Ro, V = pkg.Reflectance(**GLASS), O.reflectance(**GLASS), pkg.Vec3f
    for q in panes:
        s.shapes.append(pkg.polygon.ConvexPolygon.create([V(*p) for p in q], R))
        o.add_polygon(q, Ro)
    s.shapes.append(pkg.sphere.create(V(1.5, 0.5, -30.), 6., R))
    o.add_sphere((1.5, 0.5, -30.), 6., Ro)
    s.lights.append(pkg.create_light(V(0., 10., 0.), V(1., 1., 1.), 1.))
    o.add_light((0., 10., 0.), (1., 1., 1.), 1.)
    return s, o


def pane_rays(rng, n=1024):
    """n rays from in front of the stack through it, towards the sphere behind: up to 0.5 off the axis in x and y per unit of z."""
    o = np.column_stack([rng.uniform(-3., 3., n), rng.uniform(-3., 3., n), rng.uniform(-2., 0., n)])
    d = GQ.unit(np.column_stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n), -np.ones(n)]))
    return np.ascontiguousarray(o), np.ascontiguousarray(d)
