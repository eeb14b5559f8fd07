"""The yardstick of the diffuse bounce's tests (include/rusty_marcher_amd.h, "diffuse bounce"): rm_bounce_sequence and steps 1-3
of the rule restated in numpy, operation for operation as the header states them, and the bounce frame from the oracle alone.
No GPU, no product code.

Per lens ray (lens_reference.lens_rays', as every sampled frame's yardstick) a few lines of C compiled here against oracle/ run
orc_find_closest_intersect -- which says whether the sample bounces and gives P, N and the material -- then numpy forms the
bounce ray, and the same C casts it: orc_cast_ray(O', omega, moved scene, bg, 2, depth).  The lights are moved by
soft_reference.moved_scene, the fold is progressive_reference.accumulate.  tests/test_bounce_abi.py pins this file on the
library's sequence and on soft_reference and shows it is not vacuous; tests/test_gpu_bounce.py and
tests/test_gpu_converge_bounce.py hold the GPU to it."""
import ctypes as C
import os
import subprocess

import numpy as np

import lens_reference as LR
import progressive_reference as PR
import radiance_reference as RR
import soft_reference as SR

TIGHT = PR.TIGHT                     # the project's parity bound, per channel, no pixel left out
MAX_SAMPLES = PR.MAX_SAMPLES
FOUR_OVER_PI = 1.2732395447351628    # the header's literal
# Pixels of a 32 x 32 frame (aperture 0, point lights, strength 1, the library's sequences) whose mean with the bounce differs
# from the mean without by more than 0.05 in some channel, counted with the oracle alone (tests/test_bounce_abi.py):
# name -> (depth, rows, pixels)
BOUNCED = {"demo": (3, 16, 178), "cornell": (3, 16, 122), "penumbra": (3, 16, 367), "synthetic256": (6, 16, 109)}

BOUNCE_C = r"""
#include <pthread.h>
#include <stdint.h>
#include <stddef.h>
#include "rm_oracle.h"
typedef orc_vec3 (*cast_t)(orc_vec3, orc_vec3, const orc_scene *, orc_vec3, unsigned, unsigned);
typedef orc_vec3 (*norm_t)(orc_vec3);
typedef int (*fci_t)(orc_vec3, orc_vec3, const orc_shape *, size_t, orc_intersection *, uint8_t *);
typedef struct {
    cast_t cast; norm_t norm; fci_t fci; const orc_scene *s; const double *o, *d; orc_vec3 bg; unsigned recursion, depth;
    double *rgb, *dir, *surface; int32_t *kind;
    size_t begin, end;
} job_t;
static void *run(void *p) {
    job_t *j = (job_t *)p;
    for (size_t i = j->begin; i < j->end; i++) {
        const orc_vec3 o = {j->o[3 * i], j->o[3 * i + 1], j->o[3 * i + 2]};
        const orc_vec3 d = j->norm((orc_vec3){j->d[3 * i], j->d[3 * i + 1], j->d[3 * i + 2]});
        if (j->rgb) {
            const orc_vec3 c = j->cast(o, d, j->s, j->bg, j->recursion, j->depth);
            j->rgb[3 * i] = c.x; j->rgb[3 * i + 1] = c.y; j->rgb[3 * i + 2] = c.z;
        }
        if (j->kind) {
            orc_intersection is;
            const int h = j->fci(o, d, j->s->shapes, j->s->n_shapes, &is, NULL);
            double *q = j->surface + 10 * i;
            j->kind[i] = !h ? -1 : is.reflectance.is_glass_like ? 1 : 0;
            j->dir[3 * i] = d.x; j->dir[3 * i + 1] = d.y; j->dir[3 * i + 2] = d.z;
            if (h) {
                q[0] = is.point.x; q[1] = is.point.y; q[2] = is.point.z;
                q[3] = is.normal.x; q[4] = is.normal.y; q[5] = is.normal.z;
                q[6] = is.reflectance.diffusion;
                q[7] = is.reflectance.diffuse_color.x; q[8] = is.reflectance.diffuse_color.y; q[9] = is.reflectance.diffuse_color.z;
            }
        }
    }
    return NULL;
}
/* For every ray (o[i], orc_normalized(d[i])): rgb[i] (optional) = cast_ray(.., bg, recursion, depth); kind[i] (optional): -1 the
   ray leaves the scene, 1 its first hit is glass, 0 it is not -- then dir[i] is the normalised direction and surface[i] the
   hit's point, normal, diffusion and diffuse colour */
void bounce_rays(cast_t cast, norm_t norm, fci_t fci, const orc_scene *s, size_t n, const double *o, const double *d, const double *bg,
                 unsigned recursion, unsigned depth, double *rgb, int32_t *kind, double *dir, double *surface, int n_threads) {
    pthread_t th[64];
    job_t jobs[64];
    if (n_threads < 1) n_threads = 1;
    if (n_threads > 64) n_threads = 64;
    const size_t per = (n + (size_t)n_threads - 1) / (size_t)n_threads;
    for (int t = 0; t < n_threads; t++) {
        job_t j = {cast, norm, fci, s, o, d, {bg[0], bg[1], bg[2]}, recursion, depth, rgb, dir, surface, kind, 0, 0};
        j.begin = per * (size_t)t < n ? per * (size_t)t : n;
        j.end = j.begin + per < n ? j.begin + per : n;
        jobs[t] = j;
        pthread_create(&th[t], NULL, run, &jobs[t]);
    }
    for (int t = 0; t < n_threads; t++) pthread_join(th[t], NULL);
}
"""


def compile_helper(O, entry, directory):
    """As radiance_reference.compile_helper: the C above against oracle/rm_oracle.h -> an OracleBounce."""
    src, so = directory / "orc_bounce.c", directory / "orc_bounce.so"
    src.write_text(BOUNCE_C)
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-shared", "-fPIC", "-pthread",
                           "-I", os.path.join(entry.ROOT, "oracle"), str(src), "-o", str(so)])
    return OracleBounce(O, C.CDLL(str(so)))


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


class OracleBounce:
    def __init__(self, O, L):
        self.O, self.OL, self.L = O, O.lib(), L
        P, V = C.POINTER, C.c_void_p
        L.bounce_rays.argtypes = [V, V, V, V, C.c_size_t, P(C.c_double), P(C.c_double), P(C.c_double), C.c_uint, C.c_uint,
                                  P(C.c_double), P(C.c_int32), P(C.c_double), P(C.c_double), C.c_int]
        self._cast = C.cast(self.OL.orc_cast_ray, V)
        self._norm = C.cast(self.OL.orc_normalized, V)
        self._fci = C.cast(self.OL.orc_find_closest_intersect, V)
        self.threads = max(1, min(16, len(os.sched_getaffinity(0))))

    def _run(self, oscene, o, d, depth, recursion, background, want_rgb, want_hits):
        d = np.ascontiguousarray(d, dtype=np.float64)
        o = np.ascontiguousarray(np.broadcast_to(np.asarray(o, dtype=np.float64), d.shape))
        n = d.shape[0]
        rgb = np.zeros((n, 3)) if want_rgb else None
        kind = np.zeros(n, np.int32) if want_hits else None
        dirs = np.zeros((n, 3)) if want_hits else None
        surface = np.zeros((n, 10)) if want_hits else None
        bg = np.ascontiguousarray(background, dtype=np.float64)
        self.L.bounce_rays(self._cast, self._norm, self._fci, C.cast(oscene.ptr, C.c_void_p), n, _p(o), _p(d), _p(bg), int(recursion), int(depth),
                           _p(rgb), _p(kind, C.c_int32), _p(dirs), _p(surface), self.threads)
        return rgb, kind, dirs, surface

    def cast(self, oscene, o, d, depth, recursion=1, background=RR.BACKGROUND):
        """orc_cast_ray(o[i], orc_normalized(d[i]), scene, background, recursion, depth) -> (N, 3)"""
        return self._run(oscene, o, d, depth, recursion, background, True, False)[0]

    def first_hits(self, oscene, o, d):
        """orc_find_closest_intersect along (o[i], orc_normalized(d[i])) -> (kind: -1 / 0 / 1 leaves the scene / not glass / glass,
        the normalised directions, [point(3), normal(3), diffusion, diffuse_color(3)] of the hits)"""
        return self._run(oscene, o, d, 0, 1, RR.BACKGROUND, False, True)[1:]

    def renderer(self, w, h, fov=None):
        import workloads
        return self.OL.orc_create_renderer(float(workloads.FOV if fov is None else fov), float(h), float(w))


# ---------------------------------------------------------------- the sequence and steps 1-3, as the header states them
def bounce_sequence(first, count):
    """rm_bounce_sequence: rows first .. first + count - 1, (count, 2): (phi_19(s), phi_23(s))."""
    assert first >= 0 and count >= 0 and first + count <= MAX_SAMPLES
    t = np.empty((count, 2))
    for k in range(count):
        for c, base in enumerate((19, 23)):
            r, q = PR.digit_reversed(first + k, base)
            t[k, c] = np.float64(r) / np.float64(q)
    return t


def random_table(rng, n):
    """A bounce table that is not the library's: n points of [0, 1)^2."""
    return np.ascontiguousarray(rng.uniform(0., 1., (n, 2)))


def lowbias32(h):
    """The header's hash of a 32-bit word, on an array of uint32."""
    h = np.asarray(h, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x7feb352d)
        h ^= h >> np.uint32(15)
        h *= np.uint32(0x846ca68b)
        h ^= h >> np.uint32(16)
    return h


def shifted(t0, t1, pix, shift=True):
    """Step 1: the row's point moved by the pixel's own shift, wrapped into [0, 1).  shift = False: the step left out (the
    tests' counter-example)."""
    t0, t1 = np.asarray(t0, dtype=np.float64), np.asarray(t1, dtype=np.float64)
    if not shift:
        return np.full(np.shape(pix), t0), np.full(np.shape(pix), t1)
    h = lowbias32(pix)
    sx = (h & np.uint32(0xffff)).astype(np.float64) / 65536.
    sy = (h >> np.uint32(16)).astype(np.float64) / 65536.
    x = t0 + sx
    x = x - np.floor(x)
    y = t1 + sy
    y = y - np.floor(y)
    return x, y


def disc(x, y):
    """Step 2: (u, v, w, k) of the point (x, y) of [0, 1)^2."""
    a, b = 2. * x - 1., 2. * y - 1.
    sA, sB = np.sqrt(1. - a * a / 2.), np.sqrt(1. - b * b / 2.)
    u, v = a * sB, b * sA
    w = np.sqrt(np.fmax(1. - (u * u + v * v), 0.))
    k = FOUR_OVER_PI * (sA * sB - (a * a * b * b) / (4. * sA * sB))
    return u, v, w, k


def bounce_ray(P, N, dirs, u, v, w):
    """Step 3: (O', the un-normalised omega) for hits at P with normals N under rays of the normalised directions `dirs`; the
    oracle's own normalized() makes omega unit when the ray is cast."""
    facing = (dirs[:, 0] * N[:, 0] + dirs[:, 1] * N[:, 1]) + dirs[:, 2] * N[:, 2] < 0.       # orc_dot's order
    Nf = np.where(facing[:, None], N, -N)
    nx, ny, nz = Nf[:, 0], Nf[:, 1], Nf[:, 2]
    sg = np.where(nz < 0., -1., 1.)
    q = -1. / (sg + nz)
    c = nx * ny * q
    T = np.stack([1. + sg * nx * nx * q, sg * c, -sg * nx], axis=1)
    B = np.stack([c, sg + ny * ny * q, -ny], axis=1)
    omega = (T * u[:, None] + B * v[:, None]) + Nf * w[:, None]
    origin = P + Nf * 1e-3
    return origin, omega


# ---------------------------------------------------------------- frames
def samples(O, orb, oscene, eye, basis, width, height, depth, aperture, focus, table, offsets, bounce, strength, shift=True, nudge=None,
            pix_width=None):
    """The radiance of every lens ray of the rows a frame writes, row s shaded with the lights at offsets[s] and bounced by row
    s of `bounce`: [pixel][s][3], pixels row-major.  offsets None: the lights where they stand.  nudge: None, or a function
    omega -> omega' applied to the un-normalised bounce directions (the boundary check below).  pix_width: None, or a width
    other than the frame's to number the pixels by (the tests' counter-example: y * pix_width + x is hashed)."""
    rows = LR.rows_of(height)
    table, bounce = np.asarray(table, dtype=np.float64), np.asarray(bounce, dtype=np.float64)
    n = table.shape[0]
    assert bounce.shape == (n, 2) and (offsets is None or len(offsets) == n)
    strength = np.float64(strength)
    o, d = LR.lens_rays(width, rows, orb.renderer(width, height), eye, basis, aperture, focus, table)
    o, d = o.reshape(rows * width, n, 3), d.reshape(rows * width, n, 3)
    pix = np.arange(rows * width, dtype=np.uint32)                            # y * frame_width + x, row-major
    if pix_width is not None:
        pix = (pix // np.uint32(width)) * np.uint32(pix_width) + pix % np.uint32(width)
    out = np.empty((rows * width, n, 3))
    for s in range(n):
        scene = oscene if offsets is None else SR.moved_scene(O, oscene, offsets[s])
        os_, ds_ = np.ascontiguousarray(o[:, s]), np.ascontiguousarray(d[:, s])
        base = orb.cast(scene, os_, ds_, depth)
        out[:, s] = base
        if depth == 0 or strength == 0.:
            continue
        kind, dirs, surface = orb.first_hits(scene, os_, ds_)
        hit = np.flatnonzero(kind == 0)
        if hit.size == 0:
            continue
        x, y = shifted(bounce[s, 0], bounce[s, 1], pix[hit], shift)
        u, v, w, k = disc(x, y)
        origin, omega = bounce_ray(surface[hit, 0:3], surface[hit, 3:6], dirs[hit], u, v, w)
        if nudge is not None:
            omega = nudge(omega)
        back = orb.cast(scene, origin, omega, depth, recursion=2)
        wb = (strength * surface[hit, 6]) * k
        out[hit, s] = base[hit] + surface[hit, 7:10] * (back * wb[:, None])
    return out


def frames(O, orb, oscene, eye, basis, width, height, depth, aperture, focus, table, offsets, bounce, strength, passes, shift=True,
           pix_width=None):
    """progressive_reference.frames with the offset table and the bounce: (sum, mean) after the passes, each [height][width][3]."""
    rows = LR.rows_of(height)
    assert sum(passes) == np.asarray(table).shape[0]
    s = samples(O, orb, oscene, eye, basis, width, height, depth, aperture, focus, table, offsets, bounce, strength, shift, pix_width=pix_width)
    acc, mean, done = None, None, 0
    for n in passes:
        acc, mean = PR.accumulate(acc, s[:, done:done + n], done)
        done += n
    out_sum, out_mean = np.zeros((height, width, 3)), np.zeros((height, width, 3))
    out_sum[:rows], out_mean[:rows] = acc.reshape(rows, width, 3), mean.reshape(rows, width, 3)
    return out_sum, out_mean


def boundary_rays(O, orb, oscene, eye, basis, width, height, depth, aperture, focus, table, offsets, bounce, strength):
    """How many samples change by more than 1e-6 in some channel when every component of their bounce direction is moved one
    ulp up, or one ulp down: rays on a hit / miss boundary, which no bound on rounding covers.  0 for inputs fit for a parity test."""
    ref = samples(O, orb, oscene, eye, basis, width, height, depth, aperture, focus, table, offsets, bounce, strength)
    worst = np.zeros(ref.shape[:2], dtype=bool)
    for toward in (np.inf, -np.inf):
        moved = samples(O, orb, oscene, eye, basis, width, height, depth, aperture, focus, table, offsets, bounce, strength,
                        nudge=lambda w: np.nextafter(w, toward))
        worst |= (np.abs(moved - ref) > 1e-6).any(axis=2)
    return int(worst.sum())


# ---------------------------------------------------------------- the floor scene
# A flat floor under one light and nothing else (soft_reference's floor and its light overhead): every pixel that sees the floor
# shades the same material under the same light, so with ONE table row the only thing that tells two neighbouring pixels'
# bounces apart is the per-pixel shift.
def floor_scenes(pkg, O):
    """-> (product Scene, oracle scene), from soft_reference's recipe."""
    s, o = pkg.Scene.new(), O.OracleScene()
    V = pkg.Vec3f
    s.shapes.append(pkg.polygon.ConvexPolygon.create([V(*p) for p in SR.PENUMBRA_FLOOR], pkg.Reflectance(**SR.PENUMBRA_FLOOR_MATERIAL)))
    o.add_polygon(SR.PENUMBRA_FLOOR, O.reflectance(**SR.PENUMBRA_FLOOR_MATERIAL))
    pos, col, inten = SR.PENUMBRA_LIGHTS[0]
    s.lights.append(pkg.create_light(V(*pos), V(*col), inten))
    o.add_light(pos, col, inten)
    return s, o


class Yardstick(SR.Yardstick):
    """SR.Yardstick with reference bounce frames, each made once and shared (never written to).  orb: the OracleBounce."""

    def __init__(self, pkg, O, orc, orb):
        super().__init__(pkg, O, orc)
        self.orb = orb
        self._bounce = {}

    def scene(self, name):
        if name == "floor" and name not in self._scene:
            self._scene[name] = floor_scenes(self.pkg, self.O)
        return super().scene(name)

    def bounce(self, name, w, h, depth, aperture, focus, table, offsets, bounce, strength, passes, view=None, shift=True, pix_width=None):
        """(sum, mean) after the passes; offsets None: the lights where they stand."""
        t = np.ascontiguousarray(table, dtype=np.float64)
        f = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.float64)
        b = np.ascontiguousarray(bounce, dtype=np.float64)
        key = (name, w, h, depth, float(aperture), float(focus), t.tobytes(), None if f is None else f.tobytes(), b.tobytes(), float(strength),
               tuple(passes), view, shift, pix_width)
        if key not in self._bounce:
            eye, basis = (self.eye(name), None) if view is None else view
            pair = frames(self.O, self.orb, self.scene(name)[1], eye, basis, w, h, depth, aperture, focus, t, f, b, strength, passes, shift,
                          pix_width)
            for a in pair:
                a.setflags(write=False)
            self._bounce[key] = pair
        return self._bounce[key]

    def bounce_samples(self, name, w, h, depth, aperture, focus, table, offsets, bounce, strength, view=None):
        """[pixel][s][3] of every row of the tables (the converging frames' prefix sums are made of these)."""
        eye, basis = (self.eye(name), None) if view is None else view
        return samples(self.O, self.orb, self.scene(name)[1], eye, basis, w, h, depth, aperture, focus, table, offsets, bounce, strength)
