"""The yardstick of the diffuse bounce's tests (include/rusty_marcher_amd.h, "diffuse bounce"): rm_bounce_sequence and steps 1-3
of the rule restated in numpy, operation for operation as the header states them, and the bounce frame from the oracle alone.
No GPU, no product code.

Per lens ray (lens_reference.lens_rays', as every sampled frame's yardstick) a few lines of C compiled here against oracle/ run
orc_find_closest_intersect -- which says whether the sample bounces and gives P, N and the material -- then numpy forms the
bounce ray, and the same C casts it: orc_cast_ray(O', omega, moved scene, bg, 2, depth).  The lights are moved by
soft_reference.moved_scene, the fold is progressive_reference.accumulate.  tests/test_bounce_abi.py pins this file on the
library's sequence and on soft_reference and shows it is not vacuous; tests/test_gpu_bounce.py and
tests/test_gpu_converge_bounce.py hold the GPU to it.

counters() says what a parity input exercises of steps 2 and 3 -- surfaces met from behind, the two halves and the poles of the
basis, the edges of the square where only the clamp keeps the square root from NaN -- and VIEWS, the screens scene and
edge_table are inputs made to exercise them; every case that uses them asserts its counters first."""
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


def disc_unclamped(x, y):
    """Step 2 up to its clamp: (u, v, the radicand 1 - (u u + v v) as it rounds -- below zero at some points of the square's
    edges --, k) of the point (x, y) of [0, 1)^2."""
    a, b = 2. * x - 1., 2. * y - 1.
    sA, sB = np.sqrt(1. - a * a / 2.), np.sqrt(1. - b * b / 2.)
    u, v = a * sB, b * sA
    k = FOUR_OVER_PI * (sA * sB - (a * a * b * b) / (4. * sA * sB))
    return u, v, 1. - (u * u + v * v), k


def disc(x, y):
    """Step 2: (u, v, w, k) of the point (x, y) of [0, 1)^2."""
    u, v, r, k = disc_unclamped(x, y)
    return u, v, np.sqrt(np.fmax(r, 0.)), k


def facing_normals(N, dirs):
    """Step 3's first line: (front: the ray meets the side N points to, Nf: N there and -N elsewhere)."""
    front = (dirs[:, 0] * N[:, 0] + dirs[:, 1] * N[:, 1]) + dirs[:, 2] * N[:, 2] < 0.        # orc_dot's order
    return front, np.where(front[:, None], N, -N)


def bounce_ray(P, N, dirs, u, v, w):
    """Step 3: (O', the un-normalised omega) for hits at P with normals N under rays of the normalised directions `dirs`; the
    oracle's own normalized() makes omega unit when the ray is cast."""
    _, Nf = facing_normals(N, dirs)
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


ONE_BELOW = 1. - 2. ** -53                # the last double of [0, 1): the far edge of the square
COUNTERS = ("bouncing", "front", "back", "below", "steep", "min_z", "max_z", "pole_up", "pole_down", "negative", "min_radicand",
            "x_lo", "x_hi", "y_lo", "y_hi", "edge", "corner")


def bouncing_pixels(orb, oscene, eye, basis, width, height, aperture, focus, table):
    """[pixel][s]: the sample bounces -- its lens ray's first hit is not glass (the lights do not enter: offsets move only them)."""
    rows = LR.rows_of(height)
    n = np.asarray(table).shape[0]
    o, d = LR.lens_rays(width, rows, orb.renderer(width, height), eye, basis, aperture, focus, table)
    o, d = o.reshape(rows * width, n, 3), d.reshape(rows * width, n, 3)
    return np.stack([orb.first_hits(oscene, np.ascontiguousarray(o[:, s]), np.ascontiguousarray(d[:, s]))[0] == 0 for s in range(n)], axis=1)


def counters(O, orb, oscene, eye, basis, width, height, depth, aperture, focus, table, offsets, bounce, strength, shift=True):
    """What the bouncing samples of samples(the same arguments) exercise of steps 2 and 3, from the oracle alone -> a dict:
    bouncing   the samples that bounce;
    front, back   those whose facing normal is N, and -N (the ray met the surface from behind);
    below      those with Nf.z < 0 (the sg = -1 half of the basis), steep: with Nf.z < -0.5; min_z, max_z: the extremes of Nf.z;
    pole_up, pole_down   those with Nf exactly (0, 0, 1) and exactly (0, 0, -1);
    negative   those whose radicand 1 - (u u + v v) is below zero before step 2's clamp; min_radicand: the lowest;
    x_lo, x_hi, y_lo, y_hi   those with x == 0, x == 1 - 2^-53, y == 0, y == 1 - 2^-53; edge: on any of the four; corner: on two."""
    rows = LR.rows_of(height)
    table, bounce = np.asarray(table, dtype=np.float64), np.asarray(bounce, dtype=np.float64)
    n = table.shape[0]
    assert bounce.shape == (n, 2) and (offsets is None or len(offsets) == n)
    c = dict.fromkeys(COUNTERS, 0)
    c["min_z"], c["max_z"], c["min_radicand"] = np.inf, -np.inf, np.inf
    if depth == 0 or np.float64(strength) == 0.:
        return c
    o, d = LR.lens_rays(width, rows, orb.renderer(width, height), eye, basis, aperture, focus, table)
    o, d = o.reshape(rows * width, n, 3), d.reshape(rows * width, n, 3)
    pix = np.arange(rows * width, dtype=np.uint32)
    for s in range(n):
        scene = oscene if offsets is None else SR.moved_scene(O, oscene, offsets[s])
        kind, dirs, surface = orb.first_hits(scene, np.ascontiguousarray(o[:, s]), np.ascontiguousarray(d[:, s]))
        hit = np.flatnonzero(kind == 0)
        if hit.size == 0:
            continue
        x, y = shifted(bounce[s, 0], bounce[s, 1], pix[hit], shift)
        radicand = disc_unclamped(x, y)[2]
        front, Nf = facing_normals(surface[hit, 3:6], dirs[hit])
        on = np.stack([x == 0., x == ONE_BELOW, y == 0., y == ONE_BELOW])
        for key, count in (("bouncing", hit.size), ("front", front.sum()), ("back", (~front).sum()), ("below", (Nf[:, 2] < 0.).sum()), ("steep", (Nf[:, 2] < -0.5).sum()),
                           ("pole_up", (Nf == (0., 0., 1.)).all(axis=1).sum()), ("pole_down", (Nf == (0., 0., -1.)).all(axis=1).sum()),
                           ("negative", (radicand < 0.).sum()), ("x_lo", on[0].sum()), ("x_hi", on[1].sum()), ("y_lo", on[2].sum()),
                           ("y_hi", on[3].sum()), ("edge", on.any(axis=0).sum()), ("corner", (on.sum(axis=0) == 2).sum())):
            c[key] += int(count)
        c["min_z"], c["max_z"] = min(c["min_z"], float(Nf[:, 2].min())), max(c["max_z"], float(Nf[:, 2].max()))
        c["min_radicand"] = min(c["min_radicand"], float(radicand.min()))
    return c


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


# ---------------------------------------------------------------- the screens scene
# Two screens in the plane z = -12 (planes perpendicular to z are the only axis-aligned ones the reference's xy inside-test can
# hit), so their normal is (0, 0, 1) exactly: seen from the fixed view the facing normal is the basis's +z pole (q = -1/2), seen
# from behind it is -N = (0, 0, -1), the other half's pole (sg = -1, q = 1/2).  A diffuse sphere before the gap between them and
# a glass one behind it give the bounce rays something to bring back from either side; a light stands on either side.
SCREENS = [[(-8., -6., -12.), (-1., -6., -12.), (-1., 6., -12.), (-8., 6., -12.)], [(1., -6., -12.), (8., -6., -12.), (8., 6., -12.), (1., 6., -12.)]]
SCREENS_DIFFUSE = ((0., -1., -7.), 1.5, dict(diffusion=0.8, diffuse_color=(0.9, 0.3, 0.2), specular=0.5, specular_exponent=20.,
                                             is_glass_like=False, reflection=0., refractive_index=1.))
SCREENS_GLASS = ((0., 1., -17.), 1.5)
SCREENS_LIGHTS = [((0., 5., -3.), (1., 1., 1.), 1.), ((0., 5., -21.), (1., 0.7, 0.5), 0.8)]


def screens_scenes(pkg, O):
    """-> (product Scene, oracle scene), from the one recipe above."""
    s, o = pkg.Scene.new(), O.OracleScene()
    V = pkg.Vec3f
    for q in SCREENS:
        s.shapes.append(pkg.polygon.ConvexPolygon.create([V(*p) for p in q], pkg.Reflectance(**SR.PENUMBRA_FLOOR_MATERIAL)))
        o.add_polygon(q, O.reflectance(**SR.PENUMBRA_FLOOR_MATERIAL))
    for centre, radius, material in (SCREENS_DIFFUSE, SCREENS_GLASS + (RR.GLASS,)):
        s.shapes.append(pkg.sphere.create(V(*centre), radius, pkg.Reflectance(**material)))
        o.add_sphere(centre, radius, O.reflectance(**material))
    for pos, col, inten in SCREENS_LIGHTS:
        s.lights.append(pkg.create_light(V(*pos), V(*col), inten))
        o.add_light(pos, col, inten)
    return s, o


# ---------------------------------------------------------------- views from every side
# name -> (scene, max_depth, f(c, R, e) -> (eye, target, up hint)): c the centre, R the diagonal and e the extent of the scene's
# padded bounds (test_gpu_query.bounds_of); f None: the fixed view, from the scene's camera down -z, with `target` only for the focus.
# tests/test_bounce_abi.py pins each view's counters in COVERAGE and that none has a sample on a hit / miss boundary;
# tests/test_gpu_bounce.py holds the GPU to the yardstick under each.
UP = (0., 1., 0.)
VIEWS = {
    # the box from behind (the padded bounds are half as wide again as the box: 0.2 R stands just outside it): the faces the
    # fixed view meets from the front are met from behind
    "cornell-behind": ("cornell", 3, lambda c, R, e: (c + np.array([0., 0.1, -1.]) * 0.2 * R, c, UP)),
    # from inside the box, below and before its middle, towards +z: every sample bounces, every one from a back face
    "cornell-inside": ("cornell", 3, lambda c, R, e: (c + np.array([0., -0.13, 0.03]) * e, c + np.array([0., -0.13, 0.03]) * e + np.array([0.05, 0.03, 1.]), UP)),
    # from below: front and back faces in one frame, so in one wave
    "cornell-below": ("cornell", 3, lambda c, R, e: (c + np.array([0.1, -1., 0.1]) * 0.25 * R, c, (0., 0., -1.))),
    # the demo's spheres from behind: facing normals about the -z pole
    "demo-behind": ("demo", 3, lambda c, R, e: (c + np.array([0., 0.1, -1.]) * 0.25 * R, c, UP)),
    "screens-fixed": ("screens", 3, None),
    "floor-fixed": ("floor", 3, None),                                 # (for the edge rows alone: no condition in REQUIRED)
    "screens-behind": ("screens", 3, lambda c, R, e: (np.array([0., 0., -24.]), np.array([0., 0., -12.]), UP)),
    # ... and from the side: the facing normal is still (0, 0, -1), the rays arrive obliquely
    "screens-oblique": ("screens", 3, lambda c, R, e: (np.array([7., 2., -23.]), np.array([0., 0., -12.]), UP)),
}
FIXED_TARGET = {"screens": (0., 0., -12.), "floor": (0., 0., -LR.FOCUS)}
# What a view is there for: the least of each counter (min_z: the most) its parity case demands of its own inputs before it
# compares anything -- a view that stops exercising its branch fails instead of passing vacuously
REQUIRED = {
    "cornell-behind": dict(back=1000),
    "cornell-inside": dict(bouncing=5120, back=5120),                  # every sample of the frame
    "cornell-below": dict(back=100, front=500),
    "demo-behind": dict(steep=50, min_z=-0.99),
    "screens-fixed": dict(pole_up=500),
    "screens-behind": dict(pole_down=500),
    "screens-oblique": dict(pole_down=500),
}
# ... and what the oracle alone counts at the parity cases' inputs (32 x 32, 5 lens rows from row 3, aperture 0; the counters do
# not depend on the bounce table), pinned by tests/test_bounce_abi.py: (bouncing, back, below, steep, pole_up, pole_down)
COVERAGE = {
    "cornell-behind": (1099, 1099, 1099, 874, 0, 0),
    "cornell-inside": (5120, 5120, 5120, 2047, 0, 0),
    "cornell-below": (1801, 1116, 1116, 614, 0, 0),
    "demo-behind": (166, 7, 165, 133, 0, 0),
    "screens-fixed": (1850, 0, 0, 0, 1622, 0),
    "screens-behind": (1638, 1621, 1638, 1636, 0, 1621),
    "screens-oblique": (1439, 1439, 1439, 1439, 0, 1439),
}
# The five fixed-view inputs the suite had before the views: no sample of theirs meets a surface from behind
FIXED_COVERAGE = {
    "demo": (836, 0, 21, 0, 0, 0), "cornell": (611, 0, 0, 0, 0, 0), "synthetic256": (453, 0, 25, 0, 0, 0),
    "penumbra": (1876, 0, 0, 0, 0, 0), "floor": (2089, 0, 0, 0, 0, 0),
}
PINNED = ("bouncing", "back", "below", "steep", "pole_up", "pole_down")
# the views under which the converging call is held to the plain run and the yardstick (tests/test_gpu_converge_bounce.py: the
# library's rows 0 .. 14)
CONVERGING_VIEWS = ("cornell-inside", "screens-behind")


def assert_covers(name, c):
    """The view's conditions of REQUIRED on the counters `c` of its inputs."""
    for key, least in REQUIRED[name].items():
        if key == "min_z":
            assert c["min_z"] <= least, "%s: the lowest Nf.z is %g, not below %g" % (name, c["min_z"], least)
        else:
            assert c[key] >= least, "%s: %d samples count as `%s`, fewer than %d" % (name, c[key], key, least)


def look_from(name, lo, hi):
    """(scene, depth, eye or None for the scene's camera, target, up hint) of the view `name` of a scene with the bounds lo, hi."""
    scene, depth, f = VIEWS[name]
    if f is None:
        return scene, depth, None, FIXED_TARGET[scene], UP
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    eye, target, up = f((lo + hi) / 2., float(np.linalg.norm(hi - lo)), hi - lo)
    return scene, depth, tuple(float(v) for v in eye), tuple(float(v) for v in target), up


def view_tables(name, first, n):
    """The two bounce tables a view's parity case runs: the library's rows from `first` on and a seeded random table."""
    seed = 20262200 + sorted(VIEWS).index(name)
    return (("sequence", bounce_sequence(first, n)), ("random", random_table(np.random.default_rng(seed), n)))


# ---------------------------------------------------------------- the edges of the square
EDGES = ("x_lo", "x_hi", "y_lo", "y_hi")
CORNERS = tuple(a + "+" + b for a in EDGES[:2] for b in EDGES[2:])


# the rows of the edge cases (tests/test_gpu_bounce.py; pinned by tests/test_bounce_abi.py): every edge four times, every corner twice
EDGE_KINDS = EDGES * 4 + CORNERS * 2
EDGE_VIEWS = ("floor-fixed", "screens-behind", "cornell-inside")
EDGE_SEED = 20262300


def assert_edges(c):
    """What an edge case demands of its inputs' counters: 16 samples on an edge, 8 with a radicand below zero, every edge and
    two corners."""
    assert c["edge"] >= 16 and c["negative"] >= 8 and c["corner"] >= 2, c
    assert min(c[e] for e in EDGES) >= 1, c


def edge_coordinate(shift16, far):
    """The table entry t of [0, 1) with which a pixel whose shift is shift16 / 65536 lands on 0 exactly (far False) or on
    1 - 2^-53 (far True) behind step 1's wrap; None where the sum rounds to 1 and so wraps to 0."""
    s = np.float64(shift16) / 65536.
    t = (1. - s) % 1.                                                  # exact: a multiple of 2^-16
    if far:
        t = np.nextafter(t, 0.) if t > 0. else ONE_BELOW
    x = t + s
    x = x - np.floor(x)
    return float(t) if x == (ONE_BELOW if far else 0.) and 0. <= t < 1. else None


def edge_table(rng, bouncing, kinds):
    """A bounce table whose row s puts sample s of one pixel that bounces there on an edge or a corner of the square.
    bouncing: [pixel][s] (bouncing_pixels), kinds: one of EDGES or CORNERS a row; the free coordinate of an edge row is
    searched in `rng`'s stream until the radicand at the target is below zero (about one candidate in seven at x == 0).
    -> (the table, the target pixel of every row)."""
    n = len(kinds)
    assert bouncing.shape[1] == n <= 64
    out, targets = random_table(rng, n), []
    for s, kind in enumerate(kinds):
        want = kind.split("+")
        for p in rng.permutation(np.flatnonzero(bouncing[:, s])):
            h = int(lowbias32(np.array([p], dtype=np.uint32))[0])
            t = [None, None]
            for w in want:
                t[EDGES.index(w) // 2] = edge_coordinate((h & 0xffff) if w[0] == "x" else (h >> 16), w.endswith("hi"))
            if any(t[EDGES.index(w) // 2] is None for w in want):
                continue                                              # this pixel's shift cannot reach the far edge: the next
            free = [k for k in (0, 1) if t[k] is None]
            for _ in range(200 if free else 1):
                row = [rng.uniform(0., 1.) if v is None else v for v in t]
                x, y = shifted(row[0], row[1], np.array([p], dtype=np.uint32))
                if not free or disc_unclamped(x, y)[2][0] < 0.:
                    break
            else:
                continue
            out[s] = row
            targets.append(int(p))
            break
        else:
            raise AssertionError("row %d: no pixel that bounces reaches %s" % (s, kind))
    return np.ascontiguousarray(out), np.array(targets)


class Yardstick(SR.Yardstick):
    """SR.Yardstick with reference bounce frames, each made once and shared (never written to).  orb: the OracleBounce."""

    def __init__(self, pkg, O, orc, orb):
        super().__init__(pkg, O, orc)
        self.orb = orb
        self._bounce = {}

    def scene(self, name):
        if name == "floor" and name not in self._scene:
            self._scene[name] = floor_scenes(self.pkg, self.O)
        if name == "screens" and name not in self._scene:
            self._scene[name] = screens_scenes(self.pkg, self.O)
        return super().scene(name)

    def counters(self, name, w, h, depth, aperture, focus, table, offsets, bounce, strength, view=None):
        eye, basis = (self.eye(name), None) if view is None else view
        return counters(self.O, self.orb, self.scene(name)[1], eye, basis, w, h, depth, aperture, focus, table, offsets, bounce, strength)

    def bouncing_pixels(self, name, w, h, aperture, focus, table, view=None):
        eye, basis = (self.eye(name), None) if view is None else view
        return bouncing_pixels(self.orb, self.scene(name)[1], eye, basis, w, h, aperture, focus, table)

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
