"""Ray queries on the GPU (-m gpu): rm_intersect_rays / rm_occluded_rays / their device variants / rm_pick /
rm_primary_hits_device, through the C ABI, against the CPU oracle's own find_closest_intersect (shapes.rs:110-143),
intersect_shape_set (shapes.rs:92-108) and backproject (renderer.rs:128-135).

Decisions (hit, shape, occluded) must be the oracle's exactly; points and normals are held to TIGHT = 1e-9 per
component, as the render parity is.  The oracle is driven for many rays at once by a few lines of C compiled here
(`orc_batch`) that call liboracle.so's functions through the pointers ctypes hands them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import workloads

pytestmark = pytest.mark.gpu

TIGHT = 1e-9
RM_OK = 0

BATCH_C = r"""
#include <stdint.h>
#include <stddef.h>
#include "rm_oracle.h"
typedef int (*fci_t)(orc_vec3, orc_vec3, const orc_shape *, size_t, orc_intersection *, uint8_t *);
typedef int (*iss_t)(orc_vec3, orc_vec3, const orc_shape *, size_t);
typedef orc_vec3 (*bp_t)(const orc_renderer *, size_t, size_t);

static void one(fci_t fci, const orc_scene *s, orc_vec3 o, orc_vec3 d, int32_t *hit, int32_t *shape, double *pn) {
    orc_intersection is;
    uint8_t sh = 0;
    *hit = fci(o, d, s->shapes, s->n_shapes, &is, &sh);
    *shape = *hit ? (int32_t)sh : -1;
    pn[0] = *hit ? is.point.x : 0.; pn[1] = *hit ? is.point.y : 0.; pn[2] = *hit ? is.point.z : 0.;
    pn[3] = *hit ? is.normal.x : 0.; pn[4] = *hit ? is.normal.y : 0.; pn[5] = *hit ? is.normal.z : 0.;
}
void batch_closest(fci_t fci, const orc_scene *s, size_t n, const double *o, const double *d, int32_t *hit, int32_t *shape, double *pn) {
    for (size_t i = 0; i < n; i++) {
        orc_vec3 oo = {o[3 * i], o[3 * i + 1], o[3 * i + 2]}, dd = {d[3 * i], d[3 * i + 1], d[3 * i + 2]};
        one(fci, s, oo, dd, hit + i, shape + i, pn + 6 * i);
    }
}
void batch_occluded(iss_t iss, const orc_scene *s, size_t n, const double *o, const double *d, int32_t *occ) {
    for (size_t i = 0; i < n; i++) {
        orc_vec3 oo = {o[3 * i], o[3 * i + 1], o[3 * i + 2]}, dd = {d[3 * i], d[3 * i + 1], d[3 * i + 2]};
        occ[i] = iss(oo, dd, s->shapes, s->n_shapes);
    }
}
/* renderer.rs:80: pixel (x, y) -> backproject(x, y) from the camera, for the rows [0, rows) */
void batch_primary(fci_t fci, bp_t bp, const orc_renderer *r, const orc_scene *s, size_t w, size_t rows,
                   int32_t *hit, int32_t *shape, double *pn) {
    for (size_t y = 0; y < rows; y++)
        for (size_t x = 0; x < w; x++)
            one(fci, s, s->camera, bp(r, x, y), hit + y * w + x, shape + y * w + x, pn + 6 * (y * w + x));
}
"""


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batch(O, entry, tmp_path_factory):
    d = tmp_path_factory.mktemp("orc_batch")
    src, so = d / "orc_batch.c", d / "orc_batch.so"
    src.write_text(BATCH_C)
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-shared", "-fPIC",
                           "-I", os.path.join(entry.ROOT, "oracle"), str(src), "-o", str(so)])
    return OracleBatch(O, C.CDLL(str(so)))


class OracleBatch:
    def __init__(self, O, L):
        self.O, self.OL, self.L = O, O.lib(), L
        P, V = C.POINTER, C.c_void_p
        L.batch_closest.argtypes = [V, V, C.c_size_t, P(C.c_double), P(C.c_double), P(C.c_int32), P(C.c_int32), P(C.c_double)]
        L.batch_occluded.argtypes = [V, V, C.c_size_t, P(C.c_double), P(C.c_double), P(C.c_int32)]
        L.batch_primary.argtypes = [V, V, V, V, C.c_size_t, C.c_size_t, P(C.c_int32), P(C.c_int32), P(C.c_double)]
        self.fci = C.cast(self.OL.orc_find_closest_intersect, V)
        self.iss = C.cast(self.OL.orc_intersect_shape_set, V)
        self.bp = C.cast(self.OL.orc_backproject, V)

    @staticmethod
    def _p(a, t):
        return a.ctypes.data_as(C.POINTER(t))

    def closest(self, oscene, o, d):
        """-> hit (int32), shape (u8-wrapped as the reference's shape_hit; -1 on a miss), point / normal (N, 3)"""
        o, d = np.ascontiguousarray(o, np.float64), np.ascontiguousarray(d, np.float64)
        n = o.shape[0]
        hit, shape, pn = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 6))
        self.L.batch_closest(self.fci, C.cast(oscene.ptr, C.c_void_p), n, self._p(o, C.c_double), self._p(d, C.c_double),
                             self._p(hit, C.c_int32), self._p(shape, C.c_int32), self._p(pn, C.c_double))
        return hit, shape, pn[:, :3], pn[:, 3:]

    def occluded(self, oscene, o, d):
        o, d = np.ascontiguousarray(o, np.float64), np.ascontiguousarray(d, np.float64)
        occ = np.zeros(o.shape[0], np.int32)
        self.L.batch_occluded(self.iss, C.cast(oscene.ptr, C.c_void_p), o.shape[0], self._p(o, C.c_double),
                              self._p(d, C.c_double), self._p(occ, C.c_int32))
        return occ

    def primary(self, oscene, w, h, fov=workloads.FOV):
        rows = (h // 32) * 32
        r = self.OL.orc_create_renderer(float(fov), float(h), float(w))
        hit, shape, pn = np.zeros(rows * w, np.int32), np.zeros(rows * w, np.int32), np.zeros((rows * w, 6))
        self.L.batch_primary(self.fci, self.bp, C.cast(C.pointer(r), C.c_void_p), C.cast(oscene.ptr, C.c_void_p), w, rows,
                             self._p(hit, C.c_int32), self._p(shape, C.c_int32), self._p(pn, C.c_double))
        return hit.reshape(rows, w), shape.reshape(rows, w), pn.reshape(rows, w, 6)


# ---------------------------------------------------------------- scenes and rays
def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def random_rays(rng, n, lo, hi):
    o = rng.uniform(lo, hi, size=(n, 3))
    return o, unit(rng.normal(size=(n, 3)))


def inside_spheres(rng, desc, n):
    """Origins strictly inside the scene's spheres (radius from radius_square)."""
    sp = [desc.spheres[i] for i in range(desc.n_spheres)]
    k = rng.integers(0, len(sp), size=n)
    c = np.array([[sp[j].center.x, sp[j].center.y, sp[j].center.z] for j in k])
    r = np.sqrt(np.array([sp[j].radius_square for j in k]))
    return c + unit(rng.normal(size=(n, 3))) * (0.9 * r * rng.uniform(0., 1., n) ** (1. / 3.))[:, None]


def bounds_of(desc):
    pts = [[desc.spheres[i].center.x, desc.spheres[i].center.y, desc.spheres[i].center.z] for i in range(desc.n_spheres)]
    pts += [[desc.polygon_vertices[i].x, desc.polygon_vertices[i].y, desc.polygon_vertices[i].z] for i in range(desc.n_polygon_vertices)]
    for i in range(desc.n_triangles):
        pts += [[v.x, v.y, v.z] for v in desc.triangles[i].vertices]
    p = np.array(pts)
    lo, hi = p.min(axis=0), p.max(axis=0)
    pad = 0.25 * (hi - lo) + 1.
    return lo - pad, hi + pad


def build_pair(pkg, O, shapes, lights=workloads.DEMO_LIGHTS):
    """The same shape list as a product Scene and an oracle scene.  shapes: ("sphere", centre, radius) |
    ("polygon", vertices) | ("mesh", (n, 9) triangles)."""
    s, o = pkg.Scene.new(), O.OracleScene()
    for sh in shapes:
        if sh[0] == "sphere":
            s.shapes.append(pkg.sphere.create(pkg.Vec3f(*sh[1]), sh[2], pkg.Reflectance()))
            o.add_sphere(sh[1], sh[2], O.reflectance())
        elif sh[0] == "polygon":
            s.shapes.append(pkg.polygon.ConvexPolygon.create([pkg.Vec3f(*v) for v in sh[1]], pkg.Reflectance()))
            o.add_polygon(sh[1], O.reflectance())
        else:
            s.shapes.append(pkg.obj.Obj(np.asarray(sh[1], dtype=np.float64)))
            o.add_obj(np.asarray(sh[1], dtype=np.float64))
    for pos, col, inten in lights:
        s.lights.append(pkg.create_light(pkg.Vec3f(*pos), pkg.Vec3f(*col), inten))
        o.add_light(pos, col, inten)
    return s, o


def cloud(seed, n):
    rng = np.random.default_rng(seed)
    return [("sphere", tuple(rng.uniform((-40., -30., -120.), (40., 30., -10.))), float(rng.uniform(0.3, 2.5))) for _ in range(n)]


def upload(ctx, scene):
    h = scene.flatten()
    ctx.upload(h)
    return h.desc()


def check_closest(batch, ctx, oscene, o, d, wrap=False, label=""):
    """GPU closest hits of rays (o, d) against the oracle's; returns (GPU records, worst |point / normal delta|)."""
    g = ctx.intersect(o, d)
    hit, shape, point, normal = batch.closest(oscene, o, d)
    assert np.array_equal(g["hit"], hit), "%s: %d hit/miss decisions differ" % (label, int((g["hit"] != hit).sum()))
    m = hit == 1
    gs = g["shape"][m] % 256 if wrap else g["shape"][m]
    assert np.array_equal(gs, shape[m]), "%s: %d shape decisions differ" % (label, int((gs != shape[m]).sum()))
    worst = max(float(np.abs(g["point"][m] - point[m]).max(initial=0.)), float(np.abs(g["normal"][m] - normal[m]).max(initial=0.)))
    assert worst < TIGHT, "%s: point / normal differ by %.3e" % (label, worst)
    # a miss is all zeros; t places the point on the ray
    assert not g[~m].view(np.float64).reshape(-1, 9).any()
    assert np.abs(o[m] + d[m] * g["t"][m][:, None] - g["point"][m]).max(initial=0.) < 1e-9 * (1. + np.abs(g["point"][m]).max(initial=0.))
    return g, worst


def check_occluded(batch, ctx, oscene, o, d, label=""):
    g = ctx.occluded(o, d)
    ref = batch.occluded(oscene, o, d).astype(bool)
    assert np.array_equal(g, ref), "%s: %d occlusion decisions differ" % (label, int((g != ref).sum()))
    return g


# ---------------------------------------------------------------- 1. demo scene, random rays
def test_demo_random_rays_match_the_oracle(pkg, O, ctx, batch):
    scene, oscene = workloads.product_scene(pkg, "demo"), workloads.oracle_scene(O, "demo")
    desc = upload(ctx, scene)
    rng = np.random.default_rng(20261016)
    lo, hi = bounds_of(desc)
    o1, d1 = random_rays(rng, 16000, lo, hi)
    o2 = inside_spheres(rng, desc, 4000)
    o = np.concatenate([o1, o2])
    d = np.concatenate([d1, unit(rng.normal(size=(4000, 3)))])
    g, worst = check_closest(batch, ctx, oscene, o, d, label="demo random")
    occ = check_occluded(batch, ctx, oscene, o, d, label="demo random")
    assert np.array_equal(occ[g["hit"] == 1], np.ones(int((g["hit"] == 1).sum()), bool))      # a closest hit is a hit
    print("demo random rays: %d of %d hit, %d occluded, max |point / normal delta| %.3e" %
          (int(g["hit"].sum()), len(o), int(occ.sum()), worst))
    assert 0.1 * len(o) < g["hit"].sum() < len(o)


# ---------------------------------------------------------------- 2. exact incidence
def exact_incidence_rays(rng, desc, origins):
    """Rays aimed at polygon vertices, edge points and triangle edges, lying in planes, and grazing spheres."""
    O_, D_ = [], []

    def aim(o, target):
        v = np.asarray(target, float) - o
        if np.linalg.norm(v) > 1e-9:
            O_.append(o); D_.append(unit(v))

    def planar(verts, normal):
        verts = [np.array([v.x, v.y, v.z]) for v in verts]
        n = np.array([normal.x, normal.y, normal.z])
        for o in origins:
            for k, v in enumerate(verts):
                w = verts[(k + 1) % len(verts)]
                aim(o, v)
                for f in (0.5, 0.25, 1. / 3.):
                    aim(o, v + f * (w - v))
        # lying in the plane: origin on the plane, direction perpendicular to the normal (zero or tiny denominator)
        c = np.mean(verts, axis=0)
        for k in range(8):
            t = np.cross(n, rng.normal(size=3))
            O_.append(c + 0.1 * k * (verts[0] - c)); D_.append(unit(t))
            O_.append(verts[k % len(verts)] - 3. * unit(t)); D_.append(unit(t))

    for i in range(desc.n_polygons):
        p = desc.polygons[i]
        planar([desc.polygon_vertices[p.first_vertex + k] for k in range(p.n_vertices)], p.plane_normal)
    for i in range(min(desc.n_triangles, 64)):
        t = desc.triangles[i]
        planar(list(t.vertices), t.normal)
    for i in range(desc.n_spheres):
        s = desc.spheres[i]
        c, r = np.array([s.center.x, s.center.y, s.center.z]), np.sqrt(s.radius_square)
        for o in origins:
            axis = c - o
            L = np.linalg.norm(axis)
            if L <= r * 1.01:
                continue
            alpha = np.arcsin(r / L)
            for k in range(8):
                u = unit(np.cross(axis, rng.normal(size=3)))
                O_.append(o); D_.append(unit(np.cos(alpha) * unit(axis) + np.sin(alpha) * u))
    return np.array(O_), np.array(D_)


def test_exact_incidence_and_shadow_offset_rays_match_the_oracle(pkg, O, ctx, batch):
    scene, oscene = workloads.product_scene(pkg, "demo"), workloads.oracle_scene(O, "demo")
    desc = upload(ctx, scene)
    rng = np.random.default_rng(7)
    origins = [np.zeros(3), np.array([1., 2., 3.]), np.array([-7., 4., 2.]), np.array([0., 10., -10.])]
    o, d = exact_incidence_rays(rng, desc, origins)
    check_closest(batch, ctx, oscene, o, d, label="exact incidence")
    check_occluded(batch, ctx, oscene, o, d, label="exact incidence")
    # the render's shadow rays: from a hit point 1e-3 of the normal off it, towards each light (renderer.rs:166-172)
    lo, hi = bounds_of(desc)
    ro, rd = random_rays(rng, 6000, lo, hi)
    g = ctx.intersect(ro, rd)
    m = g["hit"] == 1
    p, n = g["point"][m], g["normal"][m]
    so, sd = [], []
    for pos, _, _ in workloads.DEMO_LIGHTS:
        ld = unit(np.asarray(pos) - p)
        side = np.where((ld * n).sum(axis=1) < 0., -1e-3, 1e-3)
        so.append(p + n * side[:, None]); sd.append(ld)
    so, sd = np.concatenate(so), np.concatenate(sd)
    ok = np.abs((sd * sd).sum(axis=1) - 1.) < 1e-4
    check_occluded(batch, ctx, oscene, so[ok], sd[ok], label="shadow rays")
    check_closest(batch, ctx, oscene, so[ok], sd[ok], label="shadow rays")
    print("exact incidence: %d rays; shadow-offset rays: %d" % (len(o), int(ok.sum())))


# ---------------------------------------------------------------- 3. ties: first in list order wins
def test_coincident_primitives_go_to_the_first_in_list_order(pkg, O, ctx, batch):
    quad = [(-3., -3., -20.), (3., -3., -20.), (3., 3., -20.), (-3., 3., -20.)]
    shapes = [("sphere", (8., 0., -15.), 2.), ("polygon", quad), ("sphere", (-8., 0., -15.), 2.5),
              ("sphere", (8., 0., -15.), 2.), ("polygon", quad), ("sphere", (-8., 0., -15.), 2.5)]
    scene, oscene = build_pair(pkg, O, shapes)
    upload(ctx, scene)
    rng = np.random.default_rng(3)
    targets = np.concatenate([rng.uniform((6.5, -1.5, -15.), (9.5, 1.5, -15.), (300, 3)),
                              rng.uniform((-2.9, -2.9, -20.), (2.9, 2.9, -20.), (300, 3)),
                              rng.uniform((-10., -2., -15.), (-6., 2., -15.), (300, 3))])
    o = np.zeros_like(targets)
    d = unit(targets - o)
    g, _ = check_closest(batch, ctx, oscene, o, d, label="ties")
    m = g["hit"] == 1
    assert m.sum() > 600
    assert set(np.unique(g["shape"][m])) <= {0, 1, 2}, "a duplicate later in the list won a tie"
    check_occluded(batch, ctx, oscene, o, d, label="ties")


# ---------------------------------------------------------------- 4. meshes: shape and element
def test_cornell_meshes_name_shape_and_triangle(pkg, O, ctx, batch):
    scene, oscene = workloads.product_scene(pkg, "cornell"), workloads.oracle_scene(O, "cornell")
    desc = upload(ctx, scene)
    assert desc.n_triangles >= 12
    rng = np.random.default_rng(11)
    lo, hi = bounds_of(desc)
    o1, d1 = random_rays(rng, 6000, lo, hi)
    # ... and rays aimed at random points of random triangles (most of the box's walls lie along z: the reference's
    # 2-D inside test never lets a ray hit those, so blind rays find few hits)
    tri = np.array([[[v.x, v.y, v.z] for v in desc.triangles[i].vertices] for i in range(desc.n_triangles)])
    k = rng.integers(0, len(tri), 6000)
    b = rng.dirichlet((1., 1., 1.), 6000)
    o2 = rng.uniform(lo, hi, size=(6000, 3))
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, unit((tri[k] * b[:, :, None]).sum(axis=1) - o2)])
    g, worst = check_closest(batch, ctx, oscene, o, d, label="cornell")
    check_occluded(batch, ctx, oscene, o, d, label="cornell")
    m = np.nonzero(g["hit"] == 1)[0]
    assert len(m) > 1000
    ref_hit, _, ref_point, _ = batch.closest(oscene, o[m], d[m])
    L = O.lib()
    shapes = oscene.c.shapes
    counts = [desc.shapes[i].count for i in range(desc.n_shapes)]
    for j, i in enumerate(m[:3000]):
        sh, el = int(g["shape"][i]), int(g["element"][i])
        assert el < counts[sh]
        alone = O.Intersection()
        assert L.orc_triangle_intersect(C.byref(shapes[sh].triangles[el]), O.v3(o[i]), O.v3(d[i]), C.byref(alone)) == 1
        assert alone.point.tup() == tuple(ref_point[j]), "ray %d: triangle %d of shape %d is not the one hit" % (i, el, sh)
    print("cornell: %d of %d rays hit, max |point / normal delta| %.3e" % (len(m), len(o), worst))


# ---------------------------------------------------------------- 5. hierarchy paths, shape indices past 255
@pytest.mark.parametrize("which", ["synthetic256", "cloud1000"])
def test_hierarchy_scenes_match_the_oracle(pkg, O, ctx, batch, which):
    if which == "synthetic256":
        scene, oscene = workloads.product_scene(pkg, "synthetic256"), workloads.oracle_scene(O, "synthetic256")
    else:
        scene, oscene = build_pair(pkg, O, cloud(1000, 1000))
    desc = upload(ctx, scene)
    rng = np.random.default_rng(5)
    lo, hi = bounds_of(desc)
    o1, d1 = random_rays(rng, 12000, lo, hi)
    o2 = inside_spheres(rng, desc, 3000)
    o = np.concatenate([o1, o2, np.tile(0.5 * (lo + hi), (3000, 1))])
    d = np.concatenate([d1, unit(rng.normal(size=(6000, 3)))])
    g, worst = check_closest(batch, ctx, oscene, o, d, wrap=True, label=which)
    check_occluded(batch, ctx, oscene, o, d, label=which)
    m = np.nonzero(g["hit"] == 1)[0]
    _, _, ref_point, _ = batch.closest(oscene, o[m], d[m])
    L = O.lib()
    shapes = oscene.c.shapes
    for j, i in enumerate(m[:3000]):
        alone = O.Intersection()
        assert L.orc_shape_intersect(C.byref(shapes[int(g["shape"][i])]), O.v3(o[i]), O.v3(d[i]), C.byref(alone)) == 1
        assert alone.point.tup() == tuple(ref_point[j])
    if which == "cloud1000":
        assert g["shape"][m].max() > 255                        # the record is not wrapped to u8
    print("%s: %d of %d rays hit, max |point / normal delta| %.3e" % (which, len(m), len(o), worst))


# ---------------------------------------------------------------- 6. the primary-hit buffer
@pytest.mark.parametrize("name,w,h,cam", [("demo", 320, 240, (1., 2., 3.)), ("demo", 1920, 1080, (-2., 1., 4.)),
                                          ("cornell", 1920, 1080, (20., 30., -50.))])
def test_primary_hits_match_the_oracle_and_the_frame(pkg, O, ctx, batch, name, w, h, cam):
    import torch
    scene, oscene = workloads.product_scene(pkg, name), workloads.oracle_scene(O, name)
    upload(ctx, scene)
    ctx.set_camera(cam)
    oscene.set_camera(cam)
    p = pkg.backend.make_params(workloads.FOV, float(h), float(w), 5)
    sentinel = -7.25
    out = torch.full((h, w, 9), sentinel, dtype=torch.float64, device="cuda:0")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    hits = ctx.primary_hits_device(p, out=out, stream=s)
    s.synchronize()
    rows = (h // 32) * 32
    raw = out.cpu().numpy()
    assert (raw[rows:] == sentinel).all(), "the rows below the last whole patch row were written"
    rec = raw[:rows].reshape(-1).view(pkg.backend.HIT_DTYPE).reshape(rows, w)
    ref_hit, ref_shape, ref_pn = batch.primary(oscene, w, h)
    assert np.array_equal(rec["hit"], ref_hit)
    m = ref_hit == 1
    assert np.array_equal(rec["shape"][m] % 256, ref_shape[m])
    assert np.abs(rec["point"][m] - ref_pn[..., :3][m]).max(initial=0.) < TIGHT
    assert np.abs(rec["normal"][m] - ref_pn[..., 3:][m]).max(initial=0.) < TIGHT
    assert hits.hit.shape == (h, w) and bool((hits.hit[:rows].cpu().numpy() == rec["hit"]).all())
    # the render at the same params: a primary ray that hits nothing leaves the primary-miss value, +0.0 in every
    # channel (renderer.rs:305); one that hits something gets at least the background (renderer.rs:40-44, 270-275)
    frame = np.zeros((h, w, 3))
    ctx.render(p, frame)
    lit = frame[:rows].max(axis=2) > 0.
    assert np.array_equal(lit, m), "%d pixels where the frame and the hit buffer disagree" % int((lit != m).sum())
    assert (frame[:rows][~m] == 0.).all() and not np.signbit(frame[:rows][~m]).any()          # +0.0 exactly
    # rm_pick at sampled pixels is the buffer's entry, bit for bit; the strip below the patch rows is answered too
    rng = np.random.default_rng(w + h)
    for x, y in list(zip(rng.integers(0, w, 40), rng.integers(0, rows, 40))) + [(0, 0), (w - 1, rows - 1), (w // 2, h // 2)]:
        pk = ctx.pick(p, int(x), int(y))
        assert bytes(pk) == rec[y, x].tobytes(), (x, y)
    if rows < h:
        y = h - 1
        pk = ctx.pick(p, 5, y)
        r = O.lib().orc_create_renderer(workloads.FOV, float(h), float(w))
        dref = O.lib().orc_backproject(C.byref(r), 5, y)
        rh, rs, _, _ = batch.closest(oscene, np.array([oscene.c.camera.tup()]), np.array([dref.tup()]))
        assert pk.hit == rh[0] and (not pk.hit or pk.shape % 256 == rs[0])
    print("%s %dx%d: %d of %d pixels hit" % (name, w, h, int(m.sum()), m.size))


# ---------------------------------------------------------------- 7. device variants
@pytest.mark.parametrize("n", [0, 1, 63, 65, 1000, 4097])
def test_device_variants_equal_the_host_variants(pkg, ctx, n):
    import torch
    scene = workloads.product_scene(pkg, "synthetic256")
    desc = upload(ctx, scene)
    rng = np.random.default_rng(n)
    lo, hi = bounds_of(desc)
    o, d = random_rays(rng, n, lo, hi)
    host = ctx.intersect(o, d)
    host_occ = ctx.occluded(o, d)
    s = torch.cuda.Stream()
    to, td = torch.from_numpy(o).to("cuda:0"), torch.from_numpy(d).to("cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        dh = ctx.intersect_device(to, td)
        docc = ctx.occluded_device(to, td)
    s.synchronize()
    assert dh.raw.shape == (n, 9) and docc.shape == (n,) and docc.dtype == torch.bool
    assert dh.raw.cpu().numpy().tobytes() == host.tobytes()
    assert np.array_equal(docc.cpu().numpy(), host_occ)
    assert np.array_equal(dh.shape.cpu().numpy(), host["shape"].astype(np.int32))
    assert np.array_equal(dh.point.cpu().numpy(), host["point"])
    # torch's current stream by default (here its default stream): ordered with what torch does next, no sync of ours
    dd = ctx.intersect_device(to, td)
    assert dd.raw.cpu().numpy().tobytes() == host.tobytes()
    assert np.array_equal(ctx.occluded_device(to, td).cpu().numpy(), host_occ)


# ---------------------------------------------------------------- 8. queries leave the frames alone
def test_queries_do_not_disturb_the_frames(pkg):
    import torch
    demo, cornell = workloads.product_scene(pkg, "demo"), workloads.product_scene(pkg, "cornell")
    rng = np.random.default_rng(8)
    o, d = random_rays(rng, 5000, (-20., -10., -50.), (20., 10., 5.))

    def queries(c):
        c.intersect(o, d)
        c.occluded(o, d)
        c.pick(pkg.backend.make_params(1.2, 480., 640., 3), 17, 23)                   # another frame geometry
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            c.primary_hits_device(pkg.backend.make_params(workloads.FOV, 256., 320., 3))
            c.intersect_device(torch.from_numpy(o).to("cuda:0"), torch.from_numpy(d).to("cuda:0"))
        s.synchronize()

    def frames(with_queries):
        c = pkg.backend.Context(0)
        out = []
        p = pkg.backend.make_params(workloads.FOV, 1080., 1920., 5)
        for step in range(6):
            if step == 4:
                c.upload(cornell.flatten())
            elif step == 0:
                c.upload(demo.flatten())
            if step == 3:
                c.set_camera((0., 1., -2.))
            if with_queries and step in (1, 2, 4):
                queries(c)
            f = np.zeros((1080, 1920, 3))
            c.render(p, f)
            out.append(f)
        c.close()
        return out

    plain, queried = frames(False), frames(True)
    for k, (a, b) in enumerate(zip(plain, queried)):
        assert a.tobytes() == b.tobytes(), "frame %d differs once queries ran in between" % k


# ---------------------------------------------------------------- 9. refusals
def test_refusals(pkg, ctx):
    L, B = pkg.lib(), pkg._lib
    fresh = pkg.backend.Context(0)
    o, d = np.zeros((1, 3)), np.array([[0., 0., -1.]])
    p = pkg.backend.make_params(workloads.FOV, 240., 320., 3)
    with pytest.raises(pkg.BackendError) as e:
        fresh.intersect(o, d)
    assert e.value.status == B.RM_ERR_NO_SCENE
    with pytest.raises(pkg.BackendError) as e:
        fresh.pick(p, 0, 0)
    assert e.value.status == B.RM_ERR_NO_SCENE
    assert L.rm_occluded_rays_device(fresh.ptr, None, None, 4, None, None) == B.RM_ERR_NO_SCENE
    fresh.close()

    upload(ctx, workloads.product_scene(pkg, "demo"))
    # n_rays == 0 does nothing
    assert L.rm_intersect_rays(ctx.ptr, None, None, 0, None) == RM_OK
    assert L.rm_occluded_rays_device(ctx.ptr, None, None, 0, None, None) == RM_OK
    # flags: RM_FLAG_FAST_FP is accepted and ignored (the answer is the strict one), anything else refused
    strict = ctx.pick(p, 160, 200)
    p.flags = B.RM_FLAG_FAST_FP
    assert bytes(ctx.pick(p, 160, 200)) == bytes(strict)
    for bad in (B.RM_FLAG_U8_COMPACT, B.RM_FLAG_F64_COMPACT, B.RM_FLAG_FAST_FP | B.RM_FLAG_U8_COMPACT, 1):
        p.flags = bad
        with pytest.raises(pkg.BackendError) as e:
            ctx.pick(p, 0, 0)
        assert e.value.status == B.RM_ERR_INVALID_ARG
    p.flags = 0
    p.patch_row_begin, p.patch_row_end = 1, 3
    with pytest.raises(pkg.BackendError) as e:
        ctx.primary_hits_device(p)
    assert e.value.status == B.RM_ERR_INVALID_ARG
    p.patch_row_begin, p.patch_row_end = 0, 0
    # directions: unit within 1e-4 (the reference asserts), finite; the first bad ray is named
    for bad_d, bad_o in (([0., 0., -1.01], [0., 0., 0.]), ([np.nan, 0., -1.], [0., 0., 0.]), ([0., 0., -1.], [np.inf, 0., 0.])):
        oo = np.zeros((4, 3))
        dd = np.tile([0., 0., -1.], (4, 1))
        dd[2], oo[2] = bad_d, bad_o
        for call in (ctx.intersect, ctx.occluded):
            with pytest.raises(pkg.BackendError) as e:
                call(oo, dd)
            assert e.value.status == B.RM_ERR_INVALID_ARG and "ray 2" in str(e.value)
    ctx.intersect(np.zeros((1, 3)), np.array([[0., 0., -1.00004]]))                    # within the assert: answered (and held to the oracle: tests/test_gpu_hierarchy_walk.py)
    # pixels outside the frame; the frame width need not be a multiple of 32 for a pick, it must for the buffer
    for x, y in ((320, 0), (0, 240), (10**6, 10**6)):
        with pytest.raises(pkg.BackendError) as e:
            ctx.pick(p, x, y)
        assert e.value.status == B.RM_ERR_INVALID_ARG
    odd = pkg.backend.make_params(workloads.FOV, 240., 100., 3)
    ctx.pick(odd, 99, 239)
    with pytest.raises(pkg.BackendError) as e:
        ctx.primary_hits_device(odd)
    assert e.value.status == B.RM_ERR_DIMENSIONS


def test_renderer_pick_names_the_shape_of_the_scene(pkg, O, batch):
    scene = workloads.product_scene(pkg, "demo")
    r = pkg.create_renderer(workloads.FOV, 240., 320.)
    fb = pkg.create_frame_buffer(320, 240)
    oscene = workloads.oracle_scene(O, "demo")
    ref_hit, ref_shape, _ = batch.primary(oscene, 320, 240)
    seen = set()
    for x, y in [(160, 120), (10, 10), (300, 200), (80, 200), (250, 60), (160, 220)]:
        h = r.pick(fb, scene, x, y)
        assert (h is not None) == bool(ref_hit[y, x])
        if h is not None:
            assert h.shape == ref_shape[y, x] and 0 <= h.shape < len(scene.shapes)
            seen.add(h.shape)
    assert seen
