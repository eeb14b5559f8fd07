"""The oriented camera on the GPU (-m gpu): rm_camera_orient / rm_camera_look_at through the C ABI against the CPU oracle.

The reference for every oriented frame is the oracle's own cast_ray: per pixel the un-normalised direction is formed here in
numpy exactly as the header states it -- d.c = (bx * right.c + by * up.c) + forward.c, bx and by the two numbers backproject
(renderer.rs:128-135) forms for the pixel, every operation rounded once -- normalised by orc_normalized and cast by
orc_cast_ray(eye, dir, scene, (0.1, 0.1, 0.1), 1, max_depth).  A few lines of C compiled here (`orc_camera`) drive the oracle
for a frame's rays on several threads.  Strict flavour: every channel of every pixel within TIGHT = 1e-9.  Fast flavour: the
rule of tests/tie_reference.py (compare_fast): the same bound but at certified ties, and no tie where none is named.  Rows from height - height % 32 on are not rendered
(renderer.rs:53) and must stay untouched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tie_reference as TR
import workloads

pytestmark = pytest.mark.gpu

TIGHT = 1e-9
RM_FLAG_FAST_FP = 2
RM_FLAG_U8_COMPACT = 4
LIT_FLOOR = 0.05                      # share of the oracle's own frame that is not sky: no view passes vacuously

CAMERA_C = r"""
#include <pthread.h>
#include <stdint.h>
#include <stddef.h>
#include "rm_oracle.h"
typedef orc_vec3 (*cast_t)(orc_vec3, orc_vec3, const orc_scene *, orc_vec3, unsigned, unsigned);
typedef orc_vec3 (*norm_t)(orc_vec3);
typedef int (*fci_t)(orc_vec3, orc_vec3, const orc_shape *, size_t, orc_intersection *, uint8_t *);
typedef struct {
    cast_t cast; norm_t norm; fci_t fci; const orc_scene *s; orc_vec3 eye; const double *d; unsigned depth;
    double *rgb; int32_t *hit, *shape; double *pn;
    size_t begin, end;
} job_t;
static void *run(void *p) {
    job_t *j = (job_t *)p;
    const orc_vec3 bg = {0.1, 0.1, 0.1};
    for (size_t i = j->begin; i < j->end; i++) {
        orc_vec3 d = {j->d[3 * i], j->d[3 * i + 1], j->d[3 * i + 2]};
        d = j->norm(d);
        if (j->rgb) {
            const orc_vec3 c = j->cast(j->eye, d, j->s, bg, 1, j->depth);
            j->rgb[3 * i] = c.x; j->rgb[3 * i + 1] = c.y; j->rgb[3 * i + 2] = c.z;
        }
        if (j->hit) {
            orc_intersection is;
            uint8_t sh = 0;
            const int h = j->fci(j->eye, d, j->s->shapes, j->s->n_shapes, &is, &sh);
            double *pn = j->pn + 9 * i;
            j->hit[i] = h; j->shape[i] = h ? (int32_t)sh : -1;
            pn[0] = h ? is.point.x : 0.; pn[1] = h ? is.point.y : 0.; pn[2] = h ? is.point.z : 0.;
            pn[3] = h ? is.normal.x : 0.; pn[4] = h ? is.normal.y : 0.; pn[5] = h ? is.normal.z : 0.;
            pn[6] = d.x; pn[7] = d.y; pn[8] = d.z;
        }
    }
    return NULL;
}
/* n rays from `eye` along the un-normalised directions d[n][3]: radiance into rgb (NULL: not asked for), closest hits into
   hit / shape / pn[n][9] = point, normal, the normalised direction (hit NULL: not asked for) */
void camera_rays(cast_t cast, norm_t norm, fci_t fci, const orc_scene *s, const double *eye, size_t n, const double *d, unsigned depth,
                 double *rgb, int32_t *hit, int32_t *shape, double *pn, int n_threads) {
    pthread_t th[64];
    job_t jobs[64];
    if (n_threads < 1) n_threads = 1;
    if (n_threads > 64) n_threads = 64;
    const size_t per = (n + (size_t)n_threads - 1) / (size_t)n_threads;
    for (int t = 0; t < n_threads; t++) {
        job_t j = {cast, norm, fci, s, {eye[0], eye[1], eye[2]}, d, depth, rgb, hit, shape, pn, 0, 0};
        j.begin = per * (size_t)t < n ? per * (size_t)t : n;
        j.end = j.begin + per < n ? j.begin + per : n;
        jobs[t] = j;
        pthread_create(&th[t], NULL, run, &jobs[t]);
    }
    for (int t = 0; t < n_threads; t++) pthread_join(th[t], NULL);
}
"""

_FLAGS = {"value": 0}


@pytest.fixture(params=["strict", "fast"])
def flavour(request):
    _FLAGS["value"] = RM_FLAG_FAST_FP if request.param == "fast" else 0
    yield request.param
    _FLAGS["value"] = 0


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cam(O, entry, tmp_path_factory):
    d = tmp_path_factory.mktemp("orc_camera")
    src, so = d / "orc_camera.c", d / "orc_camera.so"
    src.write_text(CAMERA_C)
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-shared", "-fPIC", "-pthread",
                           "-I", os.path.join(entry.ROOT, "oracle"), str(src), "-o", str(so)])
    return OracleCamera(O, C.CDLL(str(so)))


class OracleCamera:
    def __init__(self, O, L):
        self.O, self.OL, self.L = O, O.lib(), L
        P, V = C.POINTER, C.c_void_p
        L.camera_rays.argtypes = [V, V, V, V, P(C.c_double), C.c_size_t, P(C.c_double), C.c_uint, P(C.c_double), P(C.c_int32),
                                  P(C.c_int32), P(C.c_double), C.c_int]
        self.cast = C.cast(self.OL.orc_cast_ray, V)
        self.norm = C.cast(self.OL.orc_normalized, V)
        self.fci = C.cast(self.OL.orc_find_closest_intersect, V)
        self.threads = max(1, min(16, len(os.sched_getaffinity(0))))
        self.frames = {}

    def directions(self, basis, w, h, fov=workloads.FOV, rows=None):
        """Un-normalised primary directions of the rows [0, rows) of a w x h frame, formed as the header states."""
        r = self.OL.orc_create_renderer(float(fov), float(h), float(w))
        rows = (h // 32) * 32 if rows is None else rows
        # backproject's two numbers, its operations one by one (renderer.rs:128-135)
        bx = 2. * (np.arange(w, dtype=np.float64) / r.width - 0.5) * r.half_fov * r.ratio
        by = -2. * (np.arange(rows, dtype=np.float64) / r.height - 0.5) * r.half_fov
        right, up, forward = basis
        d = np.empty((rows, w, 3))
        for c in range(3):
            d[:, :, c] = (bx[None, :] * right[c] + by[:, None] * up[c]) + forward[c]
        return d

    def _rays(self, oscene, eye, d, depth, want_rgb, want_hits):
        d = np.ascontiguousarray(d.reshape(-1, 3))
        n = d.shape[0]
        eye = np.ascontiguousarray(eye, dtype=np.float64)
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a is not None else None
        rgb = np.zeros((n, 3)) if want_rgb else None
        hit = np.zeros(n, np.int32) if want_hits else None
        shape = np.zeros(n, np.int32) if want_hits else None
        pn = np.zeros((n, 9)) if want_hits else None
        self.L.camera_rays(self.cast, self.norm, self.fci, C.cast(oscene.ptr, C.c_void_p), p(eye, C.c_double), n, p(d, C.c_double),
                           depth, p(rgb, C.c_double), p(hit, C.c_int32), p(shape, C.c_int32), p(pn, C.c_double), self.threads)
        return rgb, hit, shape, pn

    def frame(self, name, oscene, eye, basis, w, h, depth):
        """The oracle's frame of the rendered rows, (rows, w, 3); kept per view so that the two flavours share it."""
        key = (name, tuple(eye), tuple(map(tuple, basis)), w, h, depth)
        if key not in self.frames:
            rgb, _, _, _ = self._rays(oscene, eye, self.directions(basis, w, h), depth, True, False)
            self.frames[key] = rgb.reshape((h // 32) * 32, w, 3)
        return self.frames[key]

    def hits(self, oscene, eye, basis, w, h):
        d = self.directions(basis, w, h)
        _, hit, shape, pn = self._rays(oscene, eye, d, 1, False, True)
        rows = d.shape[0]
        return hit.reshape(rows, w), shape.reshape(rows, w), pn.reshape(rows, w, 9)


# ---------------------------------------------------------------- helpers
def basis_rows(b):
    """rm_camera_basis -> ((right), (up), (forward)) as tuples of Python floats: the very doubles the library holds."""
    return tuple((v.x, v.y, v.z) for v in (b.right, b.up, b.forward))


def view(pkg, eye, target, up=(0., 1., 0.), roll=0.):
    b = pkg.backend.basis_look_at(eye, target, up)
    if roll:
        b = pkg.backend.basis_turn(b, 0., 0., roll)
    return tuple(float(c) for c in eye), b


def params(pkg, w, h, depth, band=None, flags=None):
    p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth, band)
    p.flags = _FLAGS["value"] if flags is None else flags
    return p


def set_view(ctx, eye, basis):
    ctx.set_camera(eye)
    ctx.orient(basis)


def device_frame(ctx, p, sentinel=-1.):
    """One frame into a device buffer that holds `sentinel` everywhere beforehand."""
    import torch
    dev = torch.full((p.frame_height, p.frame_width, 3), sentinel, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.render_device(p, dev.data_ptr())
    torch.cuda.synchronize()
    return dev.cpu().numpy()


def compare(gpu, ref, label, tol=TIGHT, tie=None):
    """strict -- every channel within tol; fast -- tests/tie_reference.py compare_fast: the same bound but at the certified
    ties of `tie` (a tie_reference.Tie; None: the frame may differ nowhere).  Returns (worst delta among the pixels held to
    the bound, differing pixels seen)."""
    d = np.abs(gpu - ref)
    if _FLAGS["value"] & RM_FLAG_FAST_FP:
        worst, n_bad = TR.compare_fast(gpu, ref, tol, tie, label)
        print("%s: fast flavour, %d differing pixels" % (label, n_bad))
        return worst, n_bad
    worst = float(d.max())
    print("%s: strict flavour, max |delta| %.3e" % (label, worst))
    assert worst < tol, "%s: max |delta| %.3e (channels above 1e-12: %d)" % (label, worst, int((d > 1e-12).sum()))
    return worst, 0


def check_frame(pkg, ctx, cam, name, scene, oscene, eye, basis, w, h, depth, label):
    ctx.upload(scene.flatten())
    set_view(ctx, eye, basis)
    sentinel = -1.
    got = device_frame(ctx, params(pkg, w, h, depth), sentinel)
    rows = (h // 32) * 32
    assert (got[rows:] == sentinel).all(), "%s: rows below the last whole patch row were written" % label
    ref = cam.frame(name, oscene, eye, basis_rows(basis), w, h, depth)
    lit = float((ref.max(axis=2) > 0.).mean())
    print("%s: %.3f of the oracle's pixels are not sky" % (label, lit))
    assert lit > LIT_FLOOR, "%s: the oracle's frame is %.3f not sky" % (label, lit)
    assert not (got[:rows] == sentinel).any(), "%s: a pixel of the rendered rows was left out" % label
    return compare(got[:rows], ref, label)


@pytest.fixture
def fixed_view_after(ctx):
    yield
    ctx.orient(None)


DEMO_VIEWS = [
    ("right-front", (25., 10., 5.), (0., 0., -16.), (0., 1., 0.), 0.),
    ("left-above", (-30., 20., -16.), (0., 0., -16.), (0., 1., 0.), 0.),
    ("straight-down", (0., 40., -15.), (0., 0., -16.), (0., 0., -1.), 0.),
    ("from-behind", (0., 5., -45.), (0., 0., -16.), (0., 1., 0.), 0.),
    ("off-axis", (10., 3., 10.), (-5., 0., -20.), (0., 1., 0.), 0.),
    ("left-above-rolled", (-30., 20., -16.), (0., 0., -16.), (0., 1., 0.), 0.3),
]


# ---------------------------------------------------------------- 1. oriented frames match the oracle
@pytest.mark.parametrize("w,h", [(256, 160), (1920, 1080)])
@pytest.mark.parametrize("v", DEMO_VIEWS, ids=[v[0] for v in DEMO_VIEWS])
def test_demo_views_match_the_oracle(pkg, O, ctx, cam, flavour, fixed_view_after, v, w, h):
    _, eye, target, up, roll = v
    eye, basis = view(pkg, eye, target, up, roll)
    scene, oscene = workloads.product_scene(pkg, "demo"), workloads.oracle_scene(O, "demo")
    check_frame(pkg, ctx, cam, "demo", scene, oscene, eye, basis, w, h, 5, "demo %s %dx%d" % (v[0], w, h))


CORNELL_TARGET = (277., 189., -218.)      # the mean of the box's triangle centres


@pytest.mark.parametrize("eye", [(0., 0., 0.), (600., 200., -100.)])
def test_cornell_views_match_the_oracle(pkg, O, ctx, cam, flavour, fixed_view_after, eye):
    eye, basis = view(pkg, eye, CORNELL_TARGET)
    scene, oscene = workloads.product_scene(pkg, "cornell"), workloads.oracle_scene(O, "cornell")
    check_frame(pkg, ctx, cam, "cornell", scene, oscene, eye, basis, 256, 160, 5, "cornell from %s" % (eye,))


@pytest.mark.parametrize("eye,target,up", [((35., 10., -5.), (0., 2., -42.), (0., 1., 0.)), ((-30., 5., -75.), (0., 2., -42.), (0., 1., 0.)),
                                           ((0., 45., -41.), (0., 2., -41.), (0., 0., -1.))])
def test_hierarchy_scene_views_match_the_oracle(pkg, O, ctx, cam, flavour, fixed_view_after, eye, target, up):
    """256 spheres and the floor: the hierarchy kernels, depth 10."""
    eye, basis = view(pkg, eye, target, up)
    scene, oscene = workloads.product_scene(pkg, "synthetic256"), workloads.oracle_scene(O, "synthetic256")
    ctx.upload(scene.flatten())
    ctx.orient(basis)
    targs = ctx.kernel_name(params(pkg, 512, 512, 10)).split("<")[1].rstrip(">").split(", ")
    assert targs[5] == "true" and targs[6] == "true", targs                   # STACK, POW, waves, per wave, STAGED, BVH, CULL, ...
    check_frame(pkg, ctx, cam, "synthetic256", scene, oscene, eye, basis, 512, 512, 10, "256 spheres from %s" % (eye,))


# ---------------------------------------------------------------- 2. the fixed view is untouched
@pytest.mark.parametrize("cfg", ["C1", "C2", "C3"])
def test_the_fixed_view_is_untouched(pkg, ctx, flavour, fixed_view_after, cfg):
    """orient(identity), orient(NULL) and a fresh context give bit-equal frames and launch the same kernel; a real turn
    launches another (the oriented kernels live in namespaces of their own)."""
    c = workloads.CONFIGS[cfg]
    w, h, depth = c["width"], c["height"], c["max_depth"]
    scene = workloads.product_scene(pkg, c["scene"])
    p = params(pkg, w, h, depth)
    fresh = pkg.backend.Context(0)
    try:
        fresh.upload(scene.flatten())
        assert fresh.camera()[2] is False
        name_fresh = fresh.kernel_name(p)
        want = device_frame(fresh, p)
    finally:
        fresh.close()
    ctx.upload(scene.flatten())
    # a real turn first, rendered: whatever it leaves behind must not reach the fixed view's frames
    turned = pkg.backend.basis_turn(pkg.backend.FIXED_VIEW, 0.4, -0.1, 0.05)
    ctx.orient(turned)
    assert ctx.camera()[2] is True
    name_turned = ctx.kernel_name(p)
    assert name_turned != name_fresh and "_o::" in name_turned and "_o::" not in name_fresh
    device_frame(ctx, p)
    # the identity: from a look-at (its right.y is a -0 the cross product leaves), and as written
    for identity in (pkg.backend.basis_look_at((0., 0., 0.), (0., 0., -1.), (0., 1., 0.)), pkg.backend.FIXED_VIEW):
        ctx.orient(turned)
        ctx.orient(identity)
        pos, b, on = ctx.camera()
        assert on is False and basis_rows(b) == pkg.backend.FIXED_VIEW
        assert ctx.kernel_name(p) == name_fresh
        assert device_frame(ctx, p).tobytes() == want.tobytes(), "%s: the identity's frame differs from a fresh context's" % cfg
    ctx.orient(turned)
    device_frame(ctx, p)
    ctx.orient(None)
    assert ctx.camera()[2] is False and ctx.kernel_name(p) == name_fresh
    assert device_frame(ctx, p).tobytes() == want.tobytes(), "%s: the frame after orient(NULL) differs from a fresh context's" % cfg
    assert device_frame(ctx, p).tobytes() == want.tobytes()


# ---------------------------------------------------------------- 3. a turn invalidates carried state
def first_frame_of_a_fresh_context(pkg, scene, eye, basis, p):
    c = pkg.backend.Context(0)
    try:
        c.upload(scene.flatten())
        set_view(c, eye, basis)
        return device_frame(c, p, -2.)
    finally:
        c.close()


@pytest.mark.parametrize("move", [False, True], ids=["turn", "move-and-turn"])
def test_a_turn_invalidates_carried_state(pkg, flavour, move):
    """One context, 1080p, demo scene: twelve frames alternating between two views, then twelve of one (the standing view's
    reuse of its predecessor's order and classification, and the frozen launches, RM_ORDER_FREEZE): every frame is the first
    frame of a fresh context with that view, bit for bit, in buffers that held a sentinel."""
    w, h, depth = 1920, 1080, 5
    scene = workloads.product_scene(pkg, "demo")
    p = params(pkg, w, h, depth)
    eye_a, basis_a = view(pkg, (25., 10., 5.), (0., 0., -16.))
    eye_b, basis_b = view(pkg, (-30., 20., -16.) if move else (25., 10., 5.), (0., 0., -16.) if move else (3., -2., -20.))
    views = [(eye_a, basis_a), (eye_b, basis_b)]
    want = [first_frame_of_a_fresh_context(pkg, scene, e, b, p) for e, b in views]
    assert want[0].tobytes() != want[1].tobytes()
    rows = (h // 32) * 32
    for f in want:
        assert not (f[:rows] == -2.).any() and (f[rows:] == -2.).all()
    c = pkg.backend.Context(0)
    try:
        c.upload(scene.flatten())
        sequence = [k % 2 for k in range(12)] + [1] * 12 + [0] * 12
        for n, k in enumerate(sequence):
            set_view(c, *views[k])
            got = device_frame(c, p, -2.)
            assert got.tobytes() == want[k].tobytes(), "frame %d (view %d): %d pixels differ from a fresh context's first frame, %d left at the sentinel" % (
                n, k, int((got != want[k]).any(axis=2).sum()), int((got[:rows] == -2.).any(axis=2).sum()))
    finally:
        c.close()


# ---------------------------------------------------------------- 4. classification and order stay invisible
def test_classification_and_order_stay_invisible(pkg, O, cam, flavour, monkeypatch):
    import torch
    monkeypatch.setenv("RM_TILE_CLASSIFY", "0")
    plain = pkg.backend.Context(0)
    monkeypatch.delenv("RM_TILE_CLASSIFY")
    monkeypatch.setenv("RM_PATCH_ORDER", "0")
    unordered = pkg.backend.Context(0)
    monkeypatch.delenv("RM_PATCH_ORDER")
    default = pkg.backend.Context(0)
    demo, cornell = workloads.product_scene(pkg, "demo"), workloads.product_scene(pkg, "cornell")
    w, h = 1920, 1080
    rows = (h // 32) * 32
    cases = [("demo from above", demo, view(pkg, (0., 40., -15.), (0., 0., -16.), (0., 0., -1.))),
             ("demo from the side", demo, view(pkg, (25., 10., 5.), (0., 0., -16.))),
             ("cornell from the side", cornell, view(pkg, (600., 200., -100.), CORNELL_TARGET)),
             ("demo, facing away", demo, view(pkg, (0., 0., 0.), (0., 0., 1.)))]
    try:
        for label, scene, (eye, basis) in cases:
            p = params(pkg, w, h, 5)
            outs = []
            for c in (plain, unordered, default):
                c.upload(scene.flatten())
                set_view(c, eye, basis)
                f64 = torch.full((h, w, 3), -1., dtype=torch.float64, device="cuda:0")
                u8 = torch.full((h, w, 3), 201, dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                c.render_device_u8(p, f64.data_ptr(), u8.data_ptr())
                c.render_device_u8(p, f64.data_ptr(), u8.data_ptr())      # (a second frame: the counters take turns)
                torch.cuda.synchronize()
                outs.append((f64.cpu().numpy(), u8.cpu().numpy()))
            for k, who in ((1, "RM_PATCH_ORDER=0"), (2, "defaults")):
                assert outs[0][0].tobytes() == outs[k][0].tobytes(), "%s: f64 frame under %s differs from RM_TILE_CLASSIFY=0" % (label, who)
                assert np.array_equal(outs[0][1], outs[k][1]), "%s: display bytes under %s differ" % (label, who)
            assert not (outs[2][0][:rows] == -1.).any() and (outs[2][0][rows:] == -1.).all()
            tiles, listed = default.tile_stats()
            print("%s: %d of %d tiles listed" % (label, listed, tiles))
            assert tiles == rows * w // 64
            if label == "demo from above":
                assert 0 < listed < tiles, "the classification keeps every tile of the view from above"
            if label == "demo, facing away":
                # all zeros in the oracle (a quarter-size frame of the same view, every pixel) and on the GPU; no tile listed
                ref = cam.frame("demo", workloads.oracle_scene(O, "demo"), eye, basis_rows(basis), 480, 288, 5)
                assert not ref.any()
                assert not outs[2][0][:rows].any() and not outs[2][1][:rows].any()
                assert listed == 0
    finally:
        for c in (plain, unordered, default):
            c.close()


# ---------------------------------------------------------------- 5. pixel queries follow the camera
@pytest.mark.parametrize("name,v,w,h", [("demo", DEMO_VIEWS[0], 640, 360), ("demo", DEMO_VIEWS[5], 640, 360),
                                        ("cornell", ("side", (600., 200., -100.), CORNELL_TARGET, (0., 1., 0.), 0.), 640, 360),
                                        ("synthetic256", ("down", (0., 45., -41.), (0., 2., -41.), (0., 0., -1.), 0.), 512, 512)],
                         ids=["demo-right-front", "demo-rolled", "cornell-side", "spheres-down"])
def test_pixel_queries_follow_the_camera(pkg, O, ctx, cam, fixed_view_after, name, v, w, h):
    import torch
    _, eye, target, up, roll = v
    eye, basis = view(pkg, eye, target, up, roll)
    scene, oscene = workloads.product_scene(pkg, name), workloads.oracle_scene(O, name)
    handle = scene.flatten()
    ctx.upload(handle)
    desc = handle.desc()
    set_view(ctx, eye, basis)
    p = params(pkg, w, h, 5, flags=0)
    sentinel = -7.25
    out = torch.full((h, w, 9), sentinel, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.primary_hits_device(p, out=out)
    torch.cuda.synchronize()
    rows = (h // 32) * 32
    raw = out.cpu().numpy()
    assert (raw[rows:] == sentinel).all(), "the rows below the last whole patch row were written"
    rec = raw[:rows].reshape(-1).view(pkg.backend.HIT_DTYPE).reshape(rows, w)
    ref_hit, ref_shape, ref_pn = cam.hits(oscene, eye, basis_rows(basis), w, h)
    assert np.array_equal(rec["hit"], ref_hit), "%d hit / miss decisions differ" % int((rec["hit"] != ref_hit).sum())
    m = ref_hit == 1
    assert m.mean() > LIT_FLOOR
    assert np.array_equal(rec["shape"][m] % 256, ref_shape[m])
    assert np.abs(rec["point"][m] - ref_pn[..., :3][m]).max(initial=0.) < TIGHT
    assert np.abs(rec["normal"][m] - ref_pn[..., 3:6][m]).max(initial=0.) < TIGHT
    # t places the point on the oracle's ray; a miss is all zeros
    d = ref_pn[..., 6:9]
    o = np.asarray(eye)
    assert np.abs(o + d[m] * rec["t"][m][:, None] - rec["point"][m]).max(initial=0.) < 1e-9 * (1. + np.abs(rec["point"][m]).max(initial=0.))
    assert not rec[~m].view(np.float64).reshape(-1, 9).any()
    # the element: the triangle of the mesh that alone gives the oracle's point (0 for spheres and polygons)
    counts = [desc.shapes[i].count for i in range(desc.n_shapes)]
    kinds = [desc.shapes[i].kind for i in range(desc.n_shapes)]
    ys, xs = np.nonzero(m)
    rng = np.random.default_rng(w * h)
    shapes = oscene.c.shapes
    for i in rng.choice(len(ys), size=min(len(ys), 1500), replace=False):
        y, x = int(ys[i]), int(xs[i])
        sh, el = int(rec["shape"][y, x]), int(rec["element"][y, x])
        if kinds[sh] != pkg._lib.RM_SHAPE_SPHERE and kinds[sh] != pkg._lib.RM_SHAPE_POLYGON:
            assert el < counts[sh]
            alone = O.Intersection()
            assert O.lib().orc_triangle_intersect(C.byref(shapes[sh].triangles[el]), O.v3(o), O.v3(d[y, x]), C.byref(alone)) == 1
            assert alone.point.tup() == tuple(ref_pn[y, x, :3]), "pixel (%d, %d): triangle %d of shape %d is not the one hit" % (x, y, el, sh)
        else:
            assert el == 0
    # the frame of the same view: a miss exactly where the pixel is zero
    frame = np.zeros((h, w, 3))
    ctx.render(p, frame)
    lit = frame[:rows].max(axis=2) > 0.
    assert np.array_equal(lit, m), "%d pixels where the frame and the hit buffer disagree" % int((lit != m).sum())
    assert (frame[:rows][~m] == 0.).all()
    # rm_pick is the buffer's entry, bit for bit; the strip below the patch rows is answered too
    for x, y in list(zip(rng.integers(0, w, 40), rng.integers(0, rows, 40))) + [(0, 0), (w - 1, rows - 1), (w // 2, h // 2)]:
        pk = ctx.pick(p, int(x), int(y))
        assert bytes(pk) == rec[y, x].tobytes(), (x, y)
    if rows < h:
        y = h - 1
        dlast = cam.directions(basis_rows(basis), w, h, rows=h)[y:y + 1, 5:6]
        _, rh, rs, _ = cam._rays(oscene, eye, dlast, 1, False, True)
        pk = ctx.pick(p, 5, y)
        assert pk.hit == rh[0] and (not pk.hit or pk.shape % 256 == rs[0])
    print("%s %s %dx%d: %d of %d pixels hit" % (name, v[0], w, h, int(m.sum()), m.size))


def test_renderer_applies_the_scenes_basis(pkg, O, cam):
    """Renderer.render / Renderer.pick hand Scene.basis to the shared default context on every call; None resets."""
    w, h, depth = 256, 160, 5
    r = pkg.create_renderer(workloads.FOV, float(h), float(w))
    r.max_depth = depth
    scene = workloads.product_scene(pkg, "demo")
    plain = pkg.create_frame_buffer(w, h)
    r.render(plain, scene)
    scene.camera = pkg.Vec3f(25., 10., 5.)
    scene.look_at((0., 0., -16.))
    fb = pkg.create_frame_buffer(w, h)
    r.render(fb, scene)
    eye = (25., 10., 5.)
    ref = cam.frame("demo", workloads.oracle_scene(O, "demo"), eye, basis_rows(scene.basis), w, h, depth)
    assert np.abs(fb.buffer[:(h // 32) * 32] - ref).max() < TIGHT
    hit_ref, shape_ref, _ = cam.hits(workloads.oracle_scene(O, "demo"), eye, basis_rows(scene.basis), w, h)
    ys, xs = np.nonzero(hit_ref == 1)
    k = len(ys) // 2
    pk = r.pick(fb, scene, int(xs[k]), int(ys[k]))
    assert pk is not None and pk.shape % 256 == shape_ref[ys[k], xs[k]]
    # a scene without a basis after one with: the fixed view again
    again = pkg.create_frame_buffer(w, h)
    r.render(again, workloads.product_scene(pkg, "demo"))
    assert again.buffer.tobytes() == plain.buffer.tobytes()


# ---------------------------------------------------------------- 6. every seam
def test_every_seam_honours_the_view(pkg, O, flavour):
    import torch
    w, h, depth = 640, 360, 5
    rows = (h // 32) * 32
    scene = workloads.product_scene(pkg, "demo")
    eye, basis = view(pkg, (-30., 20., -16.), (0., 0., -16.), roll=0.3)
    c = pkg.backend.Context(0)
    try:
        c.upload(scene.flatten())
        set_view(c, eye, basis)
        p = params(pkg, w, h, depth)
        want = np.full((h, w, 3), -4.)
        c.render(p, want)
        assert (want[rows:] == -4.).all() and not (want[:rows] == -4.).any() and (want[:rows].max(axis=2) > 0.).mean() > LIT_FLOOR
        # rm_render_rows: a FrameBuffer of rows of their own
        row_arrays = [np.full(w * 3, -4.) for _ in range(h)]
        c.render_rows(p, row_arrays)
        assert np.stack(row_arrays).reshape(h, w, 3).tobytes() == want.tobytes()
        # rm_render_display: fb.to_vec() of the frame
        u8 = np.full((h, w, 3), 201, np.uint8)
        c.render_display(p, u8)
        want8 = O.to_vec(want[:rows].copy()).reshape(rows, w, 3)
        n_diff = int((u8[:rows] != want8).sum())
        print("render_display: %d display bytes differ from to_vec of the f64 frame" % n_diff)
        assert n_diff == 0 and (u8[rows:] == 201).all()
        # rm_render_device_u8, whole frame and a strided band packed
        f64 = torch.full((h, w, 3), -4., dtype=torch.float64, device="cuda:0")
        d8 = torch.full((h, w, 3), 201, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        c.render_device_u8(p, f64.data_ptr(), d8.data_ptr())
        torch.cuda.synchronize()
        assert f64.cpu().numpy().tobytes() == want.tobytes()
        assert np.array_equal(d8.cpu().numpy()[:rows], want8) and (d8.cpu().numpy()[rows:] == 201).all()
        band = (1, 11, 3)                                                  # patch rows 1, 4, 7, 10
        pb = params(pkg, w, h, depth, band, flags=_FLAGS["value"] | RM_FLAG_U8_COMPACT)
        f64 = torch.full((h, w, 3), -4., dtype=torch.float64, device="cuda:0")
        d8 = torch.full((4 * 32, w, 3), 201, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        c.render_device_u8(pb, f64.data_ptr(), d8.data_ptr())
        torch.cuda.synchronize()
        got, got8 = f64.cpu().numpy(), d8.cpu().numpy()
        for k, row in enumerate(range(1, 11, 3)):
            assert got[row * 32:(row + 1) * 32].tobytes() == want[row * 32:(row + 1) * 32].tobytes()
            assert np.array_equal(got8[k * 32:(k + 1) * 32], want8[row * 32:(row + 1) * 32])
        owned = np.zeros(h, bool)
        for row in range(1, 11, 3):
            owned[row * 32:(row + 1) * 32] = True
        assert (got[~owned] == -4.).all()
        # rm_frame_submit_f64, a world of one
        c.comm_init(0, 1)
        _, chunk = c.exchange_layout(p, 1)
        gathered = torch.full((chunk,), -3., dtype=torch.float64, device="cuda:0")
        frame = torch.full((rows, w, 3), -5., dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        c.frame_submit_f64(p, gathered.data_ptr(), frame.data_ptr(), slot=0)
        c.frame_wait(0, timeout_ms=20000)
        assert frame.cpu().numpy().tobytes() == want[:rows].tobytes()
        assert gathered.cpu().numpy()[:rows * w * 3].tobytes() == want[:rows].tobytes()
    finally:
        c.close()


# ---------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_state_unchanged(pkg, ctx, fixed_view_after):
    B, L = pkg._lib, pkg.lib()
    scene = workloads.product_scene(pkg, "demo")
    ctx.upload(scene.flatten())
    eye, basis = view(pkg, (10., 3., 10.), (-5., 0., -20.))
    ctx.look_at(eye, (-5., 0., -20.))
    pos, b, on = ctx.camera()
    assert on is True and (pos.x, pos.y, pos.z) == eye and basis_rows(b) == basis_rows(basis)
    p = params(pkg, 256, 160, 5, flags=0)
    want = device_frame(ctx, p)

    def unchanged():
        pos2, b2, on2 = ctx.camera()
        assert on2 is True and (pos2.x, pos2.y, pos2.z) == eye and basis_rows(b2) == basis_rows(basis)
        assert device_frame(ctx, p).tobytes() == want.tobytes()

    m = np.array(basis_rows(basis))
    skew = m.copy(); skew[0] = skew[0] + 1e-6 * skew[1]
    scaled = m * 1.0001
    nan = m.copy(); nan[2, 1] = float("nan")
    for bad in (skew, scaled, nan):
        with pytest.raises(pkg.BackendError):
            ctx.orient(tuple(map(tuple, bad)))
        unchanged()
    with pytest.raises(pkg.BackendError):
        ctx.look_at((1., 2., 3.), (1., 2., 3.))
    unchanged()
    with pytest.raises(pkg.BackendError):
        ctx.look_at((1., 2., 3.), (1., 7., 3.), up=(0., 1., 0.))
    unchanged()
    assert b"rm_camera_look_at" in L.rm_last_error(ctx.ptr)
    # a left-handed basis is accepted: the mirrored picture
    mirrored = (tuple(-c for c in basis_rows(basis)[0]),) + basis_rows(basis)[1:]
    ctx.orient(mirrored)
    assert device_frame(ctx, p).tobytes() != want.tobytes()
    got = ctx.camera()
    assert got[2] is True and basis_rows(got[1]) == mirrored
    # the state survives an upload; the position is the scene's again
    scene.camera = pkg.Vec3f(1., 2., 3.)
    ctx.upload(scene.flatten())
    pos, b, on = ctx.camera()
    assert on is True and basis_rows(b) == mirrored and (pos.x, pos.y, pos.z) == (1., 2., 3.)
    # look_at needs a scene, as rm_camera_update does; orient does not
    fresh = pkg.backend.Context(0)
    try:
        with pytest.raises(pkg.BackendError):
            fresh.look_at((0., 0., 0.), (0., 0., -1.))
        fresh.orient(basis)
        assert fresh.camera()[2] is True
    finally:
        fresh.close()
