"""Ranged ray queries on the GPU (-m gpu): rm_intersect_rays_ranged / rm_occluded_rays_ranged / rm_visible_segments /
rm_lights_visible and their device variants, through the C ABI.

Yardsticks: the unranged queries (byte for byte with the range [0, +inf]), tests/ranged_reference.py (the numpy restatement
of the range rule, pinned to the oracle by tests/test_ranged_abi.py) and the oracle's own intersect_shape_set for the lights
as rendered.  Decisions and the ray parameter must be the yardstick's exactly: both sides are IEEE binary64, one rounding per
operation, in the reference's order.  A ray is left out of a comparison only where the helper finds a candidate within 1e-9
(relative) of an end of its range, and at most 1 % of the rays may be (the seeds below were chosen on the CPU: the helper
alone leaves out none)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ranged_reference as RR
import test_gpu_query as GQ
import workloads

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 4097)          # the wave tails: one lane, a wave less one, a wave, a wave and one, 64 waves and one
N = 4097
SCENES = ("demo", "cornell", "synthetic256")   # plain walk, triangle hierarchy, sphere hierarchy
SEEDS = {"demo": 101, "cornell": 102, "synthetic256": 103}
LEFT_OUT_CAP = 0.01
FULL = (0., np.inf)


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batch(O, entry, tmp_path_factory):
    d = tmp_path_factory.mktemp("orc_batch_ranged_gpu")
    src, so = d / "orc_batch.c", d / "orc_batch.so"
    src.write_text(GQ.BATCH_C)
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-shared", "-fPIC",
                           "-I", os.path.join(entry.ROOT, "oracle"), str(src), "-o", str(so)])
    return GQ.OracleBatch(O, C.CDLL(str(so)))


class Loaded:
    """A workload scene as the product holds it, its flat description and the numpy yardstick built from that."""

    def __init__(self, pkg, name):
        self.scene = workloads.product_scene(pkg, name)
        self.handle = self.scene.flatten()
        self.desc = self.handle.desc()
        self.ref = RR.Scene(self.desc)


@pytest.fixture(scope="module")
def loaded(pkg):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Loaded(pkg, name)
        return cache[name]
    return get


def ranged_rays(name, desc, n=N):
    """n rays and ranges of the scene: origins in the padded bounds, a third of them inside a sphere (between the walls for
    the Cornell box, whose rays also aim at its triangles: blind ones find few); t_min uniform in [0, 30], t_max = t_min + an
    exponential of mean 40, one ray in ten +inf."""
    rng = np.random.default_rng(SEEDS[name])
    lo, hi = GQ.bounds_of(desc)
    o, d = GQ.random_rays(rng, n, lo, hi)
    k = n // 3
    if desc.n_spheres:
        o[:k] = GQ.inside_spheres(rng, desc, k)
    else:
        tri = np.array([[[v.x, v.y, v.z] for v in desc.triangles[i].vertices] for i in range(desc.n_triangles)])
        flat = tri.reshape(-1, 3)
        o[:k] = rng.uniform(flat.min(axis=0), flat.max(axis=0), size=(k, 3))            # between the walls
        pick, b = rng.integers(0, len(tri), 2 * k), rng.dirichlet((1., 1., 1.), 2 * k)
        d[:2 * k] = GQ.unit((tri[pick] * b[:, :, None]).sum(axis=1) - o[:2 * k])
    t_min = rng.uniform(0., 30., n)
    t_max = t_min + rng.exponential(40., n)
    t_max[rng.uniform(size=n) < 0.1] = np.inf
    return o, d, np.stack([t_min, t_max], axis=1)


def kept(near_end, label):
    keep = ~near_end
    left_out = int(near_end.sum())
    print("%s: %d of %d left out (a candidate within 1e-9 of an end of the range)" % (label, left_out, near_end.size))
    assert left_out <= LEFT_OUT_CAP * near_end.size, "%s: %d rays left out, more than 1 %%" % (label, left_out)
    return keep


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


# ---------------------------------------------------------------- 1. the full range is the unranged query
@pytest.mark.parametrize("name", SCENES)
def test_full_range_equals_the_unranged_queries(ctx, loaded, name):
    import torch
    s = loaded(name)
    ctx.upload(s.handle)
    o, d, _ = ranged_rays(name, s.desc)
    for n in COUNTS:
        plain, plain_occ = ctx.intersect(o[:n], d[:n]), ctx.occluded(o[:n], d[:n])
        ranged = ctx.intersect(o[:n], d[:n], ranges=FULL)
        assert ranged.tobytes() == plain.tobytes(), "%s, %d rays: rm_hit bytes differ" % (name, n)
        assert ctx.occluded(o[:n], d[:n], ranges=FULL).tobytes() == plain_occ.tobytes()
        # ... per-ray ranges, and the device variants on a stream of their own
        r = np.tile(FULL, (n, 1))
        assert ctx.intersect(o[:n], d[:n], ranges=r).tobytes() == plain.tobytes()
        st = torch.cuda.Stream()
        to, td, tr = to_dev(o[:n]), to_dev(d[:n]), to_dev(r)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            dh = ctx.intersect_device(to, td, ranges=tr)
            docc = ctx.occluded_device(to, td, ranges=FULL)
        st.synchronize()
        assert dh.raw.cpu().numpy().tobytes() == plain.tobytes()
        assert np.array_equal(docc.cpu().numpy(), plain_occ)
    print("%s: %d of %d rays hit over the full range" % (name, int(plain["hit"].sum()), N))
    assert plain["hit"].sum() > 0.05 * N


# ---------------------------------------------------------------- 2. random ranges against the helper
@pytest.mark.parametrize("name", SCENES)
def test_random_ranges_match_the_helper(ctx, loaded, name):
    s = loaded(name)
    ctx.upload(s.handle)
    o, d, r = ranged_rays(name, s.desc)
    ref = s.ref.closest(o, d, r)
    ref_occ, near_occ = s.ref.occluded(o, d, r)
    keep = kept(ref["near_end"] | near_occ, name)
    g = ctx.intersect(o, d, ranges=r)
    occ = ctx.occluded(o, d, ranges=r)
    assert np.array_equal(g["hit"][keep], ref["hit"][keep]), "%d hit / miss decisions differ" % int((g["hit"] != ref["hit"])[keep].sum())
    assert np.array_equal(occ[keep], ref_occ[keep]), "%d occlusion decisions differ" % int((occ != ref_occ)[keep].sum())
    m = keep & (ref["hit"] == 1)
    for f in ("shape", "element", "t"):
        assert np.array_equal(g[f][m], ref[f][m]), "%s: %d rays differ in %s" % (name, int((g[f][m] != ref[f][m]).sum()), f)
    assert np.array_equal(g["point"][m], ref["point"][m]) and np.array_equal(g["normal"][m], ref["normal"][m])
    assert np.all((g["t"][m] >= r[m, 0]) & (g["t"][m] <= r[m, 1]))
    assert not g[g["hit"] == 0].view(np.float64).reshape(-1, 9).any()          # a miss is all zeros
    # the range matters: these rays' unranged answers differ for a good part of them
    plain = ctx.intersect(o, d)
    differ = int(((plain["hit"] != g["hit"]) | (plain["t"] != g["t"])).sum())
    far_root = int((m & (ref["t"] > 0.) & (plain["hit"] == 1) & (plain["shape"] == g["shape"]) & (plain["t"] < g["t"])).sum())
    print("%s: %d of %d hit in their range, %d occluded; %d answers differ from the unranged ones, %d at a far root" %
          (name, int(ref["hit"].sum()), N, int(ref_occ.sum()), differ, far_root))
    assert ref["hit"].sum() > 40 and differ > 100


# ---------------------------------------------------------------- 3. the far root
def test_a_sphere_is_hit_at_its_far_root(pkg, ctx):
    s = pkg.Scene.new()
    s.shapes.append(pkg.sphere.create(pkg.Vec3f(0., 0., -10.), 2., pkg.Reflectance()))
    ctx.upload(s.flatten())
    o = np.array([[0., 0., 0.], [0., 0., 0.], [0., 0., 0.], [0., 0., -10.], [0., 0., 0.], [0., 0., 0.]])
    d = np.tile([0., 0., -1.], (6, 1))
    #               t_min between the roots; t_max below t0; strictly between the roots; inside; the roots themselves (closed)
    r = np.array([[9., np.inf], [0., 7.], [9., 11.], [0., np.inf], [8., 8.], [12., 12.]])
    want_hit, want_t = [1, 0, 0, 1, 1, 1], [12., 0., 0., 2., 8., 12.]
    for n in (6, 1):
        g = ctx.intersect(o[:n], d[:n], ranges=r[:n])
        assert g["hit"].tolist() == want_hit[:n] and g["t"].tolist() == want_t[:n]
        assert ctx.occluded(o[:n], d[:n], ranges=r[:n]).tolist() == [bool(h) for h in want_hit[:n]]
    assert g["point"][0].tolist() == [0., 0., -12.] and g["normal"][0].tolist() == [0., 0., -1.]     # the normal of THAT point
    g = ctx.intersect(o, d, ranges=r)
    assert g["normal"][3].tolist() == [0., 0., -1.] and g["normal"][4].tolist() == [0., 0., 1.]
    assert g["shape"].tolist() == [0] * 6 and g["element"].tolist() == [0] * 6
    import torch
    dh = ctx.intersect_device(to_dev(o), to_dev(d), ranges=to_dev(r))
    docc = ctx.occluded_device(to_dev(o), to_dev(d), ranges=to_dev(r))
    torch.cuda.synchronize()
    assert dh.raw.cpu().numpy().tobytes() == g.tobytes() and docc.cpu().numpy().tolist() == [bool(h) for h in want_hit]


# ---------------------------------------------------------------- 4. segments
def primary_points(pkg, ctx, s, cam=None):
    """Points and normals under the pixels of a 128 x 64 frame of the uploaded scene (rm_primary_hits_device)."""
    import torch
    if cam is not None:
        ctx.set_camera(cam)
    p = pkg.backend.make_params(workloads.FOV, 64., 128., 3)
    hits = ctx.primary_hits_device(p)
    torch.cuda.synchronize()
    rec = hits.raw.cpu().numpy().reshape(-1).view(pkg.backend.HIT_DTYPE)
    rec = rec[rec["hit"] == 1]
    return np.ascontiguousarray(rec["point"]), np.ascontiguousarray(rec["normal"])


def test_segments_between_the_points_of_a_frame(pkg, ctx, loaded):
    import torch
    s = loaded("demo")
    ctx.upload(s.handle)
    pts, _ = primary_points(pkg, ctx, s)
    assert len(pts) > 1000
    rng = np.random.default_rng(4)
    i, j = rng.integers(0, len(pts), N), rng.integers(0, len(pts), N)
    j = np.where(np.all(pts[i] == pts[j], axis=1), (j + 1) % len(pts), j)
    a, b = pts[i], pts[j]
    want, near = s.ref.visible(a, b, 1e-3)
    keep = kept(near, "segments")
    got = ctx.visible(a, b, 1e-3)
    assert np.array_equal(got[keep], want[keep]), "%d segments differ" % int((got != want)[keep].sum())
    print("segments: %d of %d see each other" % (int(want.sum()), N))
    assert 0.02 * N < want.sum() < 0.98 * N
    # the device variant is the host variant, whatever the tail of the last wave
    for n in COUNTS:
        st = torch.cuda.Stream()
        ta, tb = to_dev(a[:n]), to_dev(b[:n])
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            dv = ctx.visible_device(ta, tb, 1e-3)
        st.synchronize()
        assert dv.dtype == torch.bool and np.array_equal(dv.cpu().numpy(), got[:n] if n == N else ctx.visible(a[:n], b[:n], 1e-3))
    # by hand: across a sphere, up to its front, and a skin that eats the whole segment
    sp = s.desc.spheres[0]
    c, rad = np.array([sp.center.x, sp.center.y, sp.center.z]), np.sqrt(sp.radius_square)
    x = np.array([1., 0., 0.])
    frm = np.array([c + (rad + 1.) * x] * 3)
    to = np.array([c - (rad + 1.) * x, c + (rad + 0.5) * x, c - (rad + 1.) * x])
    assert s.ref.visible(frm[:2], to[:2], 0.)[0].tolist() == [False, True]
    assert ctx.visible(frm[:2], to[:2]).tolist() == [False, True]
    assert ctx.visible(frm[2:], to[2:], skin=rad + 1.5).tolist() == [True]                # L - skin < skin: empty, visible
    assert ctx.visible(frm[2:], to[2:], skin=0.25).tolist() == [False]


# ---------------------------------------------------------------- 5. lights
@pytest.mark.parametrize("name,cam", [("demo", None), ("cornell", (20., 30., -50.))])
def test_lights_as_rendered_are_the_oracles_shadow_decisions(pkg, O, ctx, batch, loaded, name, cam):
    import torch
    s = loaded(name)
    ctx.upload(s.handle)
    pts, nrm = primary_points(pkg, ctx, s, cam)
    assert len(pts) > 500
    oscene = workloads.oracle_scene(O, name)
    so, sd, _ = s.ref.shadow_rays(pts, nrm)                       # renderer.rs:166-172, in numpy
    shadowed = batch.occluded(oscene, so.reshape(-1, 3), sd.reshape(-1, 3)).astype(bool).reshape(len(pts), -1)
    lit = ctx.lights_visible(pts, nrm)
    assert lit.shape == (len(pts), s.desc.n_lights) and lit.dtype == np.bool_
    assert np.array_equal(lit, ~shadowed), "%d of %d light decisions differ from intersect_shape_set" % (int((lit == shadowed).sum()), lit.size)
    want, near = s.ref.lights_visible(pts, nrm, clipped=True)
    keep = kept(near, "%s lights, clipped" % name)
    clipped = ctx.lights_visible(pts, nrm, clipped=True)
    assert np.array_equal(clipped[keep], want[keep])
    assert not (lit & ~clipped).any(), "a light that reaches the point as rendered does not reach it clipped"
    print("%s: %d points x %d lights: %d lit as rendered, %d clipped" % (name, len(pts), lit.shape[1], int(lit.sum()), int(clipped.sum())))
    assert lit.any() and (name != "demo" or not lit.all())            # (nothing in the Cornell box stands between its points and the lights)
    tp, tn = to_dev(pts), to_dev(nrm)
    d0, d1 = ctx.lights_visible_device(tp, tn), ctx.lights_visible_device(tp, tn, clipped=True)
    torch.cuda.synchronize()
    assert np.array_equal(d0.cpu().numpy(), lit) and np.array_equal(d1.cpu().numpy(), clipped)


def test_a_shape_behind_the_light_shadows_as_rendered_and_not_clipped(pkg, ctx):
    """The header's caveat: a floor, a light above it, a sphere above the light."""
    s = pkg.Scene.new()
    s.shapes.append(pkg.polygon.ConvexPolygon.create([pkg.Vec3f(*v) for v in [(-20., -3., 0.), (20., -3., 0.), (20., -3., -40.), (-20., -3., -40.)]],
                                                     pkg.Reflectance()))
    s.shapes.append(pkg.sphere.create(pkg.Vec3f(0., 10., -10.), 2., pkg.Reflectance()))
    s.shapes.append(pkg.sphere.create(pkg.Vec3f(30., 0., -10.), 1., pkg.Reflectance()))
    s.lights.append(pkg.create_light(pkg.Vec3f(0., 5., -10.), pkg.Vec3f(1., 1., 1.), 1.))
    ctx.upload(s.flatten())
    pts = np.array([[0., -3., -10.], [10., -3., -10.]])             # under the light and the sphere; well to the side
    nrm = np.tile([0., 1., 0.], (2, 1))
    assert ctx.lights_visible(pts, nrm).tolist() == [[False], [True]]
    assert ctx.lights_visible(pts, nrm, clipped=True).tolist() == [[True], [True]]
    for n in (1, 63, 64, 65):                                       # the tails of the (point, light) lanes
        many = ctx.lights_visible(np.tile(pts[0], (n, 1)), np.tile(nrm[0], (n, 1)))
        assert many.shape == (n, 1) and not many.any()


# ---------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_outputs_alone(pkg, ctx, loaded):
    L, B = pkg.lib(), pkg._lib
    E = B.RM_ERR_INVALID_ARG
    s = loaded("demo")
    ctx.upload(s.handle)
    n = 4
    V, R = B.rm_vec3 * n, B.rm_range * n
    zero = V(*[B.rm_vec3(0., 0., 0.)] * n)
    down = V(*[B.rm_vec3(0., 0., -1.)] * n)
    ahead = V(*[B.rm_vec3(0., 0., -5.)] * n)
    up = V(*[B.rm_vec3(0., 1., 0.)] * n)
    good = R(*[B.rm_range(0., 10.)] * n)

    def out_bytes(size):
        return (C.c_uint8 * size)(*([0x5A] * size))

    def untouched(buf):
        return bytes(buf) == b"\x5A" * len(bytes(buf))

    def ranges_with(bad):
        r = R(*[B.rm_range(0., 10.)] * n)
        r[2] = B.rm_range(*bad)
        return r

    def vecs_with(base, bad):
        v = V(*[B.rm_vec3(*base)] * n)
        v[2] = B.rm_vec3(*bad)
        return v

    hits, occ = out_bytes(n * 72), out_bytes(n)
    as_hits = C.cast(hits, C.POINTER(B.rm_hit))
    for bad in ((np.nan, 1.), (0., np.nan), (-1e-9, 1.), (5., 4.)):          # a NaN range, t_min < 0, t_max < t_min
        assert L.rm_intersect_rays_ranged(ctx.ptr, zero, down, ranges_with(bad), n, as_hits) == E
        assert b"ray 2" in L.rm_last_error(ctx.ptr)
        assert L.rm_occluded_rays_ranged(ctx.ptr, zero, down, ranges_with(bad), n, occ) == E
    assert L.rm_intersect_rays_ranged(ctx.ptr, zero, vecs_with((0., 0., -1.), (0., 0., -1.01)), good, n, as_hits) == E    # what check_rays checks
    assert L.rm_occluded_rays_ranged(ctx.ptr, vecs_with((0., 0., 0.), (np.inf, 0., 0.)), down, good, n, occ) == E
    # segments: from == to, a non-finite endpoint, a negative or non-finite skin
    assert L.rm_visible_segments(ctx.ptr, zero, vecs_with((0., 0., -5.), (0., 0., 0.)), n, 0., occ) == E
    assert b"segment 2" in L.rm_last_error(ctx.ptr)
    assert L.rm_visible_segments(ctx.ptr, zero, vecs_with((0., 0., -5.), (np.nan, 0., 0.)), n, 0., occ) == E
    for skin in (-1e-3, np.inf, np.nan):
        assert L.rm_visible_segments(ctx.ptr, zero, ahead, n, skin, occ) == E
    # lights: a zero normal, a non-finite point, a wrong n_lights, mode 2
    nl = s.desc.n_lights
    lit = out_bytes(n * (nl + 1))
    assert L.rm_lights_visible(ctx.ptr, ahead, vecs_with((0., 1., 0.), (0., 0., 0.)), n, nl, 0, lit) == E
    assert b"point 2" in L.rm_last_error(ctx.ptr)
    assert L.rm_lights_visible(ctx.ptr, vecs_with((0., 0., -5.), (0., np.inf, 0.)), up, n, nl, 1, lit) == E
    assert L.rm_lights_visible(ctx.ptr, ahead, up, n, nl + 1, 0, lit) == E
    assert L.rm_lights_visible(ctx.ptr, ahead, up, n, nl, 2, lit) == E
    assert L.rm_lights_visible_device(ctx.ptr, None, None, n, nl + 1, 0, None, None) == E
    assert L.rm_lights_visible_device(ctx.ptr, None, None, n, nl, 2, None, None) == E
    assert L.rm_visible_segments_device(ctx.ptr, None, None, n, -1., None, None) == E
    assert untouched(hits) and untouched(occ) and untouched(lit), "a refused call wrote into its output"
    # n == 0 does nothing
    assert L.rm_intersect_rays_ranged(ctx.ptr, None, None, None, 0, None) == 0
    assert L.rm_occluded_rays_ranged_device(ctx.ptr, None, None, None, 0, None, None) == 0
    assert L.rm_visible_segments(ctx.ptr, None, None, 0, 0., None) == 0
    assert L.rm_lights_visible(ctx.ptr, None, None, 0, nl, 0, None) == 0
    assert L.rm_lights_visible_device(ctx.ptr, None, None, 0, nl, 1, None, None) == 0
    # ... and the good calls are answered
    assert L.rm_intersect_rays_ranged(ctx.ptr, zero, down, good, n, as_hits) == 0 and not untouched(hits)
    assert L.rm_visible_segments(ctx.ptr, zero, ahead, n, 0., occ) == 0 and not untouched(occ)
    assert L.rm_lights_visible(ctx.ptr, ahead, up, n, nl, 1, lit) == 0
    assert bytes(lit)[n * nl:] == b"\x5A" * n and not untouched(lit)                    # n_points x n_lights bytes, no more
    # no scene: every entry point says so, without an upload of its own
    fresh = pkg.backend.Context(0)
    NS = B.RM_ERR_NO_SCENE
    assert L.rm_intersect_rays_ranged(fresh.ptr, zero, down, good, n, as_hits) == NS
    assert L.rm_occluded_rays_ranged(fresh.ptr, zero, down, good, n, occ) == NS
    assert L.rm_intersect_rays_ranged_device(fresh.ptr, None, None, None, n, None, None) == NS
    assert L.rm_occluded_rays_ranged_device(fresh.ptr, None, None, None, n, None, None) == NS
    assert L.rm_visible_segments(fresh.ptr, zero, ahead, n, 0., occ) == NS
    assert L.rm_visible_segments_device(fresh.ptr, None, None, n, 0., None, None) == NS
    assert L.rm_lights_visible(fresh.ptr, ahead, up, n, nl, 0, lit) == NS
    assert L.rm_lights_visible_device(fresh.ptr, None, None, n, nl, 0, None, None) == NS
    assert fresh.uploads() == (0, 0)
    fresh.close()
    # a scene without lights: RM_OK, nothing written
    dark = pkg.Scene.new()
    dark.shapes.append(pkg.sphere.create(pkg.Vec3f(0., 0., -10.), 2., pkg.Reflectance()))
    ctx.upload(dark.flatten())
    lit = out_bytes(n)
    assert L.rm_lights_visible(ctx.ptr, ahead, up, n, 0, 0, lit) == 0 and untouched(lit)
    assert L.rm_lights_visible(ctx.ptr, ahead, up, n, 1, 0, lit) == E and untouched(lit)
    assert ctx.lights_visible(np.zeros((3, 3)), np.tile([0., 1., 0.], (3, 1))).shape == (3, 0)


# ---------------------------------------------------------------- 7. render state
def test_ranged_queries_do_not_disturb_the_frames(pkg, loaded):
    import torch
    s = loaded("demo")
    o, d, r = ranged_rays("demo", s.desc, 1000)
    pts = np.array([[0., -3., -10.], [3., -3., -20.]])
    nrm = np.tile([0., 1., 0.], (2, 1))

    def queries(c):
        c.intersect(o, d, ranges=r)
        c.occluded(o, d, ranges=r)
        c.visible(o[:500], o[500:], 1e-3)
        c.lights_visible(pts, nrm)
        c.lights_visible(pts, nrm, clipped=True)
        st = torch.cuda.Stream()
        to, td, tr = to_dev(o), to_dev(d), to_dev(r)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            c.intersect_device(to, td, ranges=tr)
            c.occluded_device(to, td, ranges=tr)
            c.visible_device(to[:500], to[500:], 1e-3)
            c.lights_visible_device(to_dev(pts), to_dev(nrm), clipped=True)
        st.synchronize()

    def frames(with_queries):
        c = pkg.backend.Context(0)
        c.upload(s.handle)
        p = pkg.backend.make_params(workloads.FOV, 256., 512., 5)
        out = []
        for step in range(2):
            if step == 1:
                c.set_camera((5., 0., 0.))
                if with_queries:
                    queries(c)
            f = np.zeros((256, 512, 3))
            c.render(p, f)
            out.append(f)
        c.close()
        return out

    plain, queried = frames(False), frames(True)
    for k, (a, b) in enumerate(zip(plain, queried)):
        assert a.tobytes() == b.tobytes(), "frame %d differs once ranged queries ran in between" % k
    assert plain[0].tobytes() != plain[1].tobytes()
