"""The hierarchy walk held to the oracle where the suite never looked (-m gpu): directions the API admits but that are not
unit, and trees as deep as the builder makes them.  tests/hierarchy_reference.py holds the model and the recipes,
tests/test_hierarchy_walk.py pins on the CPU that they have teeth.

1. Admitted directions (|d.d - 1| < 1e-4) on the demo scene (flat, occluder masks), the Cornell box, the 256 spheres and the
   variant matrix's `spheres` and `mesh` cells, through rm_intersect_rays / rm_occluded_rays, their ranged forms over
   [0, inf] and two finite ranges, the device forms, and rm_radiance_rays at depth 3 and 6: decisions are the oracle's on
   every ray, t / point / normal / radiance within TIGHT.  The reference's sphere rule is no geometric test for such rays (a
   sphere acts as one of r^2 + (d.d - 1) * tca^2), so neither the hierarchy's boxes, nor the pruning distance, nor the
   occluder masks hold for them: a wave that carries such a ray takes the complete walk.  Each test
   prints, per class of d.d - 1, how many rays the model calls unreachable and how many of those the GPU answered as the
   oracle does.  Measured on an MI355X, d.d = 1 + 9e-5: 256 spheres, 76 such rays, 58 answered as the oracle does before
   that rule (18 closest hits and 9 occlusion decisions wrong), 76 with it; the matrix's 25 spheres, 60 of 60 before and
   with it -- the model walks each ray alone, a wave enters a leaf where ANY of its 64 rays meets the box, and there the
   neighbours dragged every such leaf in.  No ray of another class was ever answered wrongly, nor any on the demo scene.

2. Deep trees: the chain scenes (spheres: 27 levels; mesh: 21) through every kernel family that has a hierarchy
   instantiation, each against the flat walk of a context created under RM_DISABLE_BVH=1 byte for byte, and against the
   oracle: decisions exact, values within TIGHT relative to max(1, |value|) (the chain's coordinates reach 1e27).  Before
   every test rm_kernel_name says of the two live contexts that the one holds a hierarchy and the other none (a context
   builds one scene image, and every launcher picks its instantiation by that image's header).  Every device output lies in
   the middle of a larger buffer of a sentinel (Guarded): the GUARD elements before and behind it must stand, and -- but
   for the display bytes, whose every value is a possible answer -- no element of the output keeps the sentinel.  The
   converging frames' buffers (tests/test_gpu_converge.py Frame) have their guard behind them only; the refine workspace is
   the wrapper's own.  The host forms must equal the guarded device forms byte for byte.  The moving families walk flat
   whatever the image holds and stay out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import antialias_reference as AR
import converge_reference as CR
import hierarchy_reference as HR
import progressive_reference as PR
import radiance_reference as RR
import ranged_reference
import test_gpu_converge as GC
import test_gpu_lens as GL
import test_gpu_query as GQ
import test_gpu_render_matrix as GRM
import test_launch_plan as LP
import test_scene_image as SI
import variant_matrix as VM
import workloads

pytestmark = pytest.mark.gpu

TIGHT = RR.TIGHT
NAN = float("nan")
SENTINEL = -7.25
RM_FLAG_FAST_FP = 2
W, H = HR.CHAIN_W, HR.CHAIN_H
SMALL = 32                               # the sampled frames' side
RANGES = ((5., 45.), (20., 1e3))         # the two finite ranges of the admitted directions


@pytest.fixture(scope="module")
def contexts(pkg):
    """(the context as it comes, one created under RM_DISABLE_BVH=1: the flat walk)"""
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    before = os.environ.pop("RM_DISABLE_BVH", None)
    try:
        hier = pkg.backend.Context(0)
        os.environ["RM_DISABLE_BVH"] = "1"
        flat = pkg.backend.Context(0)
    finally:
        os.environ.pop("RM_DISABLE_BVH", None)
        if before is not None:
            os.environ["RM_DISABLE_BVH"] = before
    yield hier, flat
    hier.close()
    flat.close()


@pytest.fixture(scope="module")
def batch(O, entry, tmp_path_factory):
    d = tmp_path_factory.mktemp("orc_batch_hierarchy_gpu")
    src, so = d / "orc_batch.c", d / "orc_batch.so"
    src.write_text(GQ.BATCH_C)
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-shared", "-fPIC",
                           "-I", os.path.join(entry.ROOT, "oracle"), str(src), "-o", str(so)])
    return GQ.OracleBatch(O, C.CDLL(str(so)))


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_hierarchy_gpu"))


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def rel(got, ref):
    """The largest |got - ref| / max(1, |ref|)."""
    return float((np.abs(got - ref) / np.maximum(1., np.abs(ref))).max(initial=0.))


# ================================================================ 1. admitted directions
def wrong_closest(g, ref, hit, shape, point, normal):
    """-> bool per ray: the GPU's record is not the oracle's (decision, shape, element; t, point, normal beyond TIGHT)."""
    bad = g["hit"] != hit
    m = hit == 1
    bad |= m & ((g["shape"] % 256 != shape) | (g["shape"] != ref["shape"]) | (g["element"] != ref["element"]))
    with np.errstate(invalid="ignore"):
        bad |= m & ((np.abs(g["t"] - ref["t"]) >= TIGHT) | (np.abs(g["point"] - point) >= TIGHT).any(axis=1) |
                    (np.abs(g["normal"] - normal) >= TIGHT).any(axis=1))
    bad |= ~m & g.view(np.float64).reshape(-1, 9).any(axis=1)          # a miss is all zeros
    return bad


@pytest.mark.parametrize("name", HR.SCENES)
def test_admitted_directions_match_the_oracle(pkg, O, contexts, batch, orc, name):
    """Measured on an MI355X with the rule of DESIGN.md section 6b in place: every ray of every class answered as the oracle
    does, the model-unreachable ones among them (76 of 76 on the 256 spheres, 60 of 60 on the matrix's; the counts are
    printed); radiance within 5.4e-13 of the oracle on every scene."""
    import torch
    ctx = contexts[0]
    scene, oscene = HR.scene_pair(pkg, O, name)
    GL.upload(ctx, scene)
    desc, img = HR.image_of(pkg, scene)
    o, d, e, kind = HR.admitted_set(name, desc)
    assert kind[-1] == HR.QUERY and tuple(d[-1]) == HR.QUERY_TEST_RAY and not o[-1].any()       # the ray tests/test_gpu_query.py only asks about
    refs = ranged_reference.Scene(desc)
    ref = refs.closest(o, d, (0., np.inf))
    hit, shape, point, normal = batch.closest(oscene, o, d)
    occ_ref = batch.occluded(oscene, o, d).astype(bool)
    assert np.array_equal(ref["hit"], hit)                             # (the restatement that names the elements is the oracle's)
    unreach = HR.unreached(img, o, d, HR.pid_of(img, ref["shape"], ref["element"]))

    g = ctx.intersect(o, d)
    occ = ctx.occluded(o, d)
    bad = wrong_closest(g, ref, hit, shape, point, normal)
    bad_occ = occ != occ_ref
    classes = sorted(set(e.tolist()))
    for c in classes:
        m = e == c
        print("%s, d.d - 1 = %g: %d rays, %d hit; closest hit differs on %d, occlusion on %d; model-unreachable %d, of which the GPU "
              "answered %d as the oracle does" % (name, c, int(m.sum()), int(hit[m].sum()), int(bad[m].sum()), int(bad_occ[m].sum()),
                                                   int((m & unreach).sum()), int((m & unreach & ~bad).sum())))
    assert not bad.any(), "%s: %d closest hits differ from the oracle's (%d of them model-unreachable)" % (name, int(bad.sum()), int((bad & unreach).sum()))
    assert not bad_occ.any(), "%s: %d occlusion decisions differ" % (name, int(bad_occ.sum()))

    # the ranged forms: [0, inf] is the unranged query byte for byte; two finite ranges against the restatement, no ray left out
    assert ctx.intersect(o, d, ranges=(0., np.inf)).tobytes() == g.tobytes()
    assert ctx.occluded(o, d, ranges=(0., np.inf)).tobytes() == occ.tobytes()
    to, td = to_dev(o), to_dev(d)
    for r in RANGES:
        rr, (ro, near_o) = refs.closest(o, d, r), refs.occluded(o, d, r)
        assert not rr["near_end"].any() and not near_o.any()
        gr, go = ctx.intersect(o, d, ranges=r), ctx.occluded(o, d, ranges=r)
        assert np.array_equal(gr["hit"], rr["hit"]) and np.array_equal(go, ro), (name, r, int((gr["hit"] != rr["hit"]).sum()), int((go != ro).sum()))
        m = rr["hit"] == 1
        for f in ("shape", "element"):
            assert np.array_equal(gr[f][m], rr[f][m]), (name, r, f)
        assert max(GL.worst(gr[f][m], rr[f][m]) for f in ("t", "point", "normal")) < TIGHT
        assert not gr[~m].view(np.float64).reshape(-1, 9).any() and 0 < m.sum() < len(o)
        tr = to_dev(np.tile(r, (len(o), 1)))
        assert ctx.intersect_device(to, td, ranges=tr).raw.cpu().numpy().tobytes() == gr.tobytes()
        assert np.array_equal(ctx.occluded_device(to, td, ranges=r).cpu().numpy(), go)
    # the device forms
    assert ctx.intersect_device(to, td).raw.cpu().numpy().tobytes() == g.tobytes()
    assert np.array_equal(ctx.occluded_device(to, td).cpu().numpy(), occ)

    # radiance: depth 3 (STACK = 4) and 6 (STACK = 32)
    for depth in (3, 6):
        got = ctx.radiance(o, d, max_depth=depth, background=RR.BACKGROUND)
        want = orc.cast(oscene, o, d, depth)
        delta = np.abs(got - want).max(axis=1)
        assert not np.isnan(got).any()
        print("%s radiance, depth %d: max |delta| %.3e; beyond TIGHT on %d rays (%d of them model-unreachable)" % (
            name, depth, float(delta.max()), int((delta >= TIGHT).sum()), int(((delta >= TIGHT) & unreach).sum()))
              + "".join("; d.d - 1 = %g: %d" % (c, int((delta >= TIGHT)[e == c].sum())) for c in classes if (delta >= TIGHT)[e == c].any()))
        assert delta.max() < TIGHT
        assert ctx.radiance_device(to, td, max_depth=depth, background=RR.BACKGROUND).cpu().numpy().tobytes() == got.tobytes()
        gone = ~(want != 0.).any(axis=1)
        assert gone.any() and not got[gone].view(np.uint64).any()      # what leaves the scene is exactly +0
    torch.cuda.synchronize()


# ================================================================ 2. deep trees
class Chain:
    """A chain scene, made once: the pair, the image, the numpy restatement, the rays and the claim that the launchers see a
    hierarchy."""

    def __init__(self, pkg, O, which):
        self.which = which
        self.name = "chain-" + which
        self.pair = HR.chain_pair(pkg, O, which)
        self.desc, self.img = HR.image_of(pkg, self.pair[0])
        self.ref = ranged_reference.Scene(self.desc)
        self.tree = HR.Tree(self.img, "spheres" if which == "spheres" else "triangles")
        self.o, self.d = HR.chain_rays()
        header = [self.img["H"][k] for k in SI.HEADER_FIELDS]
        for depth in (3, 6):                                          # the shading launchers' own rule: a hierarchy kernel
            assert LP.shading_variant(pkg, header, bool(self.img["verdicts"][1]), depth)[0] is True
        none = list(header)
        none[SI.HEADER_FIELDS.index("off_bvh_spheres")] = none[SI.HEADER_FIELDS.index("off_bvh_triangles")] = 0
        assert LP.shading_variant(pkg, none, bool(self.img["verdicts"][1]), 3)[0] is False


@pytest.fixture(scope="module")
def chains(pkg, O):
    made = {}

    def get(which):
        if which not in made:
            made[which] = Chain(pkg, O, which)
        return made[which]
    return get


def load(pkg, contexts, chain):
    """Uploads the chain to both contexts and asks each what it would launch: a hierarchy kernel on the one, none on the other."""
    for c in contexts:
        GL.upload(c, chain.pair[0])
        c.set_camera((0., 0., 0.))
    p = frame_params(pkg, 3)
    assert GRM.parse(contexts[0].kernel_name(p))[0][4] == 1 and GRM.parse(contexts[1].kernel_name(p))[0][4] == 0


GUARD = 4096
BYTE = 0xAB


class Guarded:
    """A device tensor `t` of `shape` in the middle of a buffer that holds `fill` everywhere, GUARD elements before and behind."""

    def __init__(self, shape, fill, dtype=None):
        import torch
        self.dtype = torch.float64 if dtype is None else dtype
        self.n, self.shape, self.fill = int(np.prod(shape)), shape, fill
        self.buf = torch.full((self.n + 2 * GUARD,), fill, dtype=self.dtype, device="cuda:0")
        self.t = self.buf[GUARD:GUARD + self.n].view(*shape)
        assert self.t.is_contiguous() and self.t.data_ptr() == self.buf.data_ptr() + GUARD * self.buf.element_size()
        torch.cuda.synchronize()

    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def numpy(self, what, written=True):
        """The output as numpy once the guards were found standing (written: and no element of it keeps the fill)."""
        import torch
        torch.cuda.synchronize()
        raw = self.buf.cpu().numpy()
        fill = np.full(GUARD, self.fill, dtype=raw.dtype).tobytes()
        assert raw[:GUARD].tobytes() == fill, "%s: written before the output" % what
        assert raw[GUARD + self.n:].tobytes() == fill, "%s: written behind the output" % what
        out = raw[GUARD:GUARD + self.n].reshape(self.shape).copy()
        if written:
            kept = np.isnan(out) if self.fill != self.fill else out == self.fill
            assert not kept.any(), "%s: %d elements never written" % (what, int(kept.sum()))
        return out


def device_queries(pkg, c, o, d, ranges=None):
    """The C device entry points of closest hit and occlusion (plain, or ranged with an (N, 2) array) on guarded outputs ->
    (the rm_hit records, occluded as bool)."""
    import torch
    L, n = pkg.lib(), len(o)
    to, td = to_dev(o), to_dev(d)
    hits, occ = Guarded((n, 9), SENTINEL), Guarded((n,), BYTE, torch.uint8)
    vp, stream = C.c_void_p, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if ranges is None:
        pkg._lib.check(L.rm_intersect_rays_device(c.ptr, vp(to.data_ptr()), vp(td.data_ptr()), n, hits.ptr(), stream), c.ptr)
        pkg._lib.check(L.rm_occluded_rays_device(c.ptr, vp(to.data_ptr()), vp(td.data_ptr()), n, occ.ptr(), stream), c.ptr)
    else:
        tr = to_dev(ranges)
        pkg._lib.check(L.rm_intersect_rays_ranged_device(c.ptr, vp(to.data_ptr()), vp(td.data_ptr()), vp(tr.data_ptr()), n, hits.ptr(), stream), c.ptr)
        pkg._lib.check(L.rm_occluded_rays_ranged_device(c.ptr, vp(to.data_ptr()), vp(td.data_ptr()), vp(tr.data_ptr()), n, occ.ptr(), stream), c.ptr)
    got = occ.numpy("occlusion")
    assert ((got == 0) | (got == 1)).all()
    return hits.numpy("closest hits").reshape(-1).view(pkg.backend.HIT_DTYPE), got.astype(bool)


def both(contexts, call):
    """call(context) on the hierarchy context and on the flat one -> the hierarchy's answer, which the flat walk's must equal
    byte for byte (an answer: an array, or a tuple / dict of arrays and plain values)."""
    a, b = call(contexts[0]), call(contexts[1])

    def same(x, y, where):
        if isinstance(x, dict):
            assert sorted(x) == sorted(y)
            for k in x:
                same(x[k], y[k], "%s[%s]" % (where, k))
        elif isinstance(x, (tuple, list)):
            assert len(x) == len(y)
            for k, (p, q) in enumerate(zip(x, y)):
                same(p, q, "%s[%d]" % (where, k))
        elif isinstance(x, np.ndarray):
            assert x.tobytes() == y.tobytes(), "%s: the hierarchy walk's bytes are not the flat walk's" % where
        else:
            assert x == y, where
    same(a, b, "answer")
    return a


WHICH = pytest.mark.parametrize("which", ["spheres", "mesh"])


@WHICH
def test_deep_tree_queries(pkg, contexts, chains, batch, which):
    """Closest hit, occlusion, their ranged and device forms on the chain scenes, 1,100 rays (17 waves and 12 lanes).  Measured
    on an MI355X: decisions exact; t, point and normal equal to the oracle's to the last bit (largest relative delta 0)."""
    ch = chains(which)
    load(pkg, contexts, ch)
    o, d = ch.o, ch.d
    assert len(o) % 64 and HR.whole_groups(ch.tree.stack_height(o, d), ch.tree.depth - 1) >= 1
    g, occ = both(contexts, lambda c: device_queries(pkg, c, o, d))
    assert both(contexts, lambda c: c.intersect(o, d)).tobytes() == g.tobytes()               # the host forms
    assert np.array_equal(both(contexts, lambda c: c.occluded(o, d)), occ)
    hit, shape, point, normal = batch.closest(ch.pair[1], o, d)
    ref = ch.ref.closest(o, d, (0., np.inf))
    m = hit == 1
    assert np.array_equal(g["hit"], hit) and np.array_equal(g["shape"][m], shape[m]) and np.array_equal(g["element"][m], ref["element"][m])
    assert np.array_equal(occ, batch.occluded(ch.pair[1], o, d).astype(bool))
    worst = max(rel(g["t"][m], ref["t"][m]), rel(g["point"][m], point[m]), rel(g["normal"][m], normal[m]))
    print("%s chain queries: %d of %d hit, %d occluded, max relative delta %.3e" % (which, int(m.sum()), len(o), int(occ.sum()), worst))
    assert worst < TIGHT and not g[~m].view(np.float64).reshape(-1, 9).any() and 0.3 * len(o) < m.sum() < len(o)
    # ranged: per-ray ranges that scale with the chain -- between the links, and from the first link's back on
    scale = np.abs(o[:, 2]) + HR.CHAIN_R0
    for r in (np.stack([4. * scale, 400. * scale], axis=1), np.stack([0.5 * scale, np.full(len(o), np.inf)], axis=1)):
        rr, (ro, near_o) = ch.ref.closest(o, d, r), ch.ref.occluded(o, d, r)
        assert not rr["near_end"].any() and not near_o.any()
        gr, go = both(contexts, lambda c: device_queries(pkg, c, o, d, r))
        assert both(contexts, lambda c: c.intersect(o, d, ranges=r)).tobytes() == gr.tobytes()
        assert np.array_equal(both(contexts, lambda c: c.occluded(o, d, ranges=r)), go)
        k = rr["hit"] == 1
        assert np.array_equal(gr["hit"], rr["hit"]) and np.array_equal(go, ro) and 0 < k.sum() < len(o)
        assert np.array_equal(gr["shape"][k], rr["shape"][k]) and np.array_equal(gr["element"][k], rr["element"][k])
        assert max(rel(gr[f][k], rr[f][k]) for f in ("t", "point", "normal")) < TIGHT


def frame_params(pkg, depth, fast=False):
    p = pkg.backend.make_params(HR.CHAIN_FOV, float(H), float(W), depth)
    p.flags = RM_FLAG_FAST_FP if fast else 0
    return p


def guarded_frame(ctx, p):
    """rm_render_device into a guarded frame of SENTINEL."""
    frame = Guarded((H, W, 3), SENTINEL)
    ctx.render_device(p, frame.t.data_ptr())
    return frame.numpy("render")


@pytest.mark.parametrize("camera", ["fixed", "rolled"])
@pytest.mark.parametrize("flavour", ["strict", "fast"])
@WHICH
def test_deep_tree_render(pkg, contexts, chains, orc, which, flavour, camera):
    """rm_render_device, 64 x 64, depth 3 and 6.  Measured on an MI355X: strict within 5.6e-16 of the oracle on the
    sphere chain and 5.7e-15 on the mesh chain; the fast flavour within 9.9e-13, no differing pixel (none is
    allowed: tests/tie_reference.py compare_fast with no ties named)."""
    import render_matrix as RM
    ch = chains(which)
    load(pkg, contexts, ch)
    basis = None if camera == "fixed" else RM.rolled_basis()
    for c in contexts:
        c.orient(basis)
    try:
        for depth in (3, 6):
            p = frame_params(pkg, depth, flavour == "fast")
            (_, _, _, _, bvh, _, _, _, _), oriented = GRM.parse(contexts[0].kernel_name(p))
            assert bvh == 1 and oriented == (camera == "rolled") and GRM.parse(contexts[1].kernel_name(p))[0][4] == 0
            got = both(contexts, lambda c: guarded_frame(c, p))
            dirs = RR.sample_directions(RR.pixel_positions(W, H), p, basis)
            want = orc.cast(ch.pair[1], (0., 0., 0.), dirs, depth, normalize=True).reshape(H, W, 3)
            worst, ties = GRM.compare(got, want, flavour == "fast", "%s chain %s %s depth %d" % (which, flavour, camera, depth))
            print("%s chain render, %s, %s camera, depth %d: max |delta| %.3e, %d tie pixels" % (which, flavour, camera, depth, worst, ties))
            assert (want != 0.).any(axis=2).mean() > 0.5
    finally:
        for c in contexts:
            c.orient(None)


@WHICH
def test_deep_tree_primary_hits_and_pick(pkg, contexts, chains, batch, which):
    """rm_primary_hits_device and rm_pick.  Measured on an MI355X: points and normals equal to the oracle's to the last bit."""
    ch = chains(which)
    load(pkg, contexts, ch)
    p = frame_params(pkg, 3)

    def hits(c):
        out = Guarded((H, W, 9), SENTINEL)
        c.primary_hits_device(p, out=out.t)
        return out.numpy("primary hits")
    raw = both(contexts, hits)
    rec = raw.reshape(-1).view(pkg.backend.HIT_DTYPE).reshape(H, W)
    ref_hit, ref_shape, ref_pn = batch.primary(ch.pair[1], W, H, fov=HR.CHAIN_FOV)
    m = ref_hit == 1
    assert np.array_equal(rec["hit"], ref_hit) and np.array_equal(rec["shape"][m], ref_shape[m]) and m.mean() > 0.5
    worst = max(rel(rec["point"][m], ref_pn[..., :3][m]), rel(rec["normal"][m], ref_pn[..., 3:][m]))
    print("%s chain primary hits: %d of %d pixels hit, max relative delta %.3e" % (which, int(m.sum()), m.size, worst))
    assert worst < TIGHT
    for x, y in ((0, 0), (W - 1, H - 1), (W // 2, H // 2), (W // 2 - 1, H // 2), (17, 40), (45, 9)):
        pk = both(contexts, lambda c: np.frombuffer(bytes(c.pick(p, x, y)), dtype=np.uint8))
        assert pk.tobytes() == rec[y, x].tobytes(), (x, y)


def held(got, ref, what, bound=TIGHT):
    """Every channel within `bound` of the oracle's relative to max(1, |value|), nothing NaN -> the worst."""
    got = got.reshape(ref.shape)
    assert not np.isnan(got).any(), what
    worst = rel(got, ref)
    assert worst < bound, "%s: max relative delta %.3e" % (what, worst)
    return worst


@pytest.mark.parametrize("depth", [3, 6])
@WHICH
def test_deep_tree_radiance(pkg, contexts, chains, orc, which, depth):
    """rm_radiance_rays and rm_radiance_samples.  Measured on an MI355X: within 5.6e-16 of the oracle on the sphere chain, 8.9e-15 on
    the mesh chain.  The rays start where the reference's 1e-3 surface offset is representable (HR.chain_rays): with origins
    up to 2^60 * CHAIN_R0 one ray of 1,100, its hit point at 1e13, differed by 3.4e-4 -- hierarchy and flat walk alike."""
    import torch
    ch = chains(which)
    load(pkg, contexts, ch)
    o, d = HR.chain_rays(top=HR.CHAIN_SHADED_TOP)
    assert HR.whole_groups(ch.tree.stack_height(o, d), ch.tree.depth - 1) >= 1

    def rays(c):
        out = Guarded((len(o), 3), NAN)
        to, td, sh = to_dev(o), to_dev(d), pkg.backend._shading(depth, RR.BACKGROUND)
        pkg._lib.check(pkg.lib().rm_radiance_rays_device(c.ptr, C.c_void_p(to.data_ptr()), C.c_void_p(td.data_ptr()), len(o), C.byref(sh), out.ptr(),
                                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), c.ptr)
        return out.numpy("radiance of rays")

    def samples_at(c):
        out = Guarded((len(xy), 3), NAN)
        txy = to_dev(xy)
        pkg._lib.check(pkg.lib().rm_radiance_samples_device(c.ptr, C.byref(p), C.c_void_p(txy.data_ptr()), len(xy), out.ptr(),
                                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), c.ptr)
        return out.numpy("radiance of samples")

    p = frame_params(pkg, depth)
    xy = np.random.default_rng(20261502).uniform((0., 0.), (W, H), size=(HR.CHAIN_RAYS, 2))
    got = both(contexts, rays)
    d_rays = held(got, orc.cast(ch.pair[1], o, d, depth), "rays")
    samples = both(contexts, samples_at)
    want = orc.cast(ch.pair[1], (0., 0., 0.), RR.sample_directions(xy, p), depth, normalize=True)
    d_samples = held(samples, want, "samples")
    # the host forms
    assert both(contexts, lambda c: c.radiance(o, d, max_depth=depth, background=RR.BACKGROUND)).tobytes() == got.tobytes()
    assert both(contexts, lambda c: c.radiance_samples(p, xy)).tobytes() == samples.tobytes()
    print("%s chain radiance, depth %d: max delta rays %.3e, samples %.3e" % (which, depth, d_rays, d_samples))


def small_frame_goes_deep(pkg, ch):
    """The sampled frames are SMALL x SMALL at the suite's field of view: the wave that holds the axis parks the whole depth."""
    p = pkg.backend.make_params(workloads.FOV, float(SMALL), float(SMALL), 3)
    dirs = ranged_reference.normalized(RR.sample_directions(RR.pixel_positions(SMALL, SMALL), p))[0]
    assert ch.tree.stack_height(np.zeros_like(dirs), dirs).max() >= ch.tree.depth - 1


@pytest.mark.parametrize("depth", [3, 6])
@WHICH
def test_deep_tree_refine_and_lens(pkg, O, contexts, chains, orc, which, depth):
    """rm_refine_device and rm_render_lens_device, 32 x 32.  Measured on an MI355X: within 7.8e-16 of the oracle."""
    import torch
    ch = chains(which)
    load(pkg, contexts, ch)
    small_frame_goes_deep(pkg, ch)
    A, Y = AR.Yardstick(pkg, O, orc), CR.Yardstick(pkg, O, orc)
    VM.register(A, ch.name, ch.pair)
    VM.register(Y, ch.name, ch.pair)

    p = pkg.backend.make_params(workloads.FOV, float(SMALL), float(SMALL), depth)

    def refine(c):                                                     # tests/test_gpu_antialias.py Run, on guarded buffers; every pixel refined
        frame, mask = Guarded((SMALL, SMALL, 3), NAN), Guarded((SMALL, SMALL), BYTE, torch.uint8)
        c.render_device(p, frame.t.data_ptr())
        rendered = frame.numpy("frame as rendered")
        ws = c.refine_device(p, frame.t, VM.REFINE_N, -1., mask=mask.t)
        torch.cuda.synchronize()
        ws = ws.cpu().numpy()
        return dict(rendered=rendered, frame=frame.numpy("frame as refined"), mask=mask.numpy("mask"), count=int(ws[0]), listed=np.sort(ws[1:1 + int(ws[0])]))

    def lens(c):
        frame = Guarded((SMALL, SMALL, 3), NAN)
        c.render_lens_device(p, frame.t, HR.CHAIN_APERTURE, HR.CHAIN_FOCUS, table)
        return frame.numpy("lens frame")

    run = both(contexts, refine)
    m_all, f_all = A.refined(ch.name, SMALL, SMALL, depth, VM.REFINE_N, -1.)
    assert run["count"] == SMALL * SMALL and m_all.all() and (run["mask"] == 1).all() and np.array_equal(run["listed"], np.arange(SMALL * SMALL))
    d_refine = held(run["frame"], f_all, "refine")
    table = contexts[0].lens_table(VM.LENS_SAMPLES)
    got = both(contexts, lens)
    d_lens = held(got, Y.frame(ch.name, SMALL, SMALL, depth, HR.CHAIN_APERTURE, HR.CHAIN_FOCUS, table), "lens")
    print("%s chain, depth %d: max delta refine %.3e, lens %.3e" % (which, depth, d_refine, d_lens))


@pytest.mark.parametrize("depth", [3, 6])
@WHICH
def test_deep_tree_accumulate(pkg, O, contexts, chains, orc, which, depth):
    """rm_accumulate_lens_device, rm_accumulate_soft_device and rm_accumulate_converging_device (stored and offset lights),
    32 x 32, sample counts that leave idle lanes.  Measured on an MI355X: means within 8.9e-16 of the oracle, the converging frames' Q / n
    within 1.8e-14."""
    import torch
    ch = chains(which)
    load(pkg, contexts, ch)
    small_frame_goes_deep(pkg, ch)
    Y = CR.Yardstick(pkg, O, orc)
    VM.register(Y, ch.name, ch.pair)
    ap, fo = HR.CHAIN_APERTURE, HR.CHAIN_FOCUS
    table, offsets = contexts[0].lens_sequence(0, 10), contexts[0].light_sequence(0, 10, HR.CHAIN_RADII)
    p = pkg.backend.make_params(workloads.FOV, float(SMALL), float(SMALL), depth)

    def passes(c, soft):                                               # run_passes / run_soft of the suite, on guarded buffers
        total, mean = Guarded((SMALL, SMALL, 3), NAN), Guarded((SMALL, SMALL, 3), NAN)
        rgb8 = Guarded((SMALL, SMALL, 3), BYTE, torch.uint8)
        for done in (0, 5):
            rows = np.ascontiguousarray(table[done:done + 5])
            if soft:
                c.accumulate_soft_device(p, total.t, ap, fo, rows, np.ascontiguousarray(offsets[done:done + 5]), done, mean=mean.t, rgb8=rgb8.t)
            else:
                c.accumulate_lens_device(p, total.t, ap, fo, rows, done, mean=mean.t, rgb8=rgb8.t)
        return total.numpy("sum"), mean.numpy("mean"), rgb8.numpy("display bytes", written=False)

    total, mean, rgb8 = both(contexts, lambda c: passes(c, False))
    ref_sum, ref_mean = Y.progressive(ch.name, SMALL, SMALL, depth, ap, fo, table, (5, 5))
    d_lens = held(mean, ref_mean, "progressive mean")
    held(total, ref_sum, "progressive sum", 10 * TIGHT)
    assert rgb8.tobytes() == PR.to_bytes(mean).tobytes()
    total, mean, rgb8 = both(contexts, lambda c: passes(c, True))
    assert rgb8.tobytes() == PR.to_bytes(mean).tobytes()
    ref_sum, ref_mean = Y.soft(ch.name, SMALL, SMALL, depth, ap, fo, table, offsets, (5, 5))
    d_soft = held(mean, ref_mean, "soft mean")
    held(total, ref_sum, "soft sum", 10 * TIGHT)
    ns, tol, lo, hi = VM.CONVERGE
    worst = np.zeros(4)
    for radii in (None, HR.CHAIN_RADII):
        s = Y.samples(ch.name, SMALL, SMALL, depth, ap, fo, hi, radii)
        ymax = float(np.abs(CR.y_of(s)).max())
        recs, _ = CR.run(s, SMALL, SMALL, ns, tol, lo, hi)
        frames = [GC.Frame(pkg, SMALL, SMALL, guard=64) for _ in contexts]
        tables = [GC.device_tables(c, hi, radii) for c in contexts]
        for k, (listed, st) in enumerate(recs):
            snaps = []
            for c, f, t in zip(contexts, frames, tables):
                GC.converge_pass(pkg, c, f, depth, ap, fo, ns, tol, lo, hi, t, k == 0)
                snaps.append(f.snapshot())
            got = both((0, 1), lambda i: snaps[i])
            for f in frames:                                           # nothing behind the buffers was written
                for key, t in list(f.raw.items()) + [("workspace", f.ws)]:
                    tail = t[-64:].cpu().numpy()
                    fill = NAN if tail.dtype == np.float64 else GC.WORD if tail.dtype == np.int32 else GC.BYTE
                    assert tail.tobytes() == np.full(64, fill, dtype=tail.dtype).tobytes(), key
            assert got["listed"] == int(listed.sum()), "pass %d" % k
            worst = np.maximum(worst, GC.compare(ch.name, k, got, listed, st, ymax))
        assert got["listed"] == 0
        held(got["mean"], recs[-1][1].mean, "converged mean")
    print("%s chain, depth %d: max delta progressive %.3e, soft %.3e; converging mean %.3e, sum / n %.3e, Y / n %.3e, Q / n %.3e" % (
        which, depth, d_lens, d_soft, worst[0], worst[1], worst[2], worst[3]))
