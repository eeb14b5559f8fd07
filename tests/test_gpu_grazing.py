"""Sub-pixel and grazing primitives against every culling path (-m gpu).

Every speed-up of the render decides WHICH primitives a ray tests, never what a test computes, and is right only while
its bound is conservative at its edge.  The scenes here hold nothing but that edge: primitives smaller than a pixel
(tests/grazing_probes.py), CENTRED on the ray of a tile's corner pixel -- only that ray hits -- or TANGENT to it: the
centre r (1 - EPS) beside the ray, away from the middle of the tile, so that the primitive lies outside the tile's rays
and only the corner ray grazes it.  t = 3, 40 and 4000 along the ray; the far one puts tiny extents at large coordinates
(the bounds' 1e-9 (1 + magnitude) term, the boxes' inflation).  A bound too narrow by more than the inset loses the probe's
pixel, and the oracle's frame has it.

EPS = 2^-29 (the power of two closest to a true tangent at which every tangent probe is live in the oracle; 2^-30 kills the
t = 4000 probes of the 512x448 frames; no t had to be dropped for either kind).  Live counts, checked on the CPU by
tests/test_grazing_probes.py for every list used here (a dead probe fails that test): per frame size poly 7 centred +
7 tangent, s14 7 + 7, s40 20 + 20, s60 30 + 30, s70 35 + 35, s132 66 + 66 (128x96 and 512x448 only), mesh12 6 + 6,
mesh30 15 + 15; oriented s40 20 + 20; child rays 6 + 6 in each of four lists; shadow rays 4 between + 4 beyond + 4 tangent.

Which probe would catch a margin of zero, path by path (the tests assert the kernel each scene takes: expect_kernel):
  tile cone (rm_classify.inc cone_of<false>, keeps)   tangent probes at the four corner pixels of tiles: the corner ray is the
                                                      cone's own edge, the probe's centre lies outside it
  patch cone (cone_of<true>)                          the same at tiles whose corner is a 32x32 patch's corner, the four frame
                                                      corners among them (the widest cones of a frame)
  bundle cone of child rays (rm_trace.inc)            centred and tangent probes on the reflected / refracted ray of a wave's
                                                      corner pixels (test_child_rays), beside the bundle as its neighbours' child
                                                      rays draw it
  group spheres (cull_groups)                         s132 only: the upload builds group spheres from three cull steps on (129
                                                      primitives), so the scenes of up to 70 never reach them.  Its 132 tangent
                                                      and centred probes at all three t lie in three groups of 64 in the
                                                      hierarchy's leaf order; a group sphere too small drops a tangent probe
  edge planes (cull_edges)                            tangent triangle probes (poly: as polygons, mesh12 / mesh30: as a mesh):
                                                      the ray passes r EPS inside a vertex, on the edge planes' side of it; and
                                                      the dart of test_odd_vertex_lists, whose edge planes pointed the wrong way
  plane sign (keeps: `away`)                          NOT attacked at its margin.  The triangle probes lie in planes z = const
                                                      that face the camera (axis . normal 0.8 to 1), where `spread` decides
                                                      nothing: they would catch a wrong sign, not a `spread` of zero, which
                                                      matters only for a plane that holds the tile's corner ray to within EPS.
                                                      The same-x / same-y lists are dropped by their radius of -1 before it.
  box slabs (rm_bvh.hpp inflate, box_hit)             the tangent TRIANGLE probes of mesh12 / mesh30 (triangle hierarchy): the
                                                      grazed vertex is a corner of the triangle's box, at t = 4000 with extents
                                                      of 1e1 at 4e3, and on the centre row / column, where a slab's direction
                                                      component is exactly 0.  The sphere probes of s40 ... s132 (sphere
                                                      hierarchy) reach their boxes with ~0.02 r to spare -- a tangent point is
                                                      not on a face of the sphere's box -- and catch a gross error only
  occluder masks (H) (rm_scene.cpp)                   shadow probes `between` receiver and light, and `tangent` ones there, on the
                                                      shadow rays that run along the hull's edge: from the corners of a small
                                                      quad (they lie ON its bounding sphere) and from a sphere's terminator.
                                                      Neither receiver's bounding sphere holds a light, so their rows clear
                                                      bits, and each probe's bit is set for its own light only
                                                      (tests/test_grazing_probes.py reads the table)
  occluder masks (N)                                  shadow probes `beyond` the light on the same rays (the reference counts
                                                      them as blocking): the edge of the cone behind the light
  sky tail                                            every primary scene through contexts whose every patch is taken for sky
                                                      (RM_SKY_TAIL_FORCE), with and without room to hand them on: a patch that
                                                      holds one probe and nothing else is what a hint gets wrong
  tagged word                                         s40 (a word that still names primitives), s60 (past its 56 bits), three
                                                      frames on one stream -- standing, moved, back -- so that words are carried
  list-only                                           s70, s132
  oriented                                            s40 and the child-ray scene under a yawed, pitched and rolled basis, probes
                                                      built from the oriented oracle helper's rays (test_oriented)
  host bounds (rm_image.cpp put_bounds,               the t = 4000 probes; vertex lists the hull comment was not written for --
  planar_bounds)                                      bow ties, a dart, a non-convex pentagon, clockwise, twin vertices, same x,
                                                      same y -- as polygons and as moved meshes (test_odd_vertex_lists)

Strict flavour: every frame against the oracle, every channel of every pixel within TIGHT.  Fast flavour: a tangent hit is
an exact incidence, which RM_FLAG_FAST_FP may decide differently from the reference, so it is held bit for bit to the fast
frames of a context with everything switched off instead: a cull may only choose what is tested."""
import contextlib
import os

import numpy as np
import pytest

import grazing_probes as GP
import test_gpu_parity as P

pytestmark = pytest.mark.gpu

TIGHT = P.TIGHT
FAST = P.RM_FLAG_FAST_FP

FORCED = {"RM_TILE_CLASSIFY": "1", "RM_PATCH_ORDER": "1", "RM_FIRST_ROUND": "0"}
CONTEXTS = {
    "default": {},
    "forced": FORCED,
    "forced_not_in_launch": dict(FORCED, RM_CLASSIFY_IN_LAUNCH="0"),
    # every place of the order taken for sky, whatever the frames before said: handed on behind the grid / rendered by the tail's wave
    "tail": dict(FORCED, RM_SKY_TAIL="1", RM_SKY_TAIL_FORCE="100000"),
    "tail_no_room": dict(FORCED, RM_SKY_TAIL="1", RM_SKY_TAIL_FORCE="100000", RM_SKY_TAIL_CAP="0"),
    "cull": {"RM_CULL_MIN": "1"},
    "no_masks": {"RM_SHADOW_MASKS": "0"},
    "off": {"RM_TILE_CLASSIFY": "0", "RM_PATCH_ORDER": "0", "RM_DISABLE_CULL": "1", "RM_DISABLE_BVH": "1", "RM_SHADOW_MASKS": "0"},
}
# (what the fast frames of "cull" are held to: the same kernel with every bundle taken for wide -- a kernel without the cull
# compiled in may sum a pixel's terms in another order, tests/test_gpu_parity.py test_bundle_cull_equals_plain_walk_bitwise)
CONTEXTS["off_cull"] = dict(CONTEXTS["off"], RM_CULL_MIN="1")
off_for = lambda context: "off_cull" if context == "cull" else "off"
PRIMARY_CONTEXTS = ["default", "forced", "forced_not_in_launch", "tail", "tail_no_room", "off"]


@contextlib.contextmanager
def contexts(pkg, *names):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    made = []
    try:
        for name in names:
            env = CONTEXTS[name]
            before = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                made.append(pkg.backend.Context(0))
            finally:
                for k, v in before.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
        yield made
    finally:
        for c in made:
            c.close()


@pytest.fixture(scope="module")
def cam(O, tmp_path_factory):
    return GP.oracle_camera(O, tmp_path_factory.mktemp("orc_camera"))


_REFS = {}


def reference(O, key, recipe, view, depth, cam=None, lights=GP.LIGHTS):
    """The oracle's frame, computed once and shared (never written to)."""
    if key not in _REFS:
        _REFS[key] = GP.oracle_frame(O, recipe, view, depth, cam, lights=lights)
        _REFS[key].setflags(write=False)
    return _REFS[key]


def sequence(pkg, ctx, scene, eyes, w, h, depth, flags, basis=None):
    """One upload, then a frame per eye on the context's stream, each into a device buffer pre-filled with a sentinel."""
    import torch
    ctx.upload(scene.flatten())
    ctx.orient(basis)
    p = pkg.backend.make_params(GP.workloads.FOV, float(h), float(w), depth)
    p.flags = flags
    rows = h // 32 * 32
    out, tails = [], 0
    for eye in eyes:
        ctx.set_camera(tuple(eye))
        dev = torch.full((h, w, 3), -1., dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        ctx.render_device(p, dev.data_ptr())
        torch.cuda.synchronize()
        got = dev.cpu().numpy()
        assert not (got[:rows] == -1.).any(), "a pixel of the rendered rows was left out"
        assert (got[rows:] == -1.).all()
        out.append(got[:rows])
        tails += ctx.launch_stats()[1]
    return out, tails, ctx.kernel_name(p)


def against_oracle(frames, refs, label):
    P._FLAGS["value"] = 0
    for k, (got, ref) in enumerate(zip(frames, refs)):
        worst = P.compare(got, ref, TIGHT)
        print("%s frame %d: max |delta| %.3e" % (label, k, worst))


def same_bits(frames, plain, label):
    for k, (a, b) in enumerate(zip(frames, plain)):
        diff = np.argwhere((a != b).any(axis=2))
        assert diff.size == 0, "%s frame %d: %d pixels differ from the frame of the context with everything off, first (y, x) %s" % (
            label, k, len(diff), diff[:6].tolist())


def eyes_of(eye):
    """standing, camera moved, back: the carried order and words come in"""
    moved = tuple(eye[c] + GP.MOVED[c] for c in range(3))
    return [tuple(eye), moved, tuple(eye)]


def frame_sizes(name, context):
    return [f for f in GP.frames_for(name) if f != GP.BIG_FRAME or context == "default"]


# The path a scene takes, so that a threshold moved in rm_plan cannot empty a row of the map above without a failure: the
# render kernel's template arguments (stack, pow, waves, per wave, STAGED, BVH, CULL, EDGES, ORDER, FEEDBACK) as rm_kernel_name reports them.
KERNEL_ARGS = {"bvh": 5, "cull": 6, "edges": 7, "order": 8}
PRIMARY_KERNELS = {"poly": dict(bvh=False, cull=True, edges=True), "s14": dict(bvh=False, cull=True, edges=False),
                   "s40": dict(bvh=True, cull=True), "s60": dict(bvh=True, cull=True), "s70": dict(bvh=True, cull=True),
                   "s132": dict(bvh=True, cull=True), "mesh12": dict(bvh=True, cull=True, edges=True),
                   "mesh30": dict(bvh=True, cull=True, edges=True)}


def expect_kernel(kernel, context, **want):
    args = [x.strip() for x in kernel.split("<", 1)[1].rstrip(">").split(",")]
    if context.startswith("off"):
        want = dict(want, bvh=False)
    if context.startswith(("forced", "tail")):
        want = dict(want, order=True)
    for k, v in want.items():
        assert args[KERNEL_ARGS[k]] == ("true" if v else "false"), "%s: %s is not %s in %s" % (context, k.upper(), v, kernel)


# ---------------------------------------------------------------- 2. primary rays: classification, sky tail, hierarchy
@pytest.mark.parametrize("context", PRIMARY_CONTEXTS)
@pytest.mark.parametrize("name", list(GP.PRIMARY_SCENES))
def test_primary_probes_against_the_oracle(pkg, O, name, context):
    with contexts(pkg, context) as (ctx,):
        tails = 0
        for w, h in frame_sizes(name, context):
            view, recipe, probes = GP.primary_case(O, name, w, h)
            eyes = eyes_of(view.eye)
            refs = [reference(O, (name, w, h, eye), recipe, GP.View(O, w, h, eye), 3) for eye in eyes]
            for x, y, kind, _ in probes:
                assert refs[0][y, x].max() > 0.                                 # (the oracle's frame shows every probe)
            frames, n_tail, kernel = sequence(pkg, ctx, GP.product_scene(pkg, recipe), eyes, w, h, 3, 0)
            print(name, context, w, h, kernel, "patches in the tail:", n_tail, "tiles, tiles listed:", ctx.tile_stats())
            expect_kernel(kernel, context, **PRIMARY_KERNELS[name])
            tails += n_tail
            against_oracle(frames, refs, "%s %s %dx%d" % (name, context, w, h))
        assert tails > 0 or not context.startswith("tail"), "no patch went through the sky tail"


@pytest.mark.parametrize("context", PRIMARY_CONTEXTS[:-1])
@pytest.mark.parametrize("name", list(GP.PRIMARY_SCENES))
def test_primary_probes_fast_flavour_bit_for_bit(pkg, O, name, context):
    with contexts(pkg, context, off_for(context)) as (ctx, plain):
        for w, h in frame_sizes(name, context):
            view, recipe, probes = GP.primary_case(O, name, w, h)
            scene, eyes = GP.product_scene(pkg, recipe), eyes_of(view.eye)
            frames, _, _ = sequence(pkg, ctx, scene, eyes, w, h, 3, FAST)
            want, _, _ = sequence(pkg, plain, scene, eyes, w, h, 3, FAST)
            assert sum(int(want[0][y, x].max() > 0.) for x, y, _, _ in probes) >= len(probes) // 2       # (centred probes show in any flavour)
            same_bits(frames, want, "%s %s %dx%d" % (name, context, w, h))


# ---------------------------------------------------------------- 3. child rays: the bundle cone
@pytest.mark.parametrize("context", ["default", "cull", "forced"])
@pytest.mark.parametrize("padding", [0, GP.CHILD_PADDING])
def test_child_rays(pkg, O, padding, context):
    """A reflecting floor, a sphere whose rim reflects and whose middle refracts, a glass sphere; probes on the child rays
    of wave-corner pixels, centred and tangent.  Depth 4.  RM_CULL_MIN=1 sends the small scene through the cull kernel; the
    padded one (17 spheres and the probes) walks the hierarchy with incoherent rays."""
    w, h = GP.CHILD_FRAME
    view = GP.View(O, w, h)
    recipe, probes = GP.child_recipe(O, view, GP.CHILD_PROBES, 5 + padding, padding)
    scene, eyes = GP.product_scene(pkg, recipe), eyes_of(view.eye)
    refs = [reference(O, ("child", padding, eye), recipe, GP.View(O, w, h, eye), GP.CHILD_DEPTH) for eye in eyes]
    with contexts(pkg, context, off_for(context)) as (ctx, plain):
        frames, _, kernel = sequence(pkg, ctx, scene, eyes, w, h, GP.CHILD_DEPTH, 0)
        print("child +%d" % padding, context, kernel)
        expect_kernel(kernel, context, bvh=padding > 0, cull=True)
        against_oracle(frames, refs, "child +%d %s" % (padding, context))
        against_oracle(sequence(pkg, plain, scene, eyes, w, h, GP.CHILD_DEPTH, 0)[0], refs, "child +%d off" % padding)
        fast, _, _ = sequence(pkg, ctx, scene, eyes, w, h, GP.CHILD_DEPTH, FAST)
        same_bits(fast, sequence(pkg, plain, scene, eyes, w, h, GP.CHILD_DEPTH, FAST)[0], "child +%d %s fast" % (padding, context))


# ---------------------------------------------------------------- 4. shadow rays: the occluder masks
@pytest.mark.parametrize("context", ["default", "no_masks", "cull"])
def test_shadow_rays(pkg, O, context):
    """A small lit quad and a sphere, two lights outside both bounding spheres, 14 primitives (the table exists and its
    rows clear bits); probes on the shadow rays that leave the quad's corners and the sphere's terminator: between the hit
    point and the light, beyond the light, tangent to the ray -- each combination of receiver, light and kind."""
    w, h = GP.SHADOW_FRAME
    view = GP.View(O, w, h)
    recipe, probes = GP.shadow_recipe(O, view, GP.SHADOW_PROBES, 3)
    scene, eyes = GP.product_scene(pkg, recipe, lights=GP.SHADOW_LIGHTS), eyes_of(view.eye)
    refs = [reference(O, ("shadow", eye), recipe, GP.View(O, w, h, eye), GP.SHADOW_DEPTH, lights=GP.SHADOW_LIGHTS) for eye in eyes]
    lit = reference(O, ("shadow, no probes",), recipe[:len(GP.SHADOW_BASE)], view, GP.SHADOW_DEPTH, lights=GP.SHADOW_LIGHTS)
    for x, y, kind, index, light, receiver in probes:
        assert refs[0][y, x].sum() < lit[y, x].sum(), "pixel (%d, %d) is not darker for its %s probe" % (x, y, kind)
    with contexts(pkg, context, off_for(context)) as (ctx, plain):
        frames, _, kernel = sequence(pkg, ctx, scene, eyes, w, h, GP.SHADOW_DEPTH, 0)
        print("shadow", context, kernel)
        expect_kernel(kernel, context, bvh=False, cull=True)
        against_oracle(frames, refs, "shadow %s" % context)
        fast, _, _ = sequence(pkg, ctx, scene, eyes, w, h, GP.SHADOW_DEPTH, FAST)
        same_bits(fast, sequence(pkg, plain, scene, eyes, w, h, GP.SHADOW_DEPTH, FAST)[0], "shadow %s fast" % context)


# ---------------------------------------------------------------- 5. vertex lists the bounds' comment does not cover
@pytest.mark.parametrize("as_mesh", [False, True], ids=["polygon", "moved_mesh"])
@pytest.mark.parametrize("among_spheres", [False, True], ids=["alone", "among_others"])
@pytest.mark.parametrize("name", list(GP.ODD_POLYGONS))
def test_odd_vertex_lists(pkg, O, name, among_spheres, as_mesh):
    """ConvexPolygon::create takes any vertex list, and the host's bounds argue with `the hull of the lifted vertices`:
    self-intersecting, non-convex and clockwise lists, two consecutive vertices at one (x, y), every vertex at one x or one
    y (the lists the upload marks as never hit) -- alone, and among 12 spheres and 3 small triangles, where the cull and its
    edge test apply; as
    polygons, and as fans of triangles in a mesh that an offset moves (the marks are made after the move)."""
    w, h, depth = 160, 128, 3
    view = GP.View(O, w, h)
    recipe = GP.odd_recipe(name, among_spheres, as_mesh)
    scene = GP.product_scene(pkg, recipe)
    eyes = [(0., 0., 0.), (1.5, -0.5, 2.)]
    refs = [reference(O, ("odd", name, among_spheres, as_mesh, eye), recipe, GP.View(O, w, h, eye), depth) for eye in eyes]
    if among_spheres or name in ("convex_ccw", "dart_quad"):
        assert (refs[0].max(axis=2) > 0.).sum() > 50
    with contexts(pkg, "default", "off", "cull", "off_cull") as (ctx, plain, cull, plain_cull):
        for label, c, off in (("default", ctx, plain), ("cull", cull, plain_cull)):
            against_oracle(sequence(pkg, c, scene, eyes, w, h, depth, 0)[0], refs, "%s %s" % (name, label))
            same_bits(sequence(pkg, c, scene, eyes, w, h, depth, FAST)[0], sequence(pkg, off, scene, eyes, w, h, depth, FAST)[0],
                      "%s %s fast" % (name, label))
        against_oracle(sequence(pkg, plain, scene, eyes, w, h, depth, 0)[0], refs, "%s off" % name)


# ---------------------------------------------------------------- 6. oriented camera
@pytest.mark.parametrize("context", ["default", "forced", "tail", "cull"])
@pytest.mark.parametrize("what", ["primary", "child"])
def test_oriented(pkg, O, cam, what, context):
    """The oriented kernels' copies of all of the above: the 40-sphere scene and the padded child-ray scene under a yawed,
    pitched and rolled basis, probes built from the oriented oracle helper's rays."""
    w, h = GP.SMALL_FRAMES[0]
    basis = GP.oriented_basis(pkg)
    rows = GP.basis_rows(basis)
    view = GP.View(O, w, h, GP.ORIENTED_EYE, rows, cam)
    if what == "primary":
        _, recipe, probes = GP.primary_case(O, GP.ORIENTED_SCENE, w, h, GP.ORIENTED_EYE, rows, cam)
        depth = 3
    else:
        recipe, probes = GP.child_recipe(O, view, GP.CHILD_PROBES, 5 + GP.CHILD_PADDING, GP.CHILD_PADDING)
        depth = GP.CHILD_DEPTH
    scene, eyes = GP.product_scene(pkg, recipe), eyes_of(GP.ORIENTED_EYE)
    refs = [reference(O, ("oriented", what, eye), recipe, GP.View(O, w, h, eye, rows, cam), depth, cam) for eye in eyes]
    for p in probes:
        assert refs[0][p[1], p[0]].max() > 0.
    with contexts(pkg, context, off_for(context)) as (ctx, plain):
        frames, _, kernel = sequence(pkg, ctx, scene, eyes, w, h, depth, 0, basis)
        assert "_o::" in kernel, kernel
        print("oriented", what, context, kernel)
        expect_kernel(kernel, context, bvh=True, cull=True)
        against_oracle(frames, refs, "oriented %s %s" % (what, context))
        fast, _, _ = sequence(pkg, ctx, scene, eyes, w, h, depth, FAST, basis)
        same_bits(fast, sequence(pkg, plain, scene, eyes, w, h, depth, FAST, basis)[0], "oriented %s %s fast" % (what, context))
