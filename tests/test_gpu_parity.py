"""GPU parity tests proper (-m gpu): the HIP render path, called through the C ABI,
against the CPU oracle on the same inputs, the committed golden file, and
size-independent properties at BASELINE.json's full sizes.

Tolerance: BASELINE.json's north star asks per-channel |delta| < 1e-4 on every pixel.
The default (strict) flavour performs the reference's operations one rounding each, so
every test holds it to TIGHT = 1e-9 on every channel of every pixel (measured: ~3e-15).
The opt-in fast flavour (RM_FLAG_FAST_FP: FMA contraction, Newton rsqrt, hits ordered by
ray parameter) is held to the same bound EXCEPT at pixels that carry a tie certificate
(tests/tie_reference.py): the reference's own colour changes when the primary ray moves by
a few ulps, and the frame shows one of those colours -- rays lying in the plane of a polygon
edge.  A call site that names no ties (`tie=`) admits no differing pixel; the one that does
is test_resolution_sweep, on the demo scene seen from (0, 5, 0).
"""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import tie_reference as TR
import workloads

pytestmark = pytest.mark.gpu

NORTH_STAR_TOL = 1e-4
TIGHT = 1e-9

RM_FLAG_FAST_FP = 2
_FLAGS = {"value": 0}


@pytest.fixture(autouse=True, params=["strict", "fast"])
def flavour(request):
    """Every test runs against both numeric flavours of the kernel: the default (the
    reference's operations one by one) and RM_FLAG_FAST_FP."""
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


def gpu_render(pkg, ctx, scene, w, h, depth, band=None, out=None, fov=workloads.FOV):
    handle = scene.flatten()
    ctx.upload(handle)
    p = pkg.backend.make_params(fov, float(h), float(w), depth, band)
    p.flags = _FLAGS["value"]
    if out is None:
        out = np.zeros((h, w, 3), dtype=np.float64)
    t = ctx.render(p, out)
    return out, t


def device_render_with_sentinel(pkg, ctx, scene, w, h, depth, band=None, sentinel=-1.):
    """One frame into a caller-owned device buffer that holds `sentinel` everywhere beforehand."""
    import torch
    ctx.upload(scene.flatten())
    p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth, band)
    p.flags = _FLAGS["value"]
    dev = torch.full((h, w, 3), sentinel, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.render_device(p, dev.data_ptr())
    torch.cuda.synchronize()
    return dev.cpu().numpy()


def compare(gpu, ref, tol=TIGHT, tie=None):
    """tie: a tie_reference.Tie where the fast flavour's frame may differ at certified ties; None: nowhere."""
    d = np.abs(gpu - ref)
    if _FLAGS["value"] & RM_FLAG_FAST_FP:
        # opt-in flavour: same bound, but pixels the oracle itself cannot decide may show the tie's other side
        return TR.compare_fast(gpu, ref, tol, tie)[0]
    worst = float(d.max())
    n_loose = int((d > 1e-12).sum())
    assert worst < NORTH_STAR_TOL, "max |delta| %.3e breaks the north-star tolerance" % worst
    assert worst < tol, "max |delta| %.3e (channels above 1e-12: %d)" % (worst, n_loose)
    return worst


# ---------------------------------------------------------------- golden + configs
def test_demo_800x600_against_oracle_and_out_ppm(pkg, O, ctx, golden_ppm):
    """The reference's own committed render: GPU frame -> device normalize + quantize
    (rm_postprocess) -> PPM bytes, compared with engine/out.ppm."""
    gpu, _ = gpu_render(pkg, ctx, pkg.Scene.create_default(), 800, 600, 3)
    ref = O.render(O.OracleScene.create_default(), 800, 600, max_depth=3)
    compare(gpu, ref)
    assert np.all(gpu[576:] == 0.)

    out8 = np.empty(800 * 600 * 3, dtype=np.uint8)
    mx = C.c_double()
    pkg._lib.check(pkg.lib().rm_postprocess(ctx.ptr, None, 800, 600, 1,
                                            out8.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(mx)), ctx.ptr)
    assert abs(mx.value - 2.3621674603868565) < 1e-12
    data = b"P6\n800 600\n255\n" + out8.tobytes()
    n_diff = int((np.frombuffer(data, np.uint8) != np.frombuffer(golden_ppm, np.uint8)).sum())
    # u8 truncation can flip a byte when a channel sits within an ulp of k/255
    assert n_diff <= 2, "%d of 1,440,015 bytes differ from the reference's out.ppm" % n_diff
    if n_diff == 0:
        assert hashlib.sha256(data).hexdigest() == "82d51afaaf4a644547728dde89478e484c245d2e3eb1e40da8b928ebd7584797"


@pytest.mark.parametrize("cfg", ["C1", "C2", "C3"])
def test_config_full_frame(pkg, O, ctx, cfg):
    c = workloads.CONFIGS[cfg]
    gpu, _ = gpu_render(pkg, ctx, workloads.product_scene(pkg, c["scene"]), c["width"], c["height"], c["max_depth"])
    ref = O.render(workloads.oracle_scene(O, c["scene"]), c["width"], c["height"], max_depth=c["max_depth"])
    compare(gpu, ref)
    assert (gpu.sum(axis=2) > 0).mean() > 0.1
    if c["height"] % 32:
        assert np.all(gpu[c["height"] - c["height"] % 32:] == 0.)     # 1080 % 32 = 24 rows untouched


def test_config_c4_8k(pkg, O, ctx):
    c = workloads.CONFIGS["C4"]
    w, h = c["width"], c["height"]
    gpu, _ = gpu_render(pkg, ctx, pkg.Scene.create_default(), w, h, c["max_depth"])
    ref = O.render(O.OracleScene.create_default(), w, h, max_depth=c["max_depth"])
    compare(gpu, ref)


def test_config_c5_synthetic_bands(pkg, O, ctx):
    """4096x4096, 256 spheres, depth 10: the oracle needs minutes for the full frame,
    so eight patch rows spread over the image are checked pixel for pixel; the rest is
    covered by the property tests below.
    FIVE frames on the context's stream, like the frames bench.py times: this launch geometry (262,144 tiles = 16,384 patches,
    depth cap 10, hierarchy kernel) is classified at its own head -- 257 primitives: a word only says whether there is anything
    to hit -- and dispatched by the order that gives (r4; the tile-level feedback it carried until r3 is what
    test_feedback_order_renders_every_tile_once forces on): by place in the first frame, by the patches' longest tiles in the
    second and third (which dispatch by their own order), by their predecessor's order from the fourth on, the sky in the tail.
    Each frame goes into a caller-owned device buffer pre-filled with a sentinel, so a tile that was left out -- or rendered into
    the wrong place -- cannot hide behind the previous frame's pixels; all five must hold the oracle's rows and equal each
    other bit for bit."""
    import torch
    c = workloads.CONFIGS["C5"]
    w, h, depth = c["width"], c["height"], c["max_depth"]
    ctx.upload(workloads.product_scene(pkg, "synthetic256").flatten())
    p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)
    p.flags = _FLAGS["value"]
    targs = [x.strip() for x in ctx.kernel_name(p).split("<", 1)[1].rstrip(">").split(",")]   # ..., ORDER, FEEDBACK, HANDON
    assert targs[8] == "true" and targs[9] == "false", "C5 is expected to run the kernel with the dispatch order"
    so = workloads.oracle_scene(O, "synthetic256")
    ref = np.zeros((h, w, 3), dtype=np.float64)
    rows = [0, 23, 47, 64, 77, 96, 111, 127]
    for r in rows:
        O.render(so, w, h, max_depth=depth, frame=ref, band=(r, r + 1))
    dev = torch.empty((h, w, 3), dtype=torch.float64, device="cuda:0")
    first = None
    for frame_no in range(5):
        dev.fill_(-1.)
        torch.cuda.synchronize()
        ctx.render_device(p, dev.data_ptr())            # (HIP's default stream: the same one every time)
        torch.cuda.synchronize()
        gpu = dev.cpu().numpy()
        assert not (gpu == -1.).any(), "frame %d: pixels never written" % frame_no
        for r in rows:
            compare(gpu[r * 32:(r + 1) * 32], ref[r * 32:(r + 1) * 32])
        if first is None:
            first = gpu
            assert (gpu.sum(axis=2) > 0).mean() > 0.3
        else:
            assert np.array_equal(gpu, first), "frame %d differs from frame 0" % frame_no
    del dev


def test_synthetic_small_full_frame(pkg, O, ctx):
    gpu, _ = gpu_render(pkg, ctx, workloads.product_scene(pkg, "synthetic256"), 512, 384, 10)
    ref = O.render(workloads.oracle_scene(O, "synthetic256"), 512, 384, max_depth=10)
    compare(gpu, ref)


# ---------------------------------------------------------------- depth caps
@pytest.mark.parametrize("depth", [0, 1, 2, 3, 4, 6, 9, 10, 17, 18, 32])
def test_depth_caps(pkg, O, ctx, depth):
    gpu, _ = gpu_render(pkg, ctx, pkg.Scene.create_default(), 320, 256, depth)
    ref = O.render(O.OracleScene.create_default(), 320, 256, max_depth=depth)
    compare(gpu, ref)
    if depth == 0:
        assert np.all(gpu == 0.1)       # renderer.rs:262-264 with n_recursion = 1


def test_deep_recursion_needs_the_stack(pkg, O, ctx):
    """A stack of 13 glass panes in front of a glass sphere: every pane adds a level
    (refraction), so the ray trees really reach the caps being tested.  It does not fill
    the per-lane stack: the panes are nearly square to the view and have ri 1.5, and a
    glass hit has both children only beyond asin(1 / ri) off the normal.  cast_ray's tree
    replayed on the CPU under every pixel of the 256x224 frame (variant_matrix.parked_at_once)
    holds at most 1 live sibling at once at depths 5 and 10 (21,011 of the 57,344 pixels; the
    others none) and at most 2 at depths 16 and 32 (8,790 pixels).  The stacks are filled to
    the brim, in every instantiation of the render kernels, by tests/test_gpu_render_matrix.py."""
    glass = dict(diffusion=0.3, diffuse_color=(0.9, 0.8, 0.7), specular=0.9, specular_exponent=20.,
                 is_glass_like=True, reflection=0.4, refractive_index=1.5)
    panes = []
    for k in range(13):
        z = -4. - 1.25 * k
        tilt = 0.05 * k
        panes.append([(-12., -9., z - tilt), (12., -9., z + tilt), (12., 9., z + tilt), (-12., 9., z - tilt)])

    def prod():
        s = pkg.Scene.new()
        R = pkg.Reflectance(**glass)
        V = pkg.Vec3f
        for q in panes:
            s.shapes.append(pkg.polygon.ConvexPolygon.create([V(*p) for p in q], R))
        s.shapes.append(pkg.sphere.create(V(1.5, 0.5, -30.), 6., R))
        s.lights.append(pkg.create_light(V(0., 10., 0.), V(1., 1., 1.), 1.))
        return s

    def orc():
        s = O.OracleScene()
        R = O.reflectance(**glass)
        for q in panes:
            s.add_polygon(q, R)
        s.add_sphere((1.5, 0.5, -30.), 6., R)
        s.add_light((0., 10., 0.), (1., 1., 1.), 1.)
        return s

    refs = {}
    for depth in (5, 10, 16, 32):
        gpu, _ = gpu_render(pkg, ctx, prod(), 256, 224, depth)
        refs[depth] = O.render(orc(), 256, 224, max_depth=depth)
        compare(gpu, refs[depth])
    assert not np.array_equal(refs[10], refs[16])       # levels above 10 are really reached
    assert not np.array_equal(refs[5], refs[10])


@pytest.mark.parametrize("exponents", [(30., 100., 1.), (0., 2., 1000.), (12.5, 30., 7.), (0.5, 1.5, 99.9)])
def test_specular_exponent_flavours(pkg, O, ctx, exponents):
    """renderer.rs:186-188 `powf`: integer-valued exponents take the kernel's binary
    powering flavour, anything else the device pow -- both against the oracle's libm pow."""
    def build(add_sphere, add_light):
        for k, e in enumerate(exponents):
            add_sphere((-6. + 6. * k, 0.5 * k, -14.), 2.6,
                       dict(diffusion=0.8, diffuse_color=(0.2 + 0.3 * k, 0.5, 0.9 - 0.3 * k), specular=0.9,
                            specular_exponent=e, is_glass_like=(k == 1), reflection=0.3, refractive_index=1.4))
        add_light((0., 0., 0.), (1., 1., 1.), 1.)
        add_light((10., 15., 5.), (1., 0.8, 0.6), 0.7)

    s, so = pkg.Scene.new(), O.OracleScene()
    build(lambda c, r, m: s.shapes.append(pkg.sphere.create(pkg.Vec3f(*c), r, pkg.Reflectance(**m))),
          lambda p, c, i: s.lights.append(pkg.create_light(pkg.Vec3f(*p), pkg.Vec3f(*c), i)))
    build(lambda c, r, m: so.add_sphere(c, r, O.reflectance(**m)), lambda p, c, i: so.add_light(p, c, i))
    gpu, _ = gpu_render(pkg, ctx, s, 320, 160, 4)
    compare(gpu, O.render(so, 320, 160, max_depth=4))


# ---------------------------------------------------------------- edge cases
def test_bottom_rows_keep_previous_contents(pkg, O, ctx):
    """renderer.rs:53: H % 32 bottom rows are never written -- stale pixels survive."""
    out = np.full((100, 64, 3), 7.25)
    gpu, _ = gpu_render(pkg, ctx, pkg.Scene.create_default(), 64, 100, 3, out=out)
    assert np.all(gpu[96:] == 7.25)
    ref = O.render(O.OracleScene.create_default(), 64, 100, max_depth=3, frame=np.full((100, 64, 3), 7.25))
    compare(gpu, ref)


def test_width_not_multiple_of_32_is_the_reference_panic(pkg, ctx):
    ctx.upload(pkg.Scene.create_default().flatten())
    p = pkg.backend.make_params(1.5, 64., 100.)
    with pytest.raises(pkg.BackendError) as e:
        ctx.render(p, np.zeros((64, 100, 3)))
    assert e.value.status == pkg._lib.RM_ERR_DIMENSIONS


def test_render_before_upload_and_bad_params(pkg):
    c = pkg.backend.Context(0)
    try:
        p = pkg.backend.make_params(1.5, 64., 64.)
        with pytest.raises(pkg.BackendError) as e:
            c.render(p, np.zeros((64, 64, 3)))
        assert e.value.status == pkg._lib.RM_ERR_NO_SCENE
        c.upload(pkg.Scene.create_default().flatten())
        p.max_depth = 33
        with pytest.raises(pkg.BackendError) as e:
            c.render(p, np.zeros((64, 64, 3)))
        assert e.value.status == pkg._lib.RM_ERR_DEPTH
        p.max_depth = 3
        p.patch_size = 16
        with pytest.raises(pkg.BackendError):
            c.render(p, np.zeros((64, 64, 3)))
    finally:
        c.close()


def test_height_below_one_patch_renders_nothing(pkg, ctx):
    out = np.full((20, 64, 3), -1.)
    gpu, _ = gpu_render(pkg, ctx, pkg.Scene.create_default(), 64, 20, 3, out=out)
    assert np.all(gpu == -1.)


def test_empty_scene_and_no_lights(pkg, O, ctx):
    gpu, _ = gpu_render(pkg, ctx, pkg.Scene.new(), 64, 64, 3)
    assert np.all(gpu == 0.)                                     # primary miss: zero, renderer.rs:305
    s = pkg.Scene.create_default()
    s.lights = []
    so = O.OracleScene.create_default()
    so.c.n_lights = 0
    gpu, _ = gpu_render(pkg, ctx, s, 128, 96, 3)
    ref = O.render(so, 128, 96, max_depth=3)
    compare(gpu, ref)


def test_camera_offsets(pkg, O, ctx):
    """scene.rs:25-27 / main.rs:75-78: +-5 steps; second render goes through
    rm_camera_update without re-upload."""
    s = pkg.Scene.create_default()
    so = O.OracleScene.create_default()
    cam = np.zeros(3)
    for off in [(0., 0., 5.), (-5., 0., 0.), (0., 5., 0.), (0., 0., -15.)]:
        s.offset_camera(pkg.Vec3f(*off))
        cam += off
        so.set_camera(tuple(cam))
        gpu, _ = gpu_render(pkg, ctx, s, 256, 160, 3)
        compare(gpu, O.render(so, 256, 160, max_depth=3))
    ctx.set_camera((1., 2., 3.))
    so.set_camera((1., 2., 3.))
    out = np.zeros((160, 256, 3))
    ctx.render(pkg.backend.make_params(1.5, 160., 256.), out)
    compare(out, O.render(so, 256, 160, max_depth=3))


def test_renderer_dimensions_differ_from_frame(pkg, O, ctx):
    """backproject uses the Renderer's own width/height (renderer.rs:130-131), not the
    FrameBuffer's: render a 128x96 frame with a renderer created for 256x192."""
    ctx.upload(pkg.Scene.create_default().flatten())
    p = pkg.backend.make_params(1.2, 192., 256.)
    p.frame_width, p.frame_height = 128, 96
    out = np.zeros((96, 128, 3))
    ctx.render(p, out)
    L = O.lib()
    r = L.orc_create_renderer(1.2, 192., 256.)
    ref = np.zeros((96, 128, 3))
    so = O.OracleScene.create_default()
    rc = L.orc_render(C.byref(r), so.ptr, ref.ctypes.data_as(C.POINTER(C.c_double)), 128, 96, 3, 0, None)
    assert rc == 0
    compare(out, ref)


def test_exact_ties_follow_list_order(pkg, O, ctx):
    """shapes.rs:130: strict `<` -- the first shape in the list wins an exact distance
    tie.  Coincident spheres of different colours, interleaved with a mesh so that the
    device's grouping by kind differs from list order."""
    tri = np.array([[-30., -30., -40., 30., -30., -40., 0., 30., -40.]])

    def prod(order):
        s = pkg.Scene.new()
        V = pkg.Vec3f
        items = {
            "red": lambda: pkg.sphere.create(V(0., 0., -10.), 3., pkg.Reflectance(diffuse_color=(1., 0., 0.))),
            "green": lambda: pkg.sphere.create(V(0., 0., -10.), 3., pkg.Reflectance(diffuse_color=(0., 1., 0.))),
            "mesh": lambda: pkg.obj.Obj(tri),
            "mesh2": lambda: pkg.obj.Obj(tri),
        }
        for k in order:
            s.shapes.append(items[k]())
        s.lights.append(pkg.create_light(V(0., 0., 0.), V(1., 1., 1.), 1.))
        return s

    def orc(order):
        s = O.OracleScene()
        for k in order:
            if k == "red":
                s.add_sphere((0., 0., -10.), 3., O.reflectance(diffuse_color=(1., 0., 0.)))
            elif k == "green":
                s.add_sphere((0., 0., -10.), 3., O.reflectance(diffuse_color=(0., 1., 0.)))
            else:
                s.add_obj(tri)
        s.add_light((0., 0., 0.), (1., 1., 1.), 1.)
        return s

    centre = {}
    for order in (["red", "mesh", "green", "mesh2"], ["green", "mesh", "red", "mesh2"], ["mesh", "mesh2", "green", "red"]):
        gpu, _ = gpu_render(pkg, ctx, prod(order), 128, 128, 3)
        compare(gpu, O.render(orc(order), 128, 128, max_depth=3))
        centre[tuple(order)] = gpu[64, 64]
    assert centre[("red", "mesh", "green", "mesh2")][0] > centre[("red", "mesh", "green", "mesh2")][1]
    assert centre[("green", "mesh", "red", "mesh2")][1] > centre[("green", "mesh", "red", "mesh2")][0]


def test_polygon_winding_and_edge_on(pkg, O, ctx):
    """polygon.rs:54-56: 2-D inside test in the XY projection, counter-clockwise only;
    clockwise and edge-on (to z) polygons never hit."""
    ccw = [(-4., -3., -12.), (4., -3., -10.), (5., 3., -9.), (0., 5., -11.), (-5., 2., -13.)]
    cw = list(reversed(ccw))
    edge_on = [(0., -3., -5.), (0., 3., -5.), (0., 3., -15.), (0., -3., -15.)]
    for verts in (ccw, cw, edge_on):
        s = pkg.Scene.new()
        s.shapes.append(pkg.polygon.ConvexPolygon.create([pkg.Vec3f(*p) for p in verts],
                                                         pkg.Reflectance(diffuse_color=(0.5, 0.6, 0.7))))
        s.lights.append(pkg.create_light(pkg.Vec3f(2., 3., 0.), pkg.Vec3f(1., 1., 1.), 1.))
        so = O.OracleScene()
        so.add_polygon(verts, O.reflectance(diffuse_color=(0.5, 0.6, 0.7)))
        so.add_light((2., 3., 0.), (1., 1., 1.), 1.)
        gpu, _ = gpu_render(pkg, ctx, s, 160, 128, 3)
        ref = O.render(so, 160, 128, max_depth=3)
        compare(gpu, ref)
        assert (gpu.sum() > 0) == (verts is ccw)


def test_shadow_from_occluder_behind_the_light(pkg, O, ctx):
    """renderer.rs:174: the any-hit test is not limited to the light's distance."""
    def mk(with_blocker):
        s, so = pkg.Scene.new(), O.OracleScene()
        V = pkg.Vec3f
        s.shapes.append(pkg.sphere.create(V(0., 0., -10.), 2., pkg.Reflectance.create_default()))
        so.add_sphere((0., 0., -10.), 2., O.reflectance())
        if with_blocker:      # beyond the light, as seen from the lit sphere
            s.shapes.append(pkg.sphere.create(V(0., 30., -10.), 4., pkg.Reflectance.create_default()))
            so.add_sphere((0., 30., -10.), 4., O.reflectance())
        s.lights.append(pkg.create_light(V(0., 10., -10.), V(1., 1., 1.), 1.))
        so.add_light((0., 10., -10.), (1., 1., 1.), 1.)
        return s, so
    s, so = mk(True)
    gpu, _ = gpu_render(pkg, ctx, s, 128, 128, 3)
    compare(gpu, O.render(so, 128, 128, max_depth=3))
    s2, _ = mk(False)
    lit, _ = gpu_render(pkg, ctx, s2, 128, 128, 3)
    assert lit[50, 64].sum() > gpu[50, 64].sum()      # the far sphere shadows the near one


def test_large_scene_is_read_from_global_memory(pkg, O, ctx):
    """Scenes beyond the LDS copy limit (4 KB) take the unstaged kernel: 700 random
    triangles (~125 KB of scene words) + spheres, against the oracle."""
    rng = np.random.default_rng(11)
    base = rng.uniform(-12., 12., size=(700, 1, 3)) + np.array([0., 0., -40.])
    tri = (base + rng.uniform(-1.5, 1.5, size=(700, 3, 3))).reshape(700, 9)
    s, so = pkg.Scene.new(), O.OracleScene()
    s.shapes.append(pkg.obj.Obj(tri)); so.add_obj(tri)
    glass = dict(diffusion=0.4, diffuse_color=(0.8, 0.9, 0.7), specular=0.8, specular_exponent=40.,
                 is_glass_like=True, reflection=0.35, refractive_index=1.4)
    s.shapes.append(pkg.sphere.create(pkg.Vec3f(0., 0., -15.), 4., pkg.Reflectance(**glass)))
    so.add_sphere((0., 0., -15.), 4., O.reflectance(**glass))
    for pos, col, inten in workloads.DEMO_LIGHTS:
        s.lights.append(pkg.create_light(pkg.Vec3f(*pos), pkg.Vec3f(*col), inten)); so.add_light(pos, col, inten)
    gpu, _ = gpu_render(pkg, ctx, s, 192, 128, 6)
    compare(gpu, O.render(so, 192, 128, max_depth=6))
    assert (gpu.sum(axis=2) > 0).mean() > 0.03               # half the random triangles wind clockwise
    ctx.upload(pkg.Scene.create_default().flatten())         # context stays usable


@pytest.mark.parametrize("scene_name", ["demo", "cornell"])
def test_resolution_sweep(pkg, O, ctx, scene_name):
    """Small frames of many shapes (odd and even patch counts, tall and wide): the centre
    row / column, where ray components are exactly 0, moves through the scene.
    The fast flavour's ties: seen from (0, 5, 0) the demo scene has a line of rays in the plane of a triangle edge
    (the pixels are tests/test_tie_reference.py's table) -- there, and nowhere else in the sweep, its
    frames may show the other side of a certified tie."""
    scene, so = workloads.product_scene(pkg, scene_name), workloads.oracle_scene(O, scene_name)
    for w, h in [(32, 32), (64, 32), (32, 96), (96, 64), (160, 128), (224, 96), (128, 288), (352, 224)]:
        for cam in [(0., 0., 0.), (0., 5., 0.), (-5., 0., 5.)]:               # main.rs:75-78 steps
            scene.camera = pkg.Vec3f(*cam)
            so.set_camera(cam)
            gpu, _ = gpu_render(pkg, ctx, scene, w, h, 3)
            tie = TR.Tie(so, w, h, 3, eye=cam) if scene_name == "demo" and cam == (0., 5., 0.) else None
            compare(gpu, O.render(so, w, h, max_depth=3), tie=tie)


@pytest.mark.parametrize("seed", range(int(os.environ.get("RM_FUZZ_SEEDS", "12"))))   # RM_FUZZ_SEEDS=300: a longer hunt
def test_fuzz_random_scenes(pkg, O, ctx, seed):
    """Seeded random scenes: spheres (some glass, some coincident), counter-clockwise convex
    polygons, a random-triangle mesh, 1-3 lights, integer and fractional camera positions,
    random frame shapes and depth caps; enough spheres in half of the cases to switch the
    hierarchy walk on.  The product and the oracle are built from the same recipe through
    their own APIs."""
    _fuzz_case(pkg, O, ctx, seed)


@pytest.fixture(scope="module")
def ctx_order_forced(pkg):
    """A context whose every launch classifies its tiles at its head and dispatches ALL of them by the order it lays out
    (no first round): the fuzz's frames are a few hundred tiles, which by their own rules get neither."""
    forced = {"RM_TILE_CLASSIFY": "1", "RM_PATCH_ORDER": "1", "RM_FIRST_ROUND": "0"}
    before = {k: os.environ.get(k) for k in forced}
    os.environ.update(forced)
    try:
        c = pkg.backend.Context(0)
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield c
    c.close()


@pytest.mark.parametrize("seed", range(int(os.environ.get("RM_FUZZ_SEEDS", "12"))))
def test_fuzz_random_scenes_with_the_order_forced(pkg, O, ctx_order_forced, seed):
    """The same scenes with the classification and the dispatch order forced on for every launch -- one context through all
    of them: another scene, another frame shape, another kernel every time.  (r4: seed 2 -- 64 primitives with a hierarchy --
    showed the words of a launch that classifies at its head, 56 bits under the tag, taken as exact for 57-64 primitives.)"""
    _fuzz_case(pkg, O, ctx_order_forced, seed)


def _fuzz_case(pkg, O, ctx, seed):
    s, so, cam, w, h, depth = _fuzz_scene(pkg, O, seed)
    gpu, _ = gpu_render(pkg, ctx, s, w, h, depth)
    compare(gpu, O.render(so, w, h, max_depth=depth))


def fuzz_recipe(seed):
    """Fuzz case `seed` as plain data, no API of anybody's touched: dict(shapes=[("sphere", centre, radius, material) |
    ("polygon", vertices, material) | ("mesh", (nt, 9) float64 triangles, offset)] in scene order, lights=[(position, colour,
    intensity)], camera, width, height, depth).  _fuzz_scene below builds the product's and the oracle's scenes from it, and
    tests/test_second_reading.py the second reading's; the draws and their order are the fuzz's of old (that file pins the
    oracle's frames of seeds 0-11 to the hashes they had before the recipe was lifted out)."""
    rng = np.random.default_rng(1000 + seed)
    shapes, lights = [], []

    def material():
        glass = bool(rng.random() < 0.35)
        return dict(diffusion=float(rng.uniform(0.1, 1.)), diffuse_color=tuple(float(x) for x in rng.uniform(0, 1, 3)),
                    specular=float(rng.uniform(0.2, 1.)), specular_exponent=float(rng.choice([1., 8., 30., 100., 12.5][:4 + (seed % 3 == 0)])),
                    is_glass_like=glass, reflection=float(rng.uniform(0.1, 0.9)),
                    refractive_index=float(rng.uniform(1.1, 1.8)) if glass else 1.)

    n_spheres = int(rng.integers(2, 8)) if seed % 2 else int(rng.integers(20, 60))
    for k in range(n_spheres):
        c = (float(rng.uniform(-12, 12)), float(rng.uniform(-8, 8)), float(rng.uniform(-40, -6)))
        if rng.random() < 0.3:
            c = tuple(float(round(v)) for v in c)                     # integer coordinates: exact incidences
        r, m = float(rng.uniform(0.5, 3.0)), material()
        shapes.append(("sphere", c, r, m))
    for k in range(int(rng.integers(0, 4))):
        nv = int(rng.integers(3, 7))
        ang = np.sort(rng.uniform(0, 2 * np.pi, nv))                  # counter-clockwise in XY
        cx, cy, cz = rng.uniform(-8, 8), rng.uniform(-6, 6), rng.uniform(-35, -8)
        rad = rng.uniform(2, 7)
        tilt = rng.uniform(-0.6, 0.6, 2)
        verts = [(float(cx + rad * np.cos(a)), float(cy + rad * np.sin(a)),
                  float(cz + tilt[0] * rad * np.cos(a) + tilt[1] * rad * np.sin(a))) for a in ang]
        m = material()
        shapes.append(("polygon", verts, m))
    if rng.random() < 0.7:
        nt = int(rng.integers(3, 40))
        base = rng.uniform(-10, 10, size=(nt, 1, 3)) + np.array([0., 0., -25.])
        tri = (base + rng.uniform(-3, 3, size=(nt, 3, 3))).reshape(nt, 9)
        off = (0., float(rng.integers(-2, 3)), float(rng.integers(-10, 1)))
        shapes.append(("mesh", tri, off))
    for k in range(int(rng.integers(1, 4))):
        pos = tuple(float(v) for v in rng.uniform(-20, 20, 3))
        col = tuple(float(v) for v in rng.uniform(0.2, 1, 3))
        inten = float(rng.uniform(0.3, 1.))
        lights.append((pos, col, inten))
    cam = tuple(float(v) for v in (rng.integers(-5, 6, 3) if seed % 3 else rng.uniform(-3, 3, 3)))
    w, h = int(rng.integers(1, 9)) * 32, int(rng.integers(1, 7)) * 32 + int(rng.integers(0, 2)) * 7
    depth = int(rng.integers(1, 7))
    return dict(shapes=shapes, lights=lights, camera=cam, width=w, height=h, depth=depth)


def _fuzz_scene(pkg, O, seed):
    """-> the product's scene, the oracle's, the camera, frame width and height, depth cap of fuzz case `seed`."""
    recipe = fuzz_recipe(seed)
    s, so = pkg.Scene.new(), O.OracleScene()
    for shape in recipe["shapes"]:
        if shape[0] == "sphere":
            _, c, r, m = shape
            s.shapes.append(pkg.sphere.create(pkg.Vec3f(*c), r, pkg.Reflectance(**m)))
            so.add_sphere(c, r, O.reflectance(**m))
        elif shape[0] == "polygon":
            _, verts, m = shape
            s.shapes.append(pkg.polygon.ConvexPolygon.create([pkg.Vec3f(*v) for v in verts], pkg.Reflectance(**m)))
            so.add_polygon(verts, O.reflectance(**m))
        else:
            _, tri, off = shape
            mesh = pkg.obj.Obj(tri)
            mesh.offset(pkg.Vec3f(*off))
            s.shapes.append(mesh)
            so.add_obj(tri, off)
    for pos, col, inten in recipe["lights"]:
        s.lights.append(pkg.create_light(pkg.Vec3f(*pos), pkg.Vec3f(*col), inten))
        so.add_light(pos, col, inten)
    cam = recipe["camera"]
    s.camera = pkg.Vec3f(*cam)
    so.set_camera(cam)
    return s, so, cam, recipe["width"], recipe["height"], recipe["depth"]


@pytest.mark.parametrize("seed", range(int(os.environ.get("RM_FUZZ_SEQ_SEEDS", "8"))))
def test_fuzz_sequences_with_the_order_forced(pkg, O, seed):
    """Random scenes as a host's render loop sees them: seventeen frames of one scene on one stream -- the view standing for ten
    (from the fourth on a launch dispatches by its predecessor's order and takes its predecessor's words, from the fifth on
    three launches in four do not classify at all), one press of the camera, back again for six -- in a frame four times the fuzz's width and height (up to 192 patches), through contexts with the
    classification and the order forced on and the first round cut to 0 / 64 / 256 waves, keys by place / time / content in turn.
    Every frame must equal, bit for bit and in a buffer pre-filled with a sentinel, the frame of a context with neither; the
    first of them is held against the oracle."""
    import torch
    s, so, cam, w, h, depth = _fuzz_scene(pkg, O, seed)
    w, h, depth = 4 * w, 4 * (h - h % 32) + h % 32, min(depth, 3)
    forced = {"RM_TILE_CLASSIFY": "1", "RM_PATCH_ORDER": "1", "RM_FIRST_ROUND": ("0", "64", "256")[seed % 3], "RM_ORDER_KEYS": ("0", "1", "2", "")[seed % 4],
              "RM_ORDER_FREEZE": ("1", "2", "3", "7", "0")[seed % 5]}
    if not forced["RM_ORDER_KEYS"]:
        del forced["RM_ORDER_KEYS"]
    before = {k: os.environ.get(k) for k in list(forced) + ["RM_TILE_CLASSIFY", "RM_PATCH_ORDER"]}
    try:
        os.environ.update({"RM_TILE_CLASSIFY": "0", "RM_PATCH_ORDER": "0"})
        plain = pkg.backend.Context(0)
        os.environ.update(forced)
        ordered = pkg.backend.Context(0)
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        handle = s.flatten()
        plain.upload(handle)
        ordered.upload(handle)
        # (every fifth scene: a rank's share of the frame -- every second or third patch row from some row on, as at N > 1)
        n_rows = h // 32
        band = (seed % 2, n_rows, 2 + seed % 2) if seed % 5 == 4 and n_rows >= 4 else None
        p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth, band)
        p.flags = _FLAGS["value"]
        # (ten frames of one view: from the fifth on, three launches in four take order and classification from their predecessor)
        cams = [cam] * 10 + [(cam[0] + 5., cam[1], cam[2])] + [cam] * 6
        for k, c in enumerate(cams):
            outs = []
            for ctx in (plain, ordered):
                ctx.set_camera(pkg.Vec3f(*c))
                dev = torch.full((h, w, 3), -7., dtype=torch.float64, device="cuda:0")
                dev8 = torch.full((h, w, 3), 77, dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                ctx.render_device_u8(p, dev.data_ptr(), dev8.data_ptr())
                torch.cuda.synchronize()
                outs.append((dev.cpu().numpy(), dev8.cpu().numpy()))
            assert np.array_equal(outs[0][0], outs[1][0]), "frame %d of seed %d (%dx%d, %s): f64 frames differ in %d values" % (
                k, seed, w, h, forced, int((outs[0][0] != outs[1][0]).sum()))
            assert np.array_equal(outs[0][1], outs[1][1]), "frame %d of seed %d: display frames differ" % (k, seed)
            if k == 0 and band is None:
                rows = h - h % 32
                compare(outs[1][0][:rows], O.render(so, w, h, max_depth=depth)[:rows])
    finally:
        plain.close()
        ordered.close()


def _icosphere_obj(path, subdivisions):
    t = (1 + 5 ** 0.5) / 2
    v = [np.array(p, float) / np.linalg.norm(p) for p in
         [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
          (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        cache, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    with open(path, "w") as o:
        o.write("o ico\n")
        for p in v:
            o.write("v %.6f %.6f %.6f\n" % tuple(p * 120 + np.array([0., 0., 250.])))
        for a, b, c in f:
            o.write("f %d %d %d\n" % (a + 1, b + 1, c + 1))
    return len(f)


@pytest.mark.parametrize("subdivisions", [2, 4])
def test_symmetric_mesh_keeps_the_reference_cracks(pkg, O, ctx, tmp_path, subdivisions):
    """A mesh symmetric about x = 0 through the whole OBJ path (main.rs:261-327).  On the
    centre column the ray's x component is exactly 0 and the edge functions of edges in the
    plane x = 0 are exactly 0: the reference's `> 0.` (triangle.rs:13-15) makes both
    neighbouring triangles miss -- a one-pixel crack that the kernel must reproduce in BOTH
    flavours (an early fast flavour closed it: profiles/r01_notes_fast_flavour.txt)."""
    from oracle import obj_oracle
    path = str(tmp_path / "ico.obj")
    n = _icosphere_obj(path, subdivisions)
    assert n == 20 * 4 ** subdivisions
    scene = pkg.Scene.open_obj(path)
    so = O.OracleScene()
    for _, tris in obj_oracle.load_models(path):
        so.add_obj(np.array(tris), (0., 0., -500.))
    for pos, col, inten in workloads.DEMO_LIGHTS:
        so.add_light(pos, col, inten)
    w, h = 320, 256
    gpu, _ = gpu_render(pkg, ctx, scene, w, h, 3)
    ref = O.render(so, w, h, max_depth=3)
    compare(gpu, ref)
    lit = ref.sum(axis=2) > 0
    assert lit[:, w // 2 - 1].sum() > 50 and lit[:, w // 2 + 1].sum() > 50
    assert lit[:, w // 2].sum() < lit[:, w // 2 - 1].sum()          # the crack exists in the reference image


def test_hierarchy_walk_equals_flat_walk_bitwise(pkg, ctx, monkeypatch):
    """the bounding-volume hierarchy only decides WHICH primitives a wave
    tests; the image must be bit-identical to the brute-force walk (RM_DISABLE_BVH=1),
    including the list-order tie-break after the primitives were re-ordered into leaves."""
    scenes = [workloads.product_scene(pkg, "synthetic256"), workloads.product_scene(pkg, "cornell")]
    # duplicates: exact distance ties between re-ordered primitives
    dup = pkg.Scene.new()
    rng = np.random.default_rng(5)
    for k in range(40):
        c = (float(rng.uniform(-8, 8)), float(rng.uniform(-5, 5)), float(rng.uniform(-30, -12)))
        col = tuple(float(x) for x in rng.uniform(0, 1, 3))
        for rep in range(2):            # the same sphere twice, different colours: first in list must win
            dup.shapes.append(pkg.sphere.create(pkg.Vec3f(*c), 1.5, pkg.Reflectance(diffuse_color=col if rep == 0 else (1., 1., 1.),
                                                                                    is_glass_like=(k % 5 == 0), refractive_index=1.3)))
    dup.lights.append(pkg.create_light(pkg.Vec3f(0., 10., 0.), pkg.Vec3f(1., 1., 1.), 1.))
    scenes.append(dup)
    # spheres whose radii double along the view axis: a surface-area split peels one off per
    # level (depth ~ count, beyond the wave's 64-entry stack); the builder must cap the depth
    # (rm_bvh.hpp) and the image must still be the flat walk's
    chain = pkg.Scene.new()
    z, r = -1e-5, 1e-6
    for k in range(100):
        z -= 1.5 * r
        chain.shapes.append(pkg.sphere.create(pkg.Vec3f(0.9 * r * (k % 3 - 1), 0.7 * r * (k % 5 - 2), z), r,
                                              pkg.Reflectance(diffuse_color=(0.2 + 0.007 * k, 0.9 - 0.007 * k, 0.5),
                                                              is_glass_like=(k % 3 == 0), refractive_index=1.2)))
        z -= 1.5 * r
        r *= 2.
    chain.lights.append(pkg.create_light(pkg.Vec3f(5., 10., 5.), pkg.Vec3f(1., 1., 1.), 1.))
    scenes.append(chain)
    monkeypatch.setenv("RM_DISABLE_BVH", "1")
    flat_ctx = pkg.backend.Context(0)
    monkeypatch.delenv("RM_DISABLE_BVH")
    try:
        for scene in scenes:
            a, _ = gpu_render(pkg, ctx, scene, 384, 256, 6)
            b, _ = gpu_render(pkg, flat_ctx, scene, 384, 256, 6)
            assert np.array_equal(a, b)
            assert a.sum() > 0
    finally:
        flat_ctx.close()


def test_bundle_cull_equals_plain_walk_bitwise(pkg, ctx, monkeypatch):
    """The ray-bundle cull (rm_trace.inc: cone of the wave's rays against bounding spheres and,
    for planar primitives, the planes through the apex and their edges) only decides WHICH
    primitives a wave tests: with it switched off (RM_DISABLE_CULL=1: every bundle counts as
    wide) the image must be the same bit for bit.  Scenes: the Cornell box from its corner (the
    camera lies IN the planes of floor and wall, and floor / ceiling can never be hit: all
    vertices at one y), the 256 spheres, the demo scene forced through the cull kernel
    (RM_CULL_MIN=1), random meshes + polygons + spheres seen from inside, cameras on the move."""
    rng = np.random.default_rng(23)
    mixed = pkg.Scene.new()
    tri = (rng.uniform(-20., 20., size=(60, 1, 3)) + rng.uniform(-4., 4., size=(60, 3, 3))).reshape(60, 9)
    mixed.shapes.append(pkg.obj.Obj(tri))
    for k in range(10):
        c = rng.uniform(-15., 15., 3)
        quad = [c + np.array(v) for v in ((3., 0., 1.), (0., 3., -1.), (-3., 0., 1.), (0., -3., -1.))]   # not planar: lifted
        mixed.shapes.append(pkg.polygon.ConvexPolygon.create([pkg.Vec3f(*q) for q in quad],
                                                             pkg.Reflectance(diffuse_color=(0.3, 0.8, 0.4), is_glass_like=(k % 2 == 0),
                                                                             refractive_index=1.4, reflection=0.4)))
    for k in range(12):
        mixed.shapes.append(pkg.sphere.create(pkg.Vec3f(*rng.uniform(-12., 12., 3)), float(rng.uniform(0.5, 3.)),
                                              pkg.Reflectance(diffuse_color=tuple(rng.uniform(0, 1, 3)), is_glass_like=(k % 3 == 0),
                                                              refractive_index=1.5, reflection=0.3)))
    mixed.lights.append(pkg.create_light(pkg.Vec3f(0., 0., 0.), pkg.Vec3f(1., 1., 1.), 1.))
    mixed.lights.append(pkg.create_light(pkg.Vec3f(8., 30., 5.), pkg.Vec3f(1., .5, .5), .8))
    jobs = [(workloads.product_scene(pkg, "cornell"), [(0., 0., 0.), (100., 100., 20.), (278., 273., -800.)]),
            (workloads.product_scene(pkg, "synthetic256"), [(0., 0., 0.), (5., 2., -30.)]),
            (pkg.Scene.create_default(), [(0., 0., 0.), (0., 5., 0.), (-5., 0., -10.)]),
            (mixed, [(0., 0., 0.), (1., 2., 3.), (0., 0., 40.)])]
    monkeypatch.setenv("RM_CULL_MIN", "1")
    cull_ctx = pkg.backend.Context(0)
    monkeypatch.setenv("RM_DISABLE_CULL", "1")
    plain_ctx = pkg.backend.Context(0)
    monkeypatch.delenv("RM_DISABLE_CULL")
    monkeypatch.delenv("RM_CULL_MIN")
    try:
        lit = 0
        for scene, cams in jobs:
            for cam in cams:
                scene.camera = pkg.Vec3f(*cam)
                a, _ = gpu_render(pkg, cull_ctx, scene, 320, 224, 6)
                b, _ = gpu_render(pkg, plain_ctx, scene, 320, 224, 6)
                assert np.array_equal(a, b), "cull changed the image (camera %s)" % (cam,)
                c, _ = gpu_render(pkg, ctx, scene, 320, 224, 6)     # the default context's choice of kernel
                assert float(np.abs(a - c).max()) < 1e-12           # (it may sum a pixel's terms in another order)
                lit += int((a.sum(axis=2) > 0).sum())
        assert lit > 0
    finally:
        cull_ctx.close()
        plain_ctx.close()


def test_tile_classification_is_bitwise_invisible(pkg, O, monkeypatch):
    """The classification launch in front of the render launch (rm_classify.hip: one lane per tile tests the
    cone of the tile's primary rays against every primitive's bounds; tiles nothing can be hit in are
    filled there and get no wave, the others are listed with the primitives their primary rays can reach)
    only decides WHICH tiles get a wave and which primitives their primary rays test: every frame must
    equal the frame of a context without it bit for bit -- f64 and display bytes, into buffers pre-filled
    with a sentinel -- for the demo scene, the Cornell box (from outside and from inside it), 256 spheres
    (list only: more primitives than a mask holds), cameras inside and behind things, bands and strided
    packed bands, tiny frames whose tiles are wider than the cone test allows, and a scene seen from a
    camera at a NaN (everything kept)."""
    import torch
    monkeypatch.setenv("RM_TILE_CLASSIFY", "0")
    plain = pkg.backend.Context(0)
    monkeypatch.setenv("RM_TILE_CLASSIFY", "1")
    cls = pkg.backend.Context(0)
    monkeypatch.delenv("RM_TILE_CLASSIFY")
    demo = pkg.Scene.create_default()
    cornell = workloads.product_scene(pkg, "cornell")
    synth = workloads.product_scene(pkg, "synthetic256")
    mixed = pkg.Scene()
    refl = pkg.Reflectance.create_default()
    glass = pkg.Reflectance.create_default()
    glass.is_glass_like, glass.refractive_index, glass.reflection = True, 1.5, 0.3
    for k in range(9):
        mixed.shapes.append(pkg.sphere.create(pkg.Vec3f(-8. + 2. * k, -1. + 0.5 * (k % 3), -14. - k), 0.9, glass if k % 3 == 0 else refl))
    mixed.shapes.append(pkg.polygon.ConvexPolygon.create([pkg.Vec3f(-9., -3., -4.), pkg.Vec3f(9., -3., -4.), pkg.Vec3f(9., -2., -30.), pkg.Vec3f(-9., -2., -30.)][::-1], refl))
    mixed.shapes.append(pkg.polygon.ConvexPolygon.create([pkg.Vec3f(0., 4., -20.), pkg.Vec3f(-2., 2., -21.), pkg.Vec3f(0., 0., -20.), pkg.Vec3f(2., 1., -19.), pkg.Vec3f(2., 3., -19.)], refl))
    mixed.lights.append(pkg.create_light(pkg.Vec3f(0., 10., 0.), pkg.Vec3f(1., 1., 1.), 1.))
    cases = [(demo, (0., 0., 0.), 1920, 1080, 5, None), (demo, (0., 5., 0.), 640, 352, 5, None), (demo, (-5., 0., -16.), 640, 352, 6, None),
             (demo, (0., 0., -60.), 640, 352, 4, None), (demo, (0., 0., 0.), 64, 64, 3, None), (demo, (0., 0., 0.), 1920, 1080, 5, (3, 30, 4)),
             (cornell, (0., 0., 0.), 1920, 1080, 5, None), (cornell, (0., 1., -498.), 800, 608, 3, None), (cornell, (3., 0.5, -300.), 640, 352, 3, (1, 9)),
             (synth, (0., 0., 0.), 1024, 768, 6, None), (synth, (2., 1., -30.), 640, 352, 8, None),
             (mixed, (0., 0., 0.), 800, 608, 5, None), (mixed, (0., 2., -12.), 640, 352, 5, None), (demo, (float("nan"), 0., 0.), 320, 224, 3, None)]
    try:
        for k, (scene, cam, w, h, depth, band) in enumerate(cases):
            scene.camera = pkg.Vec3f(*cam)
            p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth, band)
            p.flags = _FLAGS["value"]
            outs = []
            for c in (plain, cls):
                c.upload(scene.flatten())
                f64 = torch.full((h, w, 3), -1., dtype=torch.float64, device="cuda:0")
                u8 = torch.full((h, w, 3), 201, dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                c.render_device_u8(p, f64.data_ptr(), u8.data_ptr())
                c.render_device_u8(p, f64.data_ptr(), u8.data_ptr())      # (a second frame: the counters take turns)
                torch.cuda.synchronize()
                outs.append((f64.cpu().numpy(), u8.cpu().numpy()))
            assert outs[0][0].tobytes() == outs[1][0].tobytes(), "case %d: f64 frame differs with the classification on" % k
            assert np.array_equal(outs[0][1], outs[1][1]), "case %d: display bytes differ" % k
            if band is None and cam[0] == cam[0]:
                n = h // 32 * 32
                assert not (outs[1][0][:n] == -1.).any()
        # against the oracle once, through the classified path
        demo.camera = pkg.Vec3f(0., 0., 0.)
        got, _ = gpu_render(pkg, cls, demo, 640, 352, 5)
        compare(got, O.render(O.OracleScene.create_default(), 640, 352, max_depth=5))
        # packed display bytes of a strided band (a rank's chunk of the gather buffer)
        w, h = 640, 352
        p = pkg.backend.make_params(workloads.FOV, float(h), float(w), 5, (1, 11, 3))
        p.flags = _FLAGS["value"] | 4                               # RM_FLAG_U8_COMPACT
        packs = []
        for c in (plain, cls):
            c.upload(demo.flatten())
            f64 = torch.full((h, w, 3), -1., dtype=torch.float64, device="cuda:0")
            u8 = torch.full((4 * 32, w, 3), 201, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            c.render_device_u8(p, f64.data_ptr(), u8.data_ptr())
            torch.cuda.synchronize()
            packs.append((f64.cpu().numpy(), u8.cpu().numpy()))
        assert packs[0][0].tobytes() == packs[1][0].tobytes() and np.array_equal(packs[0][1], packs[1][1])
        assert not (packs[1][1] == 201).all(axis=2).any()
    finally:
        plain.close()
        cls.close()


def test_patch_order_renders_every_tile_once(pkg, monkeypatch):
    """Dispatch order from the launch's own classification (rm_classify.inc place_patch, rm_render_kernel.inc order_entry):
    the classifying workgroups at a launch's head put every patch behind the first round into a bucket -- by the previous
    frame's tile times while the view stands, by the cost of what the patch can reach once it has moved, by place where
    there is nothing to go by -- and the render waves take the k-th patch of the buckets laid end to end.  Only the ORDER
    of dispatch may change: every frame of a sequence on one stream -- the same camera for several frames, a moved camera,
    another size, a band, another scene and back -- must equal the frame of a context without it bit for bit, f64 and
    display bytes, in buffers pre-filled with a sentinel (a patch missing from the order, or in it twice, would show).
    RM_FIRST_ROUND makes the first round small enough for frames of a few thousand tiles to have an order at all."""
    import torch
    monkeypatch.setenv("RM_PATCH_ORDER", "0")
    plain = pkg.backend.Context(0)
    monkeypatch.setenv("RM_PATCH_ORDER", "1")
    monkeypatch.setenv("RM_TILE_CLASSIFY", "1")
    ctxs = {}
    for name, env in (("default", {}), ("round256", {"RM_FIRST_ROUND": "256"}), ("round0", {"RM_FIRST_ROUND": "0"}),
                      ("by_place", {"RM_FIRST_ROUND": "64", "RM_ORDER_KEYS": "0"}), ("by_time", {"RM_FIRST_ROUND": "64", "RM_ORDER_KEYS": "1"}),
                      ("by_content", {"RM_FIRST_ROUND": "64", "RM_ORDER_KEYS": "2"}),
                      ("tags_wrap", {"RM_FIRST_ROUND": "128", "RM_ORD_TAG_WRAP": "3"}), ("no_tail", {"RM_FIRST_ROUND": "128", "RM_SKY_TAIL": "0"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctxs[name] = pkg.backend.Context(0)
        for k in env:
            monkeypatch.delenv(k)
    monkeypatch.setenv("RM_TILE_CLASSIFY", "0")
    ctxs["unclassified"] = pkg.backend.Context(0)
    monkeypatch.delenv("RM_TILE_CLASSIFY")
    monkeypatch.delenv("RM_PATCH_ORDER")
    demo = pkg.Scene.create_default()
    cornell = workloads.product_scene(pkg, "cornell")
    seq = [(demo, (0., 0., 0.), 640, 352, 5, None)] * 4 + [(demo, (0., 5., 0.), 640, 352, 5, None)] * 2 + \
          [(demo, c, 640, 352, 5, None) for c in workloads.camera_walk()[:10]] + \
          [(demo, (0., 5., 0.), 800, 608, 4, None)] * 3 + [(demo, (0., 0., 0.), 800, 608, 4, (2, 17, 3))] * 3 + \
          [(cornell, (0., 0., 0.), 640, 352, 3, None)] * 3 + [(cornell, (5., 0., 5.), 640, 352, 3, None)] * 2 + \
          [(demo, (1., 0., 1.), 1920, 1080, 5, None)] * 3 + [(demo, (6., 0., 1.), 1920, 1080, 5, None), (demo, (6., 5., 1.), 1920, 1080, 5, None)]
    try:
        for k, (scene, cam, w, h, depth, band) in enumerate(seq):
            scene.camera = pkg.Vec3f(*cam)
            p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth, band)
            p.flags = _FLAGS["value"]
            outs = {}
            for name, c in [("plain", plain)] + list(ctxs.items()):
                if os.environ.get("RM_TEST_TRACE"):
                    print("frame", k, name, cam, w, h, depth, band, flush=True)
                c.upload(scene.flatten())
                f64 = torch.full((h, w, 3), -1., dtype=torch.float64, device="cuda:0")
                u8 = torch.full((h, w, 3), 201, dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                c.render_device_u8(p, f64.data_ptr(), u8.data_ptr())
                torch.cuda.synchronize()
                outs[name] = (f64.cpu().numpy(), u8.cpu().numpy())
            for name in ctxs:
                assert outs["plain"][0].tobytes() == outs[name][0].tobytes(), "frame %d of the sequence: f64 differs with the dispatch order on (%s)" % (k, name)
                assert np.array_equal(outs["plain"][1], outs[name][1]), "frame %d: display bytes differ (%s)" % (k, name)
            if band is None:
                assert not (outs["default"][0][:h // 32 * 32] == -1.).any()
    finally:
        plain.close()
        for c in ctxs.values():
            c.close()


def test_sky_tail_renders_every_patch_once(pkg, monkeypatch):
    """Sky tail (rm_device.hip): the places of the dispatch order that hold patches nothing can be hit in get one wave instead
    of sixteen -- how many, the host takes from a hint the earlier launches left in page-locked memory.  From a frame of the
    view being rendered the count is exact; from an earlier view it is a guess, and the places it gets wrong are rendered by
    sixteen waves each behind the grid's end (while there is room: RM_SKY_TAIL_CAP) or by the tail's own wave, tile by tile.
    Only the launch's geometry may be carried over: every frame of a sequence on one stream -- a view held for several frames
    (the tail arms itself), a moved camera, bands, display bytes, another scene -- must equal the frame of a context without
    it bit for bit in buffers pre-filled with a sentinel; so must the frames of contexts whose hint is WRONG (RM_SKY_TAIL_FORCE:
    the last 37 places of the order, or every place, taken for sky whatever the earlier frames said), with room to hand on
    all, some or none of them."""
    import torch
    monkeypatch.setenv("RM_PATCH_ORDER", "1")
    monkeypatch.setenv("RM_TILE_CLASSIFY", "1")
    monkeypatch.setenv("RM_FIRST_ROUND", "256")                     # (frames of a few hundred patches: all but sixteen of them have a place in the order)
    monkeypatch.setenv("RM_SKY_TAIL", "0")
    plain = pkg.backend.Context(0)
    monkeypatch.setenv("RM_SKY_TAIL", "1")
    monkeypatch.setenv("RM_SKY_TAIL_MOTION", "0")                   # (no guesses: a hint only from frames of the view being rendered)
    tail = pkg.backend.Context(0)
    monkeypatch.delenv("RM_SKY_TAIL_MOTION")
    moving = pkg.backend.Context(0)                                 # (the default: a moved view takes the hint as a guess)
    monkeypatch.setenv("RM_SKY_TAIL_PLACE", "even")                 # (the tail's waves dealt out among the tile waves, not behind them)
    monkeypatch.setenv("RM_FIRST_ROUND", "0")
    tail_even = pkg.backend.Context(0)
    monkeypatch.delenv("RM_SKY_TAIL_PLACE")
    monkeypatch.setenv("RM_FIRST_ROUND", "256")
    monkeypatch.setenv("RM_PATCH_ORDER_MAX", "100")                 # (larger launches: no tile is timed, the order is bottom-up less the sky)
    monkeypatch.setenv("RM_SKY_TAIL_BIG_MIN", "0")
    monkeypatch.setenv("RM_SKY_TAIL_BIG", "1")
    by_place = pkg.backend.Context(0)
    monkeypatch.delenv("RM_PATCH_ORDER_MAX")
    monkeypatch.delenv("RM_SKY_TAIL_BIG_MIN")
    monkeypatch.delenv("RM_SKY_TAIL_BIG")
    monkeypatch.setenv("RM_SKY_TAIL_FORCE", "37")
    wrong_some = pkg.backend.Context(0)
    monkeypatch.setenv("RM_SKY_TAIL_CAP", "5")
    wrong_some_little_room = pkg.backend.Context(0)
    monkeypatch.setenv("RM_SKY_TAIL_CAP", "0")
    wrong_some_no_room = pkg.backend.Context(0)
    monkeypatch.delenv("RM_SKY_TAIL_CAP")
    monkeypatch.setenv("RM_SKY_TAIL_FORCE", "100000")
    wrong_all = pkg.backend.Context(0)
    for v in ("RM_SKY_TAIL_FORCE", "RM_SKY_TAIL", "RM_TILE_CLASSIFY", "RM_PATCH_ORDER", "RM_FIRST_ROUND"):
        monkeypatch.delenv(v)
    demo = pkg.Scene.create_default()
    cornell = workloads.product_scene(pkg, "cornell")
    seq = [(demo, (0., 0., 0.), 640, 352, 5, None)] * 6 + [(demo, (0., 5., 0.), 640, 352, 5, None)] * 5 + \
          [(demo, (0., 5. + k, -2. * k), 640, 352, 5, None) for k in range(4)] + \
          [(demo, (0.5 * k, 0.3 * k, -0.4 * k), 640, 352, 5, None) for k in range(8)] + \
          [(demo, c, 640, 352, 5, None) for c in workloads.camera_walk()[:12]] + \
          [(demo, (0., 0., 0.), 800, 608, 4, (2, 17, 3))] * 5 + [(cornell, (0., 0., 0.), 640, 352, 3, None)] * 6 + \
          [(cornell, (3. * k, 2. * k, -5. * (k % 3)), 640, 352, 3, None) for k in range(1, 9)] + \
          [(demo, (1., 0., 1.), 1920, 1080, 5, None)] * 4 + [(demo, (1., 0., 11.), 1920, 1080, 5, None), (demo, (1., 0., 1.), 1920, 1080, 5, None)]
    names = ("tail", "moving", "tail_even", "by_place", "wrong_some", "wrong_some_little_room", "wrong_some_no_room", "wrong_all")
    armed = {n: 0 for n in names}
    armed_on_a_new_view = 0
    ctxs = (plain, tail, moving, tail_even, by_place, wrong_some, wrong_some_little_room, wrong_some_no_room, wrong_all)
    try:
        for k, (scene, cam, w, h, depth, band) in enumerate(seq):
            scene.camera = pkg.Vec3f(*cam)
            p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth, band)
            p.flags = _FLAGS["value"]
            outs = []
            for name, c in zip(("plain",) + names, ctxs):
                if os.environ.get("RM_TEST_TRACE"):
                    print("frame", k, name, cam, w, h, depth, band, flush=True)
                c.upload(scene.flatten())
                f64 = torch.full((h, w, 3), -1., dtype=torch.float64, device="cuda:0")
                u8 = torch.full((h, w, 3), 201, dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                c.render_device_u8(p, f64.data_ptr(), u8.data_ptr())
                torch.cuda.synchronize()
                outs.append((f64.cpu().numpy(), u8.cpu().numpy()))
                grid, n_tail = c.launch_stats()
                if name == "plain":
                    assert n_tail == 0
                else:
                    armed[name] += n_tail > 0
                # without guesses a hint is taken only from frames of the view being rendered: none in the first frame of a
                # view; with them (the default) a view that has moved keeps the tail -- what it gets wrong is handed on
                new_view = k < 1 or seq[k][:4] != seq[k - 1][:4] or seq[k][5] != seq[k - 1][5]
                if name == "tail" and new_view:
                    assert n_tail == 0, "frame %d (%s): %d patches in the tail of a view that is new" % (k, name, n_tail)
                if name == "moving" and new_view:
                    armed_on_a_new_view += n_tail > 0
            for j in range(1, len(ctxs)):
                assert outs[0][0].tobytes() == outs[j][0].tobytes(), "frame %d of the sequence: f64 differs with the sky tail on (%s)" % (k, names[j - 1])
                assert np.array_equal(outs[0][1], outs[j][1]), "frame %d: display bytes differ (%s)" % (k, names[j - 1])
            if band is None:
                assert not (outs[1][0][:h // 32 * 32] == -1.).any()
        # the tail armed itself where a view was held, and the wrong hints were in force
        assert armed["tail"] >= 8 and armed["tail_even"] >= 8 and armed["by_place"] >= 8, armed
        assert armed["moving"] > armed["tail"] and armed_on_a_new_view >= 10, (armed, armed_on_a_new_view)
        assert min(armed[n] for n in names if n.startswith("wrong")) >= 15, armed
    finally:
        for c in ctxs:
            c.close()


def test_a_wait_that_is_given_up_voids_the_frame_and_says_so(pkg, monkeypatch):
    """The one wait of a render launch that has no fallback: a wave behind the first round needs its place in the
    dispatch order, which is there once every classifying workgroup of the launch has said it is done -- they are the
    launch's first workgroups and take microseconds.  A test hook keeps the launch's last classifying workgroup from laying
    the order out: each wave gives up after 10 ms, renders nothing and says so in page-locked memory.  The asynchronous launch
    has returned by then; the NEXT call on the stream must report the void frame (once), the synchronous calls report
    their own, and the context must come down cleanly."""
    import torch
    monkeypatch.setenv("RM_PATCH_ORDER", "1")
    monkeypatch.setenv("RM_TILE_CLASSIFY", "1")
    monkeypatch.setenv("RM_FIRST_ROUND", "1024")
    monkeypatch.setenv("RM_TEST_STALL_ORDER", "1")
    c = pkg.backend.Context(0)
    for v in ("RM_PATCH_ORDER", "RM_TILE_CLASSIFY", "RM_FIRST_ROUND", "RM_TEST_STALL_ORDER"):
        monkeypatch.delenv(v)
    try:
        w, h = 640, 352
        c.upload(pkg.Scene.create_default().flatten())
        p = pkg.backend.make_params(workloads.FOV, float(h), float(w), 5)
        p.flags = _FLAGS["value"]
        f64 = torch.full((h, w, 3), -1., dtype=torch.float64, device="cuda:0")
        u8 = torch.full((h, w, 3), 201, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        c.render_device_u8(p, f64.data_ptr(), u8.data_ptr())          # returns at once; its waves give up 10 ms later
        torch.cuda.synchronize()
        got = f64.cpu().numpy()
        assert (got[:h // 32 * 32] == -1.).any(), "the stalled launch rendered every tile all the same"
        with pytest.raises(pkg.BackendError) as e:
            c.render_device_u8(p, f64.data_ptr(), u8.data_ptr())
        assert "void" in str(e.value)
        # said once: the next launch is taken (and stalls like the first); a synchronous call reports its own frame
        host = np.zeros((h, w, 3))
        with pytest.raises(pkg.BackendError) as e:
            c.render(p, host)
            c.render(p, host)
        assert "void" in str(e.value)
        torch.cuda.synchronize()
    finally:
        c.close()


def test_a_wave_out_of_patience_gets_the_order_of_last_resort(pkg, monkeypatch):
    """Where a launch dispatches by its own order, the waves behind the first round wait for the classifying workgroups -- which
    on a card shared with another process may be kept off it for as long as that takes.  A wave that runs out of patience
    turns the launch's decision word to "the order of last resort" (unless the workgroups got there first: compare and swap):
    then nobody writes places and EVERY wave takes its patch from the index the launch came with -- slower, and correct.  A test
    hook keeps the classifying workgroups of such launches from ever arriving: every frame of a sequence -- the view moving,
    standing (launches that dispatch by the order of a predecessor that never laid one out), a sky tail whose hint is wrong --
    must equal the frame of a context without any of it, in buffers pre-filled with a sentinel, and no frame may be void."""
    import torch
    monkeypatch.setenv("RM_PATCH_ORDER", "0")
    plain = pkg.backend.Context(0)
    monkeypatch.setenv("RM_PATCH_ORDER", "1")
    monkeypatch.setenv("RM_TILE_CLASSIFY", "1")
    monkeypatch.setenv("RM_FIRST_ROUND", "512")
    monkeypatch.setenv("RM_TEST_STALL_ORDER", "2")
    stalled = pkg.backend.Context(0)
    monkeypatch.setenv("RM_SKY_TAIL_FORCE", "60")
    stalled_wrong_tail = pkg.backend.Context(0)
    for v in ("RM_PATCH_ORDER", "RM_TILE_CLASSIFY", "RM_FIRST_ROUND", "RM_TEST_STALL_ORDER", "RM_SKY_TAIL_FORCE"):
        monkeypatch.delenv(v)
    demo = pkg.Scene.create_default()
    seq = [(0., 0., 0.)] * 4 + [(5., 0., 0.), (5., 0., 5.), (5., 0., 5.), (5., 0., 5.), (5., 0., 5.), (0., 5., 5.)]
    try:
        w, h = 800, 608
        p = pkg.backend.make_params(workloads.FOV, float(h), float(w), 5)
        p.flags = _FLAGS["value"]
        for k, cam in enumerate(seq):
            demo.camera = pkg.Vec3f(*cam)
            outs = []
            for c in (plain, stalled, stalled_wrong_tail):
                c.upload(demo.flatten())
                f64 = torch.full((h, w, 3), -1., dtype=torch.float64, device="cuda:0")
                u8 = torch.full((h, w, 3), 201, dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                c.render_device_u8(p, f64.data_ptr(), u8.data_ptr())      # (raises if an earlier frame was void)
                torch.cuda.synchronize()
                outs.append((f64.cpu().numpy(), u8.cpu().numpy()))
            for j in (1, 2):
                assert outs[0][0].tobytes() == outs[j][0].tobytes(), "frame %d: f64 differs under the order of last resort (%d)" % (k, j)
                assert np.array_equal(outs[0][1], outs[j][1]), "frame %d: display bytes differ (%d)" % (k, j)
            assert not (outs[1][0][:h // 32 * 32] == -1.).any()
    finally:
        for c in (plain, stalled, stalled_wrong_tail):
            c.close()


def test_three_hundred_frames_of_a_camera_on_the_move(pkg, O, monkeypatch):
    """300 launches of one geometry on one stream, the camera a press further before each (workloads.camera_walk: the
    reference's own offsets): the tags of the tile masks (8 bits) and of the dispatch order (made to start afresh every
    100 launches here) wrap, the keys change from times by place to cost by content and back, guessed sky tails hand
    places on.  The last frame against the oracle; every 50th against a context that does none of it."""
    import torch
    monkeypatch.setenv("RM_PATCH_ORDER", "0")
    monkeypatch.setenv("RM_TILE_CLASSIFY", "0")
    plain = pkg.backend.Context(0)
    monkeypatch.setenv("RM_PATCH_ORDER", "1")
    monkeypatch.setenv("RM_TILE_CLASSIFY", "1")
    monkeypatch.setenv("RM_FIRST_ROUND", "512")
    monkeypatch.setenv("RM_ORD_TAG_WRAP", "100")
    c = pkg.backend.Context(0)
    for v in ("RM_PATCH_ORDER", "RM_TILE_CLASSIFY", "RM_FIRST_ROUND", "RM_ORD_TAG_WRAP"):
        monkeypatch.delenv(v)
    try:
        w, h, depth = 800, 608, 5
        scene = pkg.Scene.create_default()
        c.upload(scene.flatten()); plain.upload(scene.flatten())
        p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)
        p.flags = _FLAGS["value"]
        f64 = torch.full((h, w, 3), -1., dtype=torch.float64, device="cuda:0")
        u8 = torch.full((h, w, 3), 201, dtype=torch.uint8, device="cuda:0")
        g64 = torch.full((h, w, 3), -1., dtype=torch.float64, device="cuda:0")
        g8 = torch.full((h, w, 3), 201, dtype=torch.uint8, device="cuda:0")
        walk = workloads.camera_walk()
        tails = 0
        for k in range(300):
            cam = walk[k % len(walk)] if k % 7 else walk[(k - 1) % len(walk)]     # (now and then the camera stays where it was)
            c.set_camera(pkg.Vec3f(*cam))
            if k % 50 == 49 or k == 299:
                f64.fill_(-1.); u8.fill_(201)
                torch.cuda.synchronize()
            c.render_device_u8(p, f64.data_ptr(), u8.data_ptr())
            tails += c.launch_stats()[1] > 0
            if k % 50 == 49 or k == 299:
                plain.set_camera(pkg.Vec3f(*cam))
                plain.render_device_u8(p, g64.data_ptr(), g8.data_ptr())
                torch.cuda.synchronize()
                assert f64.cpu().numpy().tobytes() == g64.cpu().numpy().tobytes(), "frame %d differs" % k
                assert torch.equal(u8, g8), "frame %d: display bytes differ" % k
        assert tails >= 100, tails
        os_ = O.OracleScene.create_default()
        os_.set_camera(cam)
        compare(f64.cpu().numpy()[:h // 32 * 32], O.render(os_, w, h, max_depth=depth)[:h // 32 * 32])
    finally:
        plain.close()
        c.close()


def test_feedback_order_renders_every_tile_once(pkg, ctx, monkeypatch):
    """Frame-to-frame feedback (rm_device.hip, rm_feedback): the tiles that took long in the
    previous frame on a stream are dispatched first in the next.  Only the ORDER of dispatch may
    change: every frame of a sequence -- same camera, moved camera, another frame size, another
    scene in between -- must equal the frame of a context without feedback bit for bit.  Forced
    on for every launch (RM_FEEDBACK=1): with fixed thresholds (RM_FEEDBACK_TARGET=0) that put nearly
    every tile (1 us: the list overflows its capacity), some tiles (8 us) and hardly any tile (200 us)
    on the list, and with the threshold taken from the previous frame's histogram of tile times so
    that the list holds about 40 tiles / as many as it is allowed to (the default's two per wave slot
    exceed half the list's capacity at these frame sizes)."""
    monkeypatch.setenv("RM_FEEDBACK", "0")
    plain = pkg.backend.Context(0)
    monkeypatch.setenv("RM_FEEDBACK", "1")
    ctxs = []
    for us, target in (("1", "0"), ("8", "0"), ("200", "0"), ("50", "40"), ("50", None)):
        monkeypatch.setenv("RM_FEEDBACK_US", us)
        if target is None:
            monkeypatch.delenv("RM_FEEDBACK_TARGET")
        else:
            monkeypatch.setenv("RM_FEEDBACK_TARGET", target)
        ctxs.append(pkg.backend.Context(0))
    monkeypatch.delenv("RM_FEEDBACK_US")
    monkeypatch.delenv("RM_FEEDBACK")
    synth = workloads.product_scene(pkg, "synthetic256")
    demo = pkg.Scene.create_default()
    seq = [(synth, (0., 0., 0.), 512, 384, 8), (synth, (0., 0., 0.), 512, 384, 8), (synth, (0., 0., 0.), 512, 384, 8),
           (synth, (2., 1., -5.), 512, 384, 8), (synth, (2., 1., -5.), 512, 384, 10), (synth, (2., 1., -5.), 640, 352, 10),
           (demo, (0., 0., 0.), 640, 352, 5), (demo, (0., 5., 0.), 640, 352, 5), (demo, (0., 5., 0.), 640, 352, 5),
           (synth, (0., 0., 0.), 640, 352, 6), (synth, (0., 0., 0.), 640, 352, 6)]
    try:
        for k, (scene, cam, w, h, depth) in enumerate(seq):
            scene.camera = pkg.Vec3f(*cam)
            want, _ = gpu_render(pkg, plain, scene, w, h, depth)
            assert (want.sum(axis=2) > 0).any()
            for c in ctxs:
                # into a caller-owned DEVICE buffer pre-filled with a sentinel: rm_render copies rows out of
                # the context's own framebuffer, where a tile left out would still show the previous frame
                got = device_render_with_sentinel(pkg, c, scene, w, h, depth)
                assert np.array_equal(got[:h // 32 * 32], want[:h // 32 * 32]), "frame %d of the sequence differs with feedback on" % k
                assert np.all(got[h // 32 * 32:] == -1.)
        # bands of a sharded frame (another launch geometry on the same stream, back and forth)
        for band in ((0, 11, 2), (1, 11, 2), (0, 11, 2)):
            want = np.zeros((352, 640, 3)); got = np.zeros((352, 640, 3))
            gpu_render(pkg, plain, synth, 640, 352, 6, band=band, out=want)
            gpu_render(pkg, ctxs[1], synth, 640, 352, 6, band=band, out=got)
            assert np.array_equal(got, want)
    finally:
        plain.close()
        for c in ctxs:
            c.close()


# ---------------------------------------------------------------- properties at full size
def test_bands_tile_the_frame_bitwise(pkg, ctx):
    """Row sharding: the union of per-rank bands is bit-identical to the
    single-GPU frame, for even and uneven splits, at the 8K configuration."""
    c = workloads.CONFIGS["C4"]
    w, h, depth = c["width"], c["height"], c["max_depth"]
    scene = pkg.Scene.create_default()
    full, _ = gpu_render(pkg, ctx, scene, w, h, depth)
    n_rows = h // 32
    for world in (8, 3):
        parts = np.zeros_like(full)
        for r in range(world):
            band = workloads.patch_rows_for_rank(n_rows, r, world)
            gpu_render(pkg, ctx, scene, w, h, depth, band=band, out=parts)
        assert np.array_equal(full, parts)
    assert [workloads.patch_rows_for_rank(135, r, 8) for r in range(8)][-1] == (118, 135)


@pytest.mark.parametrize("world", [2, 3, 8])
def test_cyclic_rows_and_packed_display_bytes(pkg, ctx, world):
    """bench.py's N > 1 path without the network: every rank renders patch rows r, r+N, ...
    (rm_params stride) into its own full-size f64 frame and packs the display bytes of its
    rows (RM_FLAG_U8_COMPACT) into its chunk of the gather buffer; the union of the f64 rows
    and the de-interleaved chunks must equal the single-GPU frame bit for bit."""
    import torch
    c = workloads.CONFIGS["C2"]
    w, h, depth = c["width"], c["height"], c["max_depth"]
    n_rows = h // 32
    ctx.upload(pkg.Scene.create_default().flatten())
    full = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    full8 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")
    p = pkg.backend.make_params(1.5, float(h), float(w), depth)
    p.flags = _FLAGS["value"]
    ctx.render_device_u8(p, full.data_ptr(), full8.data_ptr())
    torch.cuda.synchronize()

    chunk_rows, owned = workloads.cyclic_rows(n_rows, world)
    assert sorted(r for rows in owned for r in rows) == list(range(n_rows))
    assert max(len(r) for r in owned) - min(len(r) for r in owned) <= 1
    parts = torch.zeros_like(full)
    gathered = torch.full((world * chunk_rows * 32, w, 3), 9, dtype=torch.uint8, device="cuda:0")
    for r in range(world):
        pr = pkg.backend.make_params(1.5, float(h), float(w), depth, band=(r, n_rows, world))
        pr.flags = _FLAGS["value"] | 4                                   # RM_FLAG_U8_COMPACT
        chunk = gathered[r * chunk_rows * 32:(r + 1) * chunk_rows * 32]
        ctx.render_device_u8(pr, parts.data_ptr(), chunk.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(parts, full)
    display = workloads.deinterleave_rows(gathered, world, torch.zeros_like(gathered))
    assert torch.equal(display[:n_rows * 32], full8[:n_rows * 32])

    # the host-copy entry point honours the stride too: only owned rows are written
    out = np.full((h, w, 3), -2.)
    pr = pkg.backend.make_params(1.5, float(h), float(w), depth, band=(1, n_rows, world))
    pr.flags = _FLAGS["value"]
    ctx.render(pr, out)
    ref = full.cpu().numpy()
    for row in range(n_rows):
        blk = out[row * 32:(row + 1) * 32]
        if row % world == 1:
            assert np.array_equal(blk, ref[row * 32:(row + 1) * 32])
        else:
            assert np.all(blk == -2.)
    assert np.all(out[n_rows * 32:] == -2.)


@pytest.mark.parametrize("world", [1, 2, 5, 8])
def test_frame_submit_layout_of_n_ranks_on_one_gpu(pkg, world):
    """rm_frame_submit (the C ABI's multi-GPU frame) with the layout of `world` ranks and no
    transport (rm_comm_init with a NULL id): the ranks take turns on this one GPU, each
    writes its cyclic rows and its chunk of the shared gather buffer, and the consumer's
    de-interleaved display frame must be the single-GPU frame bit for bit."""
    import torch
    c = workloads.CONFIGS["C2"]
    w, h, depth = c["width"], c["height"], c["max_depth"]
    n_rows = h // 32
    cx = pkg.backend.Context(0)
    cx.upload(pkg.Scene.create_default().flatten())
    p = pkg.backend.make_params(1.5, float(h), float(w), depth)
    p.flags = _FLAGS["value"]
    full = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    full8 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")
    cx.render_device_u8(p, full.data_ptr(), full8.data_ptr())
    torch.cuda.synchronize()

    rows, chunk = cx.exchange_layout(p, world)
    assert rows == -(-n_rows // world) and chunk == rows * 32 * w * 3
    parts = torch.zeros_like(full)
    gathered = torch.full((world * chunk,), 7, dtype=torch.uint8, device="cuda:0")
    display = torch.full((n_rows * 32, w, 3), 9, dtype=torch.uint8, device="cuda:0")
    for r in range(world):
        cx.comm_init(r, world)
        last = r == world - 1
        cx.frame_submit(p, parts.data_ptr(), gathered.data_ptr(), display.data_ptr() if last else None, slot=r % 4)
        cx.frame_wait(r % 4)
    assert torch.equal(parts, full)
    assert torch.equal(display, full8[:n_rows * 32])
    with pytest.raises(pkg.BackendError):                       # the band is the library's business here
        cx.frame_submit(pkg.backend.make_params(1.5, float(h), float(w), depth, band=(0, 4)), parts.data_ptr(),
                        gathered.data_ptr())
    cx.close()


def test_frame_submit_through_rccl_world_of_one(pkg):
    """The RCCL leg with the one rank this box has: communicator from rm_comm_unique_id /
    rm_comm_init, several frames in flight over the slots (each on a stream of its own),
    camera moved between frames; every slot's display and f64 frame must equal the plain
    single-stream render of the same camera."""
    import torch
    c = workloads.CONFIGS["SHOT"]
    w, h, depth = c["width"], c["height"], c["max_depth"]
    n_rows = h // 32
    cx = pkg.backend.Context(0)
    scene = pkg.Scene.create_default()
    cx.upload(scene.flatten())
    cx.comm_init(0, 1, pkg.backend.Context.comm_unique_id())
    p = pkg.backend.make_params(1.5, float(h), float(w), depth)
    p.flags = _FLAGS["value"]
    n_slots = 4
    f64 = [torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0") for _ in range(n_slots)]
    g8 = [torch.zeros((n_rows * 32, w, 3), dtype=torch.uint8, device="cuda:0") for _ in range(n_slots)]
    d8 = [torch.zeros((n_rows * 32, w, 3), dtype=torch.uint8, device="cuda:0") for _ in range(n_slots)]
    cams = [(0., 0., 0.), (0., 5., 0.), (-5., 0., 0.), (0., 0., -5.), (5., 5., 0.), (0., 0., 0.), (0., -5., 5.), (5., 0., 0.)]
    for k, cam in enumerate(cams):                              # two rounds over the slots
        cx.set_camera(cam)
        cx.frame_submit(p, f64[k % n_slots].data_ptr(), g8[k % n_slots].data_ptr(), d8[k % n_slots].data_ptr(), slot=k % n_slots)
    for s in range(n_slots):
        cx.frame_wait(s)
    ref = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    ref8 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")
    for s in range(n_slots):
        cx.set_camera(cams[n_slots + s])
        cx.render_device_u8(p, ref.data_ptr(), ref8.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(f64[s], ref), "slot %d f64" % s
        assert torch.equal(d8[s], ref8[:n_rows * 32]) and torch.equal(g8[s], ref8[:n_rows * 32]), "slot %d u8" % s
    cx.close()


def test_feedback_with_frames_in_flight(pkg, monkeypatch):
    """Frame-to-frame feedback under rm_frame_submit: every frame slot renders on a stream of its
    own and keeps feedback sets of its own; three ranks' cyclic bands (layout without a transport,
    the ranks taking turns on this GPU, rank r on slot r) over four rounds with the camera moving
    every other round -- each round's assembled frame must be the single-GPU frame of a context
    without feedback, bit for bit (f64 rows and display bytes)."""
    import torch
    w, h, depth, world = 640, 352, 8, 3
    n_rows = h // 32
    scene = workloads.product_scene(pkg, "synthetic256")
    monkeypatch.setenv("RM_FEEDBACK", "0")
    plain = pkg.backend.Context(0)
    monkeypatch.setenv("RM_FEEDBACK", "1")
    monkeypatch.setenv("RM_FEEDBACK_TARGET", "24")
    cx = pkg.backend.Context(0)
    monkeypatch.delenv("RM_FEEDBACK_TARGET")
    monkeypatch.delenv("RM_FEEDBACK")
    try:
        p = pkg.backend.make_params(1.5, float(h), float(w), depth)
        p.flags = _FLAGS["value"]
        rows, chunk = cx.exchange_layout(p, world)
        full = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
        full8 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")
        for rnd, cam in enumerate([(0., 0., 0.), (0., 0., 0.), (1., 1., -4.), (1., 1., -4.)]):
            scene.camera = pkg.Vec3f(*cam)
            plain.upload(scene.flatten())
            cx.upload(scene.flatten())
            plain.render_device_u8(p, full.data_ptr(), full8.data_ptr())
            torch.cuda.synchronize()
            parts = torch.full((h, w, 3), -1., dtype=torch.float64, device="cuda:0")
            gathered = torch.full((world * chunk,), 7, dtype=torch.uint8, device="cuda:0")
            display = torch.full((n_rows * 32, w, 3), 9, dtype=torch.uint8, device="cuda:0")
            for r in range(world):
                cx.comm_init(r, world)
                cx.frame_submit(p, parts.data_ptr(), gathered.data_ptr(), display.data_ptr() if r == world - 1 else None, slot=r)
                cx.frame_wait(r)                                # (the last rank de-interleaves what the others wrote)
            assert torch.equal(parts, full), "round %d: f64 rows" % rnd
            assert torch.equal(display, full8[:n_rows * 32]), "round %d: display bytes" % rnd
    finally:
        plain.close()
        cx.close()


@pytest.mark.parametrize("world", [1, 2, 5, 8])
def test_frame_submit_f64_layout_of_n_ranks_on_one_gpu(pkg, world):
    """rm_frame_submit_f64: the f64 rows themselves travel (framebuffer.rs:6-22: the reference's
    render target is f64).  Layout of `world` ranks without a transport, the ranks taking turns
    on this GPU: each renders its cyclic rows PACKED into its chunk of the gather buffer, the
    consumer's de-interleaved f64 frame must be the single-GPU frame bit for bit."""
    import torch
    c = workloads.CONFIGS["SHOT"]
    w, h, depth = c["width"], c["height"], c["max_depth"]
    n_rows = h // 32
    cx = pkg.backend.Context(0)
    cx.upload(pkg.Scene.create_default().flatten())
    p = pkg.backend.make_params(1.5, float(h), float(w), depth)
    p.flags = _FLAGS["value"]
    full = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    cx.render_device(p, full.data_ptr())
    torch.cuda.synchronize()
    rows, chunk = cx.exchange_layout(p, world)
    gathered = torch.full((world * chunk,), -3., dtype=torch.float64, device="cuda:0")
    frame = torch.full((n_rows * 32, w, 3), -5., dtype=torch.float64, device="cuda:0")
    cx.frame_timing_enable(True)
    for r in range(world):
        cx.comm_init(r, world)
        last = r == world - 1
        cx.frame_submit_f64(p, gathered.data_ptr(), frame.data_ptr() if last else None, slot=r % 4)
        cx.frame_wait(r % 4, timeout_ms=20000)
        t = cx.frame_timing(r % 4)
        assert 0. < t.kernel_ms <= t.total_ms and t.gather_ms >= 0.
    assert torch.equal(frame, full[:n_rows * 32])
    assert cx.comm_info() == (world - 1, world, 0)              # no transport: no communicator
    cx.close()


def test_frame_submit_f64_through_rccl_world_of_one(pkg):
    """The same through a real communicator (of the one rank this box has), frames in flight
    on all slots; what the communicator itself reports is echoed by rm_comm_info."""
    import torch
    c = workloads.CONFIGS["SHOT"]
    w, h, depth = c["width"], c["height"], c["max_depth"]
    n_rows = h // 32
    cx = pkg.backend.Context(0)
    cx.upload(pkg.Scene.create_default().flatten())
    cx.comm_init(0, 1, pkg.backend.Context.comm_unique_id())
    assert cx.comm_info() == (0, 1, 1)
    p = pkg.backend.make_params(1.5, float(h), float(w), depth)
    p.flags = _FLAGS["value"]
    g = [torch.zeros((n_rows * 32, w, 3), dtype=torch.float64, device="cuda:0") for _ in range(4)]
    f = [torch.zeros((n_rows * 32, w, 3), dtype=torch.float64, device="cuda:0") for _ in range(4)]
    cams = [(0., 0., 0.), (0., 5., 0.), (-5., 0., 0.), (0., 0., -5.)]
    for k, cam in enumerate(cams):
        cx.set_camera(cam)
        cx.frame_submit_f64(p, g[k].data_ptr(), f[k].data_ptr(), slot=k)
    ref = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    for k, cam in enumerate(cams):
        cx.frame_wait(k)
        cx.set_camera(cam)
        cx.render_device(p, ref.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(f[k], ref[:n_rows * 32]) and torch.equal(g[k], ref[:n_rows * 32]), "slot %d" % k
    cx.close()


def test_frame_wait_is_bounded(pkg):
    """rm_frame_wait_for gives up with RM_ERR_TIMEOUT instead of hanging the host: here the
    slot's stream is held up by a long render queued in front (8K frames), and a 1 ms bound
    must come back as a status; a generous bound then completes."""
    import torch
    cx = pkg.backend.Context(0)
    cx.upload(workloads.product_scene(pkg, "synthetic256").flatten())
    w, h = 4096, 4096
    p = pkg.backend.make_params(1.5, float(h), float(w), 10)
    f = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    g = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")
    cx.comm_init(0, 1)
    for _ in range(3):
        cx.frame_submit(p, f.data_ptr(), g.data_ptr(), None, slot=0)
    with pytest.raises(pkg.BackendError) as e:
        cx.frame_wait(0, timeout_ms=1)
    assert e.value.status == pkg._lib.RM_ERR_TIMEOUT
    torch.cuda.synchronize()
    cx.close()


def test_destroy_after_a_timeout_that_could_not_be_aborted_does_not_wait_for_the_device(pkg, monkeypatch):
    """After RM_ERR_TIMEOUT the host reports and exits.  Where RCCL cannot abort the communicator
    (ncclCommAbort absent or failing -- simulated by RM_TEST_NO_COMM_ABORT) the stuck collective
    never ends, and rm_destroy must not call anything that waits for the device (hipFree does):
    it releases nothing device-side and returns."""
    import time

    import torch
    monkeypatch.setenv("RM_TEST_NO_COMM_ABORT", "1")
    cx = pkg.backend.Context(0)
    cx.upload(workloads.product_scene(pkg, "synthetic256").flatten())
    w, h = 4096, 4096
    p = pkg.backend.make_params(1.5, float(h), float(w), 10)
    f = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    g = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")
    cx.comm_init(0, 1, pkg.backend.Context.comm_unique_id())          # a real communicator of one rank
    for _ in range(3):
        cx.frame_submit(p, f.data_ptr(), g.data_ptr(), None, slot=0)
    with pytest.raises(pkg.BackendError) as e:
        cx.frame_wait(0, timeout_ms=1)
    assert e.value.status == pkg._lib.RM_ERR_TIMEOUT
    t0 = time.perf_counter()
    cx.close()
    assert time.perf_counter() - t0 < 5.
    torch.cuda.synchronize()                                           # (here the frames do complete: nothing is really stuck)


def test_upload_of_the_resident_scene_is_not_repeated_and_a_changed_one_is(pkg, O):
    """rm_scene_upload compares the device image it builds with the resident one: the same
    scene again (any camera) costs no copy; any change of a primitive, material or light does,
    and the next frame shows it.  rm_render's band-by-band device -> host overlap (frames of
    8 MB and more) must deliver the same frame as the single-launch path."""
    cx = pkg.backend.Context(0)
    scene = pkg.Scene.create_default()
    w, h, depth = 1920, 1080, 5
    a, _ = gpu_render(pkg, cx, scene, w, h, depth)
    assert cx.uploads() == (1, 1)
    scene.camera = pkg.Vec3f(0., 5., 0.)
    b, _ = gpu_render(pkg, cx, scene, w, h, depth)
    assert cx.uploads() == (2, 1) and not np.array_equal(a, b)
    so = O.OracleScene.create_default(); so.set_camera((0., 5., 0.))
    # (the demo from (0, 5, 0): the view with the line of tie pixels, test_resolution_sweep)
    compare(b, O.render(so, w, h, max_depth=depth), tie=TR.Tie(so, w, h, depth))
    scene.lights[1] = pkg.create_light(pkg.Vec3f(20., 20., 20.), pkg.Vec3f(1., .5, .5), 0.5)
    c, _ = gpu_render(pkg, cx, scene, w, h, depth)
    assert cx.uploads() == (3, 2) and not np.array_equal(b, c)
    # the frame that came through the host path against a device-resident render of the same frame
    import torch
    dev = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)
    p.flags = _FLAGS["value"]
    cx.render_device(p, dev.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), c)
    # identity is decided on the bytes of the description, not on a digest of them: flipping the
    # sign bit of an EVEN number of doubles (mirroring a sphere in x and y) is exactly what a
    # multiplicative word hash cannot see in its top bit
    mirrored = pkg.Scene()
    mirrored.camera = pkg.Vec3f(0., 5., 0.)
    plain = pkg.Scene()
    plain.camera = pkg.Vec3f(0., 5., 0.)
    for sc, sx in ((plain, 1.), (mirrored, -1.)):
        sc.shapes.append(pkg.sphere.create(pkg.Vec3f(3. * sx, 2. * sx, -12.), 2., pkg.Reflectance.create_default()))
        sc.lights.append(pkg.create_light(pkg.Vec3f(0., 0., 0.), pkg.Vec3f(1., 1., 1.), 1.))
    e, _ = gpu_render(pkg, cx, plain, 320, 224, 3)
    calls, copies = cx.uploads()
    f, _ = gpu_render(pkg, cx, mirrored, 320, 224, 3)
    assert cx.uploads() == (calls + 1, copies + 1) and not np.array_equal(e, f)
    cx.close()


def test_render_is_deterministic(pkg, ctx):
    c = workloads.CONFIGS["C2"]
    scene = pkg.Scene.create_default()
    a, _ = gpu_render(pkg, ctx, scene, c["width"], c["height"], c["max_depth"])
    b, _ = gpu_render(pkg, ctx, scene, c["width"], c["height"], c["max_depth"])
    assert np.array_equal(a, b)


def test_depth_caps_beyond_natural_depth_agree_at_full_size(pkg, ctx):
    """the demo ray tree ends at depth 4, so caps 5, 8 and 10 give the same
    image; cap 3 differs."""
    scene = pkg.Scene.create_default()
    frames = {d: gpu_render(pkg, ctx, scene, 1920, 1080, d)[0] for d in (3, 5, 8, 10)}
    assert np.array_equal(frames[5], frames[8]) and np.array_equal(frames[8], frames[10])
    assert not np.array_equal(frames[3], frames[5])


def test_render_device_into_torch_buffer(pkg, O, ctx):
    """rm_render_device: caller-owned device memory + caller's stream (the path bench.py
    and the multi-GPU gather use)."""
    import torch
    w, h = 640, 352
    ctx.upload(pkg.Scene.create_default().flatten())
    buf = torch.full((h, w, 3), -3., dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()                                               # (the fill runs on torch's default stream, the render on another)
    stream = torch.cuda.Stream()
    p = pkg.backend.make_params(1.5, float(h), float(w), 5, band=(2, 9))
    with torch.cuda.stream(stream):
        ctx.render_device(p, buf.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    got = buf.cpu().numpy()
    ref = np.full((h, w, 3), -3.)
    O.render(O.OracleScene.create_default(), w, h, max_depth=5, frame=ref, band=(2, 9))
    compare(got, ref)
    assert np.all(got[:64] == -3.) and np.all(got[288:] == -3.)


def test_render_device_u8_display_bytes(pkg, O, ctx):
    """rm_render_device_u8: the fused epilogue writes fb.to_vec() of the band
    (framebuffer.rs:40-55: clamp, x255, truncate -- no normalisation) next to the f64 rows."""
    import torch
    w, h, depth = 640, 352, 5
    ctx.upload(pkg.Scene.create_default().flatten())
    f64 = torch.full((h, w, 3), -3., dtype=torch.float64, device="cuda:0")
    u8 = torch.full((h, w, 3), 201, dtype=torch.uint8, device="cuda:0")
    p = pkg.backend.make_params(1.5, float(h), float(w), depth, band=(1, 10))
    p.flags = _FLAGS["value"]
    torch.cuda.synchronize()                                               # (the fills run on torch's default stream, the render on another)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.render_device_u8(p, f64.data_ptr(), u8.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    ref = np.full((h, w, 3), -3.)
    O.render(O.OracleScene.create_default(), w, h, max_depth=depth, frame=ref, band=(1, 10))
    compare(f64.cpu().numpy(), ref)
    got8 = u8.cpu().numpy()
    assert np.all(got8[:32] == 201) and np.all(got8[320:] == 201)          # outside the band: untouched
    want8 = O.to_vec(ref[32:320].copy()).reshape(288, w, 3)
    n_diff = int((got8[32:320] != want8).sum())
    assert n_diff <= 2, "%d display bytes differ" % n_diff                 # truncation at k/255 +- 1 ulp
    assert got8[32:320].max() == 255 and got8[32:320].min() == 0
    p.max_depth = 0
    with pytest.raises(pkg.BackendError):
        ctx.render_device_u8(p, f64.data_ptr(), u8.data_ptr())


# ---------------------------------------------------------------- post-process (8f.1)
def test_postprocess_normalize_and_quantize(pkg, O, ctx):
    import torch
    rng = np.random.default_rng(3)
    frame = rng.uniform(-0.5, 3.0, size=(96, 160, 3))
    frame[5, 7, 1] = np.nan
    frame[9, 9] = [0., 1., 255. / 255.]
    for normalize in (0, 1):
        dev = torch.from_numpy(frame.copy()).cuda()
        out8 = np.empty(frame.size, dtype=np.uint8)
        mx = C.c_double()
        pkg._lib.check(pkg.lib().rm_postprocess(ctx.ptr, C.c_void_p(dev.data_ptr()), 160, 96, normalize,
                                                out8.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(mx)), ctx.ptr)
        ref = frame.copy()
        if normalize:
            O.normalize(ref)
            assert mx.value == np.nanmax(frame)
            got = dev.cpu().numpy()
            assert np.array_equal(got[~np.isnan(ref)], ref[~np.isnan(ref)])
        assert np.array_equal(out8, O.to_vec(ref))
    # all-zero frame: max == 0 leaves it untouched (framebuffer.rs:69)
    dev = torch.zeros((32, 32, 3), dtype=torch.float64, device="cuda")
    pkg._lib.check(pkg.lib().rm_postprocess(ctx.ptr, C.c_void_p(dev.data_ptr()), 32, 32, 1, None, None), ctx.ptr)
    assert float(dev.abs().max()) == 0.


# ---------------------------------------------------------------- reference-shaped surface
def test_reference_call_sequence(pkg, O, capsys):
    """main.rs:119-123 + 329-357: default scene, create_renderer(1.5, h, w), render,
    normalize, write_ppm -- through the Python mirror of the reference's API."""
    fb = pkg.create_frame_buffer(800, 600)
    scene = pkg.Scene.create_default()
    r = pkg.create_renderer(1.5, fb.height, fb.width)
    msg = r.render(fb, scene)
    out = capsys.readouterr().out
    assert "Rendering using patches of size 32, using 450 patches overall" in out
    assert "Dimensions mismatch" in out
    assert msg.startswith("Scene rendered in ") and msg.endswith("MP/s)")
    ref = O.render(O.OracleScene.create_default(), 800, 600, max_depth=3)
    compare(fb.buffer, ref)
    fb.normalize()
    O.normalize(ref)
    assert float(np.abs(fb.buffer - ref).max()) < TIGHT
    u8 = fb.to_vec()
    assert int((u8 != O.to_vec(ref)).sum()) <= 2


def test_smoke_entry(entry):
    entry.smoke()
