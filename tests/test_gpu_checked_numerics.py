"""GPU: the checked numerics of the strict plain-walk kernels (rm_trace.inc RM_CHECKED) change no bit of any picture.

Numerics, argument by argument (rmi_numerics_probe, an internal export): the range-free square root, the reciprocal
of its rounded value and the discriminant's root beside the compiler's __builtin_sqrt and `/` on the same device -- v_rsq_f64
and v_rcp_f64 cannot be emulated on a CPU.  Every argument inside the guarded range [2^-600, 2^600] gives identical bits
and leaves the guard silent -- the norms whose significand is all ones included, the classical hard case of a
residual-corrected reciprocal (and the norm of every nearly unit vector an ulp short of 1); every argument outside the
range, 0, -0, inf, NaN, denormals and negative numbers fire the guard.

Frames: a context as it comes and one with RM_CHECKED_NUMERICS=0 (every launch exact only: the compiler's sequences
throughout) render bit-equal f64 frames and display bytes into sentinel-filled buffers.  The count of tiles rendered again
(rmi_redone_tiles) says which path a scene took: zero for the benchmark's views, more than zero where a light sits exactly
on a visible hit point, zero and "exact only" where the upload or the plan routes the launch to the exact code."""
import ctypes as C
import os

import numpy as np
import pytest

import workloads
from test_shadow_masks import build_pair, random_shapes

pytestmark = pytest.mark.gpu

LO, HI = -600, 600                                   # the guarded range of the squared norm: [2^LO, 2^HI]
NORM_DIFF, INV_DIFF, THC_DIFF, OUTSIDE, ONES = 1, 2, 4, 8, 16


# ------------------------------------------------------------------ numerics
def probe(pkg, x):
    f = pkg.lib().rmi_numerics_probe
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64]
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros(x.size, dtype=np.uint8)
    assert f(0, x.ctypes.data, out.ctypes.data, x.size) == 0
    return out


def check_in_range(out, x, label):
    bad = (out & (NORM_DIFF | INV_DIFF | THC_DIFF)) != 0
    assert not bad.any(), "%s: %d arguments differ, first %r (code %d)" % (label, int(bad.sum()), x[bad][0].hex(), out[bad][0])
    fired = (out & OUTSIDE) != 0
    assert not fired.any(), "%s: the guard fires for %d arguments of the range, first %r" % (label, int(fired.sum()), x[fired][0].hex())


def test_random_arguments_bit_equal(pkg):
    """1e8 seeded arguments: exponent uniform over the guarded range, significand uniform."""
    rng = np.random.default_rng(0xC4EC4ED)
    total, ones = 0, 0
    for chunk in range(10):
        n = 10_000_000
        e = rng.integers(1023 + LO, 1023 + HI, n, dtype=np.uint64)          # 2^LO <= x < 2^HI
        m = rng.integers(0, 1 << 52, n, dtype=np.uint64)
        x = ((e << np.uint64(52)) | m).view(np.float64)
        out = probe(pkg, x)
        check_in_range(out, x, "chunk %d" % chunk)
        total += n
        ones += int(((out & ONES) != 0).sum())
    print("random arguments: %d, all bit-equal; %d norms with an all-ones significand among them" % (total, ones))
    assert total >= 100_000_000


def test_hard_significands_in_every_binade(pkg):
    """Every binade of the range: the all-ones significand and its three neighbours below, the power of two and its three
    neighbours above -- for x, and for the x whose rounded root has them (x = s^2 rounded down, to nearest and up)."""
    sig = np.array([0, 1, 2, 3, (1 << 52) - 1, (1 << 52) - 2, (1 << 52) - 3, (1 << 52) - 4], dtype=np.uint64)
    e = np.arange(1023 + LO, 1023 + HI, dtype=np.uint64)
    x = ((e[:, None] << np.uint64(52)) | sig[None, :]).view(np.float64).ravel()
    # norms with those significands, in every binade of the norm: squares, and their neighbours
    en = np.arange(1023 + LO // 2, 1023 + HI // 2, dtype=np.uint64)
    s = ((en[:, None] << np.uint64(52)) | sig[None, :]).view(np.float64).ravel().astype(np.longdouble)
    sq = (s * s).astype(np.float64)
    sq = sq[(sq >= 2. ** LO) & (sq < 2. ** HI)]
    near = np.concatenate([sq, np.nextafter(sq, 0.), np.nextafter(sq, np.inf), np.nextafter(np.nextafter(sq, 0.), 0.),
                           np.nextafter(np.nextafter(sq, np.inf), np.inf)])
    near = near[(near >= 2. ** LO) & (near <= 2. ** HI)]
    allx = np.concatenate([x, near, [2. ** HI, 2. ** LO]])
    out = probe(pkg, allx)
    check_in_range(out, allx, "hard significands")
    n_ones = int(((out & ONES) != 0).sum())
    print("hard significands: %d arguments, all bit-equal; %d norms with an all-ones significand among them" % (allx.size, n_ones))
    assert n_ones >= (HI - LO) // 2 - 2, "the family of all-ones norms was not reached"


def test_small_integer_vectors(pkg):
    """Squared norms of vectors with small-integer and zero components (the reference's scenes produce exact-incidence
    rays), as they are and scaled by powers of four and two."""
    k = np.arange(0, 48, dtype=np.float64)
    a, b, c = np.meshgrid(k, k, k, indexing="ij")
    x = (a * a + b * b + c * c).ravel()
    x = np.unique(x[x > 0.])
    allx = np.concatenate([x * 2. ** p for p in (0, -2, 2, -1, 1, -40, 40, -400, 400)])
    out = probe(pkg, allx)
    check_in_range(out, allx, "integer vectors")
    assert ((out & OUTSIDE) == 0).all()


def test_outside_arguments_fire_the_guard(pkg):
    tiny = np.array([1, 2, (1 << 52) - 1], dtype=np.uint64).view(np.float64)           # denormals
    x = np.concatenate([[0., -0., np.inf, -np.inf, np.nan, -np.nan, -1., -1e-300, -2. ** 100],
                        tiny, [2. ** -1030, 2. ** -1022, 2. ** -800, 2. ** -767, 2. ** -700],
                        [np.nextafter(2. ** LO, 0.), 2. ** (LO - 1) * 1.5, np.nextafter(2. ** HI, np.inf), 2. ** (HI + 1), 2. ** 700, 2. ** 1000,
                         np.finfo(np.float64).max],
                        np.nan * np.ones(3)])
    out = probe(pkg, x)
    silent = (out & OUTSIDE) == 0
    assert not silent.any(), "the guard is silent for %r" % [v.hex() for v in x[silent]]


# ------------------------------------------------------------------ frames
class Pair:
    """A context as it comes (`on`) and one whose every launch is exact only (`off`, RM_CHECKED_NUMERICS=0 at rm_init)."""

    def __init__(self, pkg):
        old = os.environ.get("RM_CHECKED_NUMERICS")
        try:
            os.environ["RM_CHECKED_NUMERICS"] = "0"
            self.off = pkg.backend.Context(0)
            os.environ.pop("RM_CHECKED_NUMERICS")
            self.on = pkg.backend.Context(0)
        finally:
            if old is None:
                os.environ.pop("RM_CHECKED_NUMERICS", None)
            else:
                os.environ["RM_CHECKED_NUMERICS"] = old
        self.pkg = pkg
        f = pkg.lib().rmi_redone_tiles
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        self._redone = f

    def redone(self, ctx):
        """(tiles the context's launches have rendered again so far, was its last launch exact only?)"""
        n, e = C.c_uint64(0), C.c_uint32(0)
        assert self._redone(ctx.ptr, C.byref(n), C.byref(e)) == 0
        return n.value, bool(e.value)

    def close(self):
        self.on.close()
        self.off.close()


@pytest.fixture(scope="module")
def pair(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    p = Pair(pkg)
    yield p
    p.close()


def render(pkg, ctx, w, h, depth, flags=0):
    """-> (f64 frame, display bytes) of one launch into buffers filled with sentinels."""
    import torch
    p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)
    p.flags = flags
    f64 = torch.full((h, w, 3), -7.25, dtype=torch.float64, device="cuda:0")
    u8 = torch.full((h, w, 3), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.render_device_u8(p, f64.data_ptr(), u8.data_ptr())
    torch.cuda.synchronize()
    return f64.cpu().numpy(), u8.cpu().numpy()


def both(pair, scene, w, h, depth, camera=None, look_at=None, label=""):
    """Renders with both contexts, asserts bit-equality, -> (frame, tiles `on` rendered again, was `on` exact only?)."""
    pkg = pair.pkg
    got = []
    before, _ = pair.redone(pair.on)
    for c in (pair.on, pair.off):
        c.upload(scene.flatten())
        c.orient(None)
        if camera is not None:
            c.set_camera(camera)
        if look_at is not None:
            c.look_at(*look_at)
        got.append(render(pkg, c, w, h, depth))
    (a, a8), (b, b8) = got
    same = a.view(np.uint64) == b.view(np.uint64)
    assert same.all(), "%s: %d f64 values differ" % (label, int((~same).sum()))
    assert np.array_equal(a8, b8), "%s: display bytes differ" % label
    rows = h - h % 32
    assert not (a[:rows] == -7.25).any(), "%s: pixels never written" % label
    after, exact = pair.redone(pair.on)
    n_off, exact_off = pair.redone(pair.off)
    assert n_off == 0 and exact_off, "%s: the reference context left the exact code" % label
    return a, after - before, exact


def test_demo_three_cameras(pkg, pair):
    scene = workloads.product_scene(pkg, "demo")
    walk = workloads.camera_walk()
    for cam in (walk[0], walk[len(walk) // 3], walk[2 * len(walk) // 3]):
        frame, redone, exact = both(pair, scene, 1920, 1080, 5, camera=cam, label="demo %s" % (cam,))
        assert frame[:1056].any() and redone == 0 and not exact
    # ... and turned (the oriented camera's kernels)
    frame, redone, exact = both(pair, scene, 1920, 1080, 5, look_at=((6., 4., 5.), (0., -1., -14.)), label="demo turned")
    assert frame[:1056].any() and redone == 0 and not exact


def test_glass_stack(pkg, pair):
    glass = dict(diffusion=0.3, diffuse_color=(0.9, 0.8, 0.7), specular=0.9, specular_exponent=20.,
                 is_glass_like=True, reflection=0.4, refractive_index=1.5)
    V, R = pkg.Vec3f, pkg.Reflectance(**glass)
    s = pkg.Scene.new()
    for k in range(13):
        z, tilt = -4. - 1.25 * k, 0.05 * k
        s.shapes.append(pkg.polygon.ConvexPolygon.create([V(-12., -9., z - tilt), V(12., -9., z + tilt), V(12., 9., z + tilt), V(-12., 9., z - tilt)], R))
    s.shapes.append(pkg.sphere.create(V(1.5, 0.5, -30.), 6., R))
    s.lights.append(pkg.create_light(V(0., 10., 0.), V(1., 1., 1.), 1.))
    for depth in (5, 16):
        both(pair, s, 256, 224, depth, label="glass stack depth %d" % depth)
    # ... and few enough panes for the plain-walk kernels (under 12 primitives), total reflection inside the sphere included
    s.shapes = s.shapes[:6] + s.shapes[13:]
    for depth in (5, 9):
        _, redone, exact = both(pair, s, 256, 224, depth, label="six panes depth %d" % depth)
        assert redone == 0 and not exact


@pytest.mark.parametrize("seed", range(12))
def test_random_scenes(pkg, O, pair, seed):
    shapes, lights = random_shapes(seed)
    scene, _ = build_pair(pkg, O, shapes, lights)
    # (every other scene with glass: the refracted ray's normalisation, the hoisted 1 / ri)
    if seed % 2:
        for k, sh in enumerate(scene.shapes):
            if hasattr(sh, "reflectance") and k % 2 == 0:
                sh.reflectance = pkg.Reflectance(diffusion=0.4, diffuse_color=(0.8, 0.9, 0.7), specular=0.8, specular_exponent=30.,
                                                 is_glass_like=True, reflection=0.3, refractive_index=1.1 + 0.1 * k)
    both(pair, scene, 256, 192, 5, label="seed %d" % seed)


QUAD = [(-2., -2., -4.), (2., -2., -4.), (2., 2., -4.), (-2., 2., -4.)]      # edges 4 x 4: the cross product is (0, 0, 16)


def quad_scene(pkg, light, sphere=None):
    V = pkg.Vec3f
    s = pkg.Scene.new()
    s.shapes.append(pkg.polygon.ConvexPolygon.create([V(*p) for p in QUAD], pkg.Reflectance()))
    if sphere is not None:
        s.shapes.append(pkg.sphere.create(V(*sphere[0]), sphere[1], pkg.Reflectance()))
    s.lights.append(pkg.create_light(V(*light), V(1., 1., 1.), 1.))
    return s


def test_light_on_a_hit_point_is_redone(pkg, pair):
    """Camera at the origin, 64 x 64: the centre pixel's ray is exactly (0, 0, -1), meets the square in z = -4 (unit normal
    exactly (0, 0, 1)) at exactly (0, 0, -4) -- where the light is: the light vector of that pixel is the zero vector."""
    frame, redone, exact = both(pair, quad_scene(pkg, (0., 0., -4.)), 64, 64, 3, camera=(0., 0., 0.), label="light on the hit point")
    assert redone > 0 and not exact
    assert frame[32, 32].tolist() != [0., 0., 0.]
    # the light a little off: nothing to render again
    _, redone, exact = both(pair, quad_scene(pkg, (0., 0., -3.5)), 64, 64, 3, camera=(0., 0., 0.), label="light off the hit point")
    assert redone == 0 and not exact


def test_routes_to_the_exact_code(pkg, pair):
    # a sphere whose radius_square is 2^-800: the upload says exact only
    _, redone, exact = both(pair, quad_scene(pkg, (3., 3., 0.), sphere=((0., 0., -3.), 2. ** -400)), 64, 64, 3, camera=(0., 0., 0.), label="r^2 = 2^-800")
    assert redone == 0 and exact
    # coordinates of 1e200 in the scene
    _, redone, exact = both(pair, quad_scene(pkg, (3., 3., 0.), sphere=((1e200, 0., -3.), 1.)), 64, 64, 3, camera=(0., 0., 0.), label="centre at 1e200")
    assert redone == 0 and exact
    _, redone, exact = both(pair, quad_scene(pkg, (1e200, 3., 0.)), 64, 64, 3, camera=(0., 0., 0.), label="light at 1e200")
    assert redone == 0 and exact
    # ... and in the camera: the plan says so, launch by launch
    scene = quad_scene(pkg, (3., 3., 0.), sphere=((1., 0., -3.), 1.))
    _, redone, exact = both(pair, scene, 64, 64, 3, camera=(1e200, 0., 0.), label="camera at 1e200")
    assert redone == 0 and exact
    _, redone, exact = both(pair, scene, 64, 64, 3, camera=(float("nan"), 0., 0.), label="camera at NaN")
    assert redone == 0 and exact
    _, redone, exact = both(pair, scene, 64, 64, 3, camera=(0., 0., 0.), label="camera home again")
    assert redone == 0 and not exact


def test_benchmark_views_redo_nothing(pkg, pair):
    """C2, C2 at 4K, C4 and every view of the camera walk: a tile rendered again there would mean that lanes without a ray
    reach a guarded site."""
    import torch
    ctx = pair.on
    ctx.orient(None)
    ctx.upload(workloads.product_scene(pkg, "demo").flatten())
    before, _ = pair.redone(ctx)
    for name in ("C2", "C2_4K", "C4"):
        c = workloads.CONFIGS[name]
        ctx.set_camera((0., 0., 0.))
        dev = torch.empty((c["height"], c["width"], 3), dtype=torch.float64, device="cuda:0")
        p = pkg.backend.make_params(workloads.FOV, float(c["height"]), float(c["width"]), c["max_depth"])
        for _ in range(3):
            ctx.render_device(p, dev.data_ptr())
        torch.cuda.synchronize()
        n, exact = pair.redone(ctx)
        assert n == before and not exact, name
        del dev
    c = workloads.CONFIGS["C2"]
    dev = torch.empty((c["height"], c["width"], 3), dtype=torch.float64, device="cuda:0")
    p = pkg.backend.make_params(workloads.FOV, float(c["height"]), float(c["width"]), c["max_depth"])
    walk = workloads.camera_walk()
    assert len(walk) >= 240
    for cam in walk:
        ctx.set_camera(cam)
        ctx.render_device(p, dev.data_ptr())
    torch.cuda.synchronize()
    n, exact = pair.redone(ctx)
    assert n == before and not exact, "%d tiles of the walk's %d views were rendered again" % (n - before, len(walk))
    # ... and the walk seen through the oriented camera
    for cam in walk[::8]:
        ctx.look_at(cam, (0., -1., -14.))
        ctx.render_device(p, dev.data_ptr())
    torch.cuda.synchronize()
    n, exact = pair.redone(ctx)
    ctx.orient(None)
    assert n == before and not exact, "%d tiles of the turned views were rendered again" % (n - before)
