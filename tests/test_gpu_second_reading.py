"""The kernels held DIRECTLY to the second reading of the reference (tests/second_reading.py): the oracle is not in the
loop.  Strict flavour only -- the fast flavour's differing pixels are tests/tie_reference.py's business.

Expected values are read by the second reading on the host when the module's first test runs, every scene once, in
processes of their own (tests/second_reading_scenes.py), and kept for the module.

  rm_render                                    32x32 and 64x39 frames: every channel within TIGHT, remainder rows zero
  rm_intersect_rays, rm_primary_hits_device    hit / miss and shape index equal, hit point within TIGHT
  rm_radiance_rays                             depth caps 1, 3, 6: every channel within TIGHT of the second reading's cast_ray
  rm_scene_offset_shape                        a moved Cornell mesh, a moved demo polygon: the 32x32 render within TIGHT

Largest deviations measured on an MI355X: frames 1.8e-14, radiance 1.8e-14, hit points 0.  The ray sets
start an eighth of their rays ON surfaces: the radiance step's viewer direction is normalize(origin - point) as
renderer.rs:149 has it, and no longer the ray's direction turned round, because of them.
"""
import numpy as np
import pytest

import second_reading_scenes as SC
import test_second_reading as TS
import workloads

pytestmark = pytest.mark.gpu

TIGHT = TS.TIGHT
N_RAYS = 4097                        # 64 waves and one: the last wave has a single live lane
RAY_DEPTHS = [1, 3, 6]
CHUNK = 512

# scene -> depth cap of its frames.  synthetic256 at 6: 257 primitives, the hierarchy walk with its stack of 32.
FRAME_SCENES = {"demo": 3, "cornell": 3, "dodecahedron": 3, "manygons": 6, "synthetic256": 6}
FRAME_FUZZ = [0, 1, 2, 3]
FRAME_CAMERAS = {"demo": ["origin", "inside"], "cornell": ["origin", "inside", "off"], "dodecahedron": ["origin", "inside", "off"]}
RAY_SCENES = ["demo", "cornell", "manygons", "synthetic256", "wrap"]
RADIANCE_SCENES = ["demo", "cornell", "manygons", "synthetic256"]


def wrap_description():
    """tests/test_second_reading.py's scene of 300 spheres in a plane: the closest hit of a ray at sphere k >= 256 has an
    index the reference wraps to u8."""
    import random
    rng = random.Random(20261208)
    centres = [((col - 9.5) * 3., (row - 7.) * 3., -60.) for row in range(15) for col in range(20)]
    return dict(shapes=[("sphere", c, 1., TS.material(rng)) for c in centres], lights=workloads.DEMO_LIGHTS, camera=(0., 0., 0.))


def seeded_rays(desc, seed, n=N_RAYS):
    """n rays of their own origins: uniform in the padded bounds of the scene; half aimed at a point of a random primitive;
    a quarter start INSIDE a sphere (where the scene has spheres), an eighth ON a surface (a point of a polygon or a
    triangle, or of a sphere's surface); directions normalised in doubles."""
    rng = np.random.default_rng(seed)
    prims = []
    for shape in desc["shapes"]:
        if shape[0] == "sphere":
            prims.append(("s", np.array(shape[1], dtype=np.float64), float(shape[2])))
        elif shape[0] == "polygon":
            prims.append(("p", np.array(shape[1], dtype=np.float64), 0.))
        else:
            for t in np.asarray(shape[1], dtype=np.float64).reshape(-1, 3, 3):
                prims.append(("p", t + np.array(shape[2], dtype=np.float64), 0.))
    pts = np.concatenate([p[1].reshape(-1, 3) for p in prims])
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    pad = 0.25 * (hi - lo) + 1.
    o = rng.uniform(lo - pad, hi + pad, size=(n, 3))
    d = rng.normal(size=(n, 3))

    def point_of(prim, inside):
        kind, geom, r = prim
        if kind == "s":
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            return geom + u * (r * (0.9 * rng.uniform() if inside else 1.))
        return (geom * rng.dirichlet(np.ones(len(geom)))[:, None]).sum(axis=0)

    spheres = [p for p in prims if p[0] == "s"]
    for j in range(n // 4):
        if spheres:
            o[j] = point_of(spheres[rng.integers(0, len(spheres))], True)
    for j in range(n // 4, n // 4 + n // 8):
        o[j] = point_of(prims[rng.integers(0, len(prims))], False)
    for j in range(0, n, 2):
        aim = point_of(prims[rng.integers(0, len(prims))], True) - o[j]
        if np.linalg.norm(aim) > 1e-6:
            d[j] = aim
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def concrete(desc):
    """the demo as a description of the other kind (for the ray sets, which aim at primitives): scene.rs:28-211 read off the
    second reading's own create_default"""
    if not desc.get("default"):
        return desc
    import math
    s = SC.second_scene(desc)
    shapes = []
    for shape in s.shapes:
        m = shape.reflectance._asdict()
        if hasattr(shape, "center"):
            shapes.append(("sphere", shape.center, math.sqrt(shape.radius_square), m))
        else:
            shapes.append(("polygon", shape.vertices, m))
    return dict(desc, shapes=shapes)


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected():
    """Everything this module compares against, read by the second reading once."""
    import time
    desc = TS.descriptions()
    desc["wrap"] = wrap_description()
    frames = [(name, cam, size) for name in FRAME_SCENES for cam in FRAME_CAMERAS.get(name, ["origin", "inside"]) for size in TS.SIZES]
    frames += [("fuzz%d" % seed, cam, size) for seed in FRAME_FUZZ for cam in ["origin", "inside"] for size in TS.SIZES]
    depth_of = dict(FRAME_SCENES, **{"fuzz%d" % seed: desc["fuzz%d" % seed]["depth"] for seed in FRAME_FUZZ})
    moved = [(name, dict(desc[name], moves=TS.MOVES[name]), SC.cameras_of(name)[TS.MOVED_CAMERA[name]]) for name in TS.MOVES]
    rays = {name: seeded_rays(concrete(desc[name]), 20261300 + k) for k, name in enumerate(RAY_SCENES)}
    centres = np.array([s[1] for s in desc["wrap"]["shapes"]])                     # a ray at every sphere of the wrap scene
    rays["wrap"][0][-300:] = 0.
    rays["wrap"][1][-300:] = centres / np.linalg.norm(centres, axis=1, keepdims=True)
    jobs = [("frame", desc[name], SC.cameras_of(name)[cam], size[0], size[1], depth_of[name]) for name, cam, size in frames]
    jobs += [("frame", d, eye, 32, 32, 3) for _, d, eye in moved]
    chunks = []
    for name in RAY_SCENES:
        o, d = rays[name]
        for b in range(0, N_RAYS, CHUNK):
            chunks.append(name)
            jobs.append(("rays", desc[name], o[b:b + CHUNK], d[b:b + CHUNK], RAY_DEPTHS if name in RADIANCE_SCENES else []))
    t0 = time.time()
    results = SC.render_jobs(jobs)
    print("second reading: %d frames and %d rays in %.1f s" % (len(frames) + len(moved), N_RAYS * len(RAY_SCENES), time.time() - t0))
    out = dict(desc=desc, depth_of=depth_of, rays=rays, frames={}, moved={}, first={n: [] for n in RAY_SCENES}, rgb={n: [] for n in RAY_SCENES})
    for key, res in zip(frames, results):
        out["frames"][key] = res
    for (name, d, eye), res in zip(moved, results[len(frames):]):
        out["moved"][name] = (d, eye, res)
    for name, res in zip(chunks, results[len(frames) + len(moved):]):
        out["first"][name] += [r[0] for r in res]
        out["rgb"][name] += [r[1] for r in res]
    return out


def upload(pkg, ctx, desc, camera=None):
    scene = SC.product_scene(pkg, desc, camera)
    ctx.upload(scene.flatten())
    return scene


def params(pkg, w, h, depth):
    p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth, None)
    p.flags = 0                                           # the strict flavour
    return p


def hold_frame(gpu, second, what):
    rgb, probes = second
    mine = np.array(rgb, dtype=np.float64)
    rows = mine.shape[0] - mine.shape[0] % 32
    assert gpu.shape == mine.shape and len(probes) == rows * mine.shape[1]
    assert np.all(gpu[rows:] == 0.) and np.all(mine[rows:] == 0.), what
    dev = float(np.abs(gpu - mine).max())
    assert dev < TIGHT, (what, dev)
    return dev


@pytest.mark.parametrize("name", list(FRAME_SCENES) + ["fuzz%d" % s for s in FRAME_FUZZ])
def test_render_against_the_second_reading(pkg, ctx, expected, name):
    worst, lit = 0., 0
    for cam in FRAME_CAMERAS.get(name, ["origin", "inside"]):
        upload(pkg, ctx, expected["desc"][name], SC.cameras_of(name)[cam])
        for w, h in TS.SIZES:
            gpu = np.zeros((h, w, 3), dtype=np.float64)
            ctx.render(params(pkg, w, h, expected["depth_of"][name]), gpu)
            worst = max(worst, hold_frame(gpu, expected["frames"][(name, cam, (w, h))], (name, cam, (w, h))))
            lit += int((gpu.sum(axis=2) > 0.).sum())
    assert lit > 0
    print("%s: largest |GPU - second reading| %.3e over %d lit pixels" % (name, worst, lit))


@pytest.mark.parametrize("name", list(FRAME_SCENES))
def test_primary_hits_against_the_second_reading(pkg, ctx, expected, name):
    """rm_primary_hits_device: under every pixel of the patch rows the second reading's first hit -- decision, shape index
    (none of these scenes has more than 256 shapes... but synthetic256, 257: the floor is shape 256, which the reference
    wraps to 0 and rm_hit.shape, documented as NOT wrapped, reports as 256), and the point within TIGHT."""
    worst, hits = 0., 0
    for cam in FRAME_CAMERAS.get(name, ["origin", "inside"]):
        upload(pkg, ctx, expected["desc"][name], SC.cameras_of(name)[cam])
        for w, h in TS.SIZES:
            got = ctx.primary_hits_device(params(pkg, w, h, expected["depth_of"][name]))
            hit, shape, point = got.hit.cpu().numpy(), got.shape.cpu().numpy(), got.point.cpu().numpy()
            probes = expected["frames"][(name, cam, (w, h))][1]
            for (y, x), p in probes.items():
                assert bool(hit[y, x]) == p[0], (name, cam, (w, h), y, x)
                if p[0]:
                    assert shape[y, x] % 256 == p[1], (name, cam, (w, h), y, x, shape[y, x], p[1])
                    worst = max(worst, float(np.abs(point[y, x] - np.array(p[5])).max()))
                    hits += 1
            assert np.all(hit[h - h % 32:] == 0)
    assert hits > 0 and worst < TIGHT, (name, worst)
    print("%s: %d primary hits, largest |point - second reading's| %.3e" % (name, hits, worst))


@pytest.mark.parametrize("name", RAY_SCENES)
def test_intersect_rays_against_the_second_reading(pkg, ctx, expected, name):
    """rm_intersect_rays on 4,097 rays with origins of their own.  include/rusty_marcher_amd.h documents rm_hit.shape as
    shapes.rs:140's shape_hit NOT wrapped to u8; the second reading returns the reference's wrapped u8.  So the device's
    index must equal the second reading's modulo 256 -- and, in the scene of 300 spheres, for the rays aimed at sphere k the
    device must say k itself."""
    upload(pkg, ctx, expected["desc"][name])
    o, d = expected["rays"][name]
    got = ctx.intersect(o, d)
    first = expected["first"][name]
    assert len(first) == N_RAYS == got.shape[0]
    hit = np.array([f is not None for f in first])
    assert np.array_equal(got["hit"].astype(bool), hit), np.flatnonzero(got["hit"].astype(bool) != hit)[:8]
    assert 0 < hit.sum() < N_RAYS
    index = np.array([f[0] for f in first if f is not None])
    assert np.array_equal(got["shape"][hit] % 256, index)
    n_shapes = len(expected["desc"][name]["shapes"]) if not expected["desc"][name].get("default") else 6
    assert np.all(got["shape"][hit] < n_shapes)
    if n_shapes <= 256:
        assert np.array_equal(got["shape"][hit], index)
    point = np.array([f[1] for f in first if f is not None])
    normal = np.array([f[2] for f in first if f is not None])
    worst = float(np.abs(got["point"][hit] - point).max())
    assert worst < TIGHT and float(np.abs(got["normal"][hit] - normal).max()) < TIGHT, (name, worst)
    assert np.all(got["point"][~hit] == 0.) and np.all(got["shape"][~hit] == 0)     # every field 0 on a miss
    if name == "wrap":
        assert np.array_equal(got["shape"][-300:], np.arange(300)) and np.all(got["hit"][-300:] == 1)
        assert int((got["shape"][hit] >= 256).sum()) >= 44
    print("%s: %d of %d rays hit, largest |point - second reading's| %.3e" % (name, hit.sum(), N_RAYS, worst))


@pytest.mark.parametrize("name", RADIANCE_SCENES)
def test_radiance_rays_against_the_second_reading(pkg, ctx, expected, name):
    upload(pkg, ctx, expected["desc"][name])
    o, d = expected["rays"][name]
    worst = 0.
    for k, depth in enumerate(RAY_DEPTHS):
        got = ctx.radiance(o, d, max_depth=depth)
        mine = np.array([rgb[k] for rgb in expected["rgb"][name]])
        assert got.shape == mine.shape == (N_RAYS, 3)
        dev = float(np.abs(got - mine).max())
        assert dev < TIGHT, (name, depth, dev, int(np.abs(got - mine).max(axis=1).argmax()))
        assert np.any(mine > 0.)
        worst = max(worst, dev)
    print("%s: largest |radiance - second reading's cast_ray| %.3e" % (name, worst))


@pytest.mark.parametrize("name", list(TS.MOVES))
def test_moved_scene_against_the_second_reading(pkg, ctx, expected, name):
    """rm_scene_offset_shape (through the shapes' own offset()) on Cornell meshes and on the demo's polygons, against the
    second reading's render of its own offset() scene."""
    desc, eye, second = expected["moved"][name]
    upload(pkg, ctx, desc, eye)
    gpu = np.zeros((32, 32, 3), dtype=np.float64)
    ctx.render(params(pkg, 32, 32, 3), gpu)
    dev = hold_frame(gpu, second, (name, "moved"))
    upload(pkg, ctx, expected["desc"][name], eye)
    still = np.zeros((32, 32, 3), dtype=np.float64)
    ctx.render(params(pkg, 32, 32, 3), still)
    assert not np.array_equal(still, gpu)                 # the move shows
    print("%s moved: largest |GPU - second reading| %.3e" % (name, dev))
