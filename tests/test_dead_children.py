"""CPU checks of the planar primitives' empty half-spaces (csrc/rm_image.cpp rm_build_empty_sides, at upload): a child ray that
leaves a glass-like polygon or triangle into a side of its plane that holds nothing is not walked by the plain-walk
kernels.  The flags of the demo scene are pinned; anything in doubt clears them; and for 200 seeded scenes every ray
that starts 1e-4 off a flagged side and runs into it misses everything by the oracle's own closest-hit search.  The
launch plan's enable bit is checked through an internal export.  The exports used here (rmi_empty_sides,
rmi_plan_dead_children) are not part of the ABI and need no device."""
import ctypes as C

import numpy as np
import pytest

import workloads
from test_shadow_masks import _unit, build_pair, random_shapes

POS, NEG = 1, 2                       # RM_EMPTY_SIDE_POS / RM_EMPTY_SIDE_NEG: the side the normal points to / the other one
GLASS = dict(workloads.FLOOR_MATERIAL)
FLOOR = list(workloads.FLOOR_QUAD)    # its normal points up (+y, a little +z)
BELOW_ALL = [(100., -40., -120.), (-100., -40., -120.), (-100., -45., 40.), (100., -45., 40.)]   # normal up; under every random shape
N_RAYS = 200


def empty_sides(pkg, scene):
    """-> (sides per pid, glass word per pid, shape index per pid, camera limit) of the image `scene` uploads to."""
    f = pkg.lib().rmi_empty_sides
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_uint32,
                  C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
    d = scene.flatten().desc()
    sides, glass, shape_of = (C.c_uint8 * 64)(), (C.c_double * 64)(), (C.c_uint32 * 64)()
    dims, limit = (C.c_uint32 * 2)(), C.c_double(-1.)
    assert f(C.addressof(d), sides, glass, shape_of, 64, dims, C.byref(limit)) == 0
    n = dims[0]
    if not dims[1]:
        return None, None, None, limit.value
    return list(sides[:n]), list(glass[:n]), list(shape_of[:n]), limit.value


def plan_bit(pkg, camera, limit, n_spheres=4, n_polygons=2, n_triangles=0, total_words=200):
    """-> (KernelArgs::dead_children, the kernel is a plain-walk one) of a launch planned with the environment's knobs."""
    f = pkg.lib().rmi_plan_dead_children
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    cam = (C.c_double * 3)(*camera)
    out = (C.c_uint32 * 2)()
    assert f(C.addressof(cam), limit, n_spheres, n_polygons, n_triangles, total_words, out) == 0
    return out[0], out[1]


def quad_scene(pkg, extra=(), floor=FLOOR, floor_material=GLASS):
    """The glass floor quad first (pid order: spheres, then polygons in list order), then `extra` shapes."""
    s = pkg.Scene.new()
    s.shapes.append(pkg.polygon.ConvexPolygon.create([pkg.Vec3f(*p) for p in floor], pkg.Reflectance(**floor_material)))
    for sh in extra:
        if sh[0] == "sphere":
            s.shapes.append(pkg.sphere.create(pkg.Vec3f(*sh[1]), sh[2], pkg.Reflectance()))
        else:
            s.shapes.append(pkg.polygon.ConvexPolygon.create([pkg.Vec3f(*p) for p in sh[1]], pkg.Reflectance(**GLASS)))
    s.lights.append(pkg.create_light(pkg.Vec3f(0., 0., 0.), pkg.Vec3f(1., 1., 1.), 1.))
    return s


def floor_sides(pkg, extra):
    scene = quad_scene(pkg, extra)
    sides, glass, shape_of, _ = empty_sides(pkg, scene)
    pid = shape_of.index(0)
    return sides[pid], glass[pid]


def plane_of(verts):
    """Normal and plane point as the scene builder forms them (polygon.rs:16-42, triangle.rs:33-47)."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    return _unit(np.cross(v[1] - v[0], v[2] - v[1])), v.mean(axis=0)


def test_demo_scene_flags_the_floors_far_side_only(pkg):
    sides, glass, shape_of, limit = empty_sides(pkg, pkg.Scene.create_default())
    # pids: the four spheres (blue, green, red, white), the triangle, the floor
    assert shape_of == [0, 1, 2, 3, 4, 5]
    # the floor's normal points up, towards everything else: the side below it holds nothing; the blue sphere
    # straddles the triangle's plane
    assert sides == [0, 0, 0, 0, 0, NEG]
    # glass word: 0 not glass-like, else 1 + 2 x empty(+) + 4 x empty(-); blue and the floor are glass-like
    assert glass == [1., 0., 0., 0., 0., 5.]
    assert 0. < limit <= 1e9


def test_flag_set_when_everything_is_clear_of_the_plane(pkg):
    assert floor_sides(pkg, [("sphere", (0., 0., -10.), 1.)]) == (NEG, 5.)
    assert floor_sides(pkg, []) == (POS | NEG, 7.)
    assert floor_sides(pkg, [("sphere", (0., -30., -10.), 1.)]) == (POS, 3.)


def test_flags_clear_for_a_sphere_through_the_plane(pkg):
    n, pp = plane_of(FLOOR)
    assert floor_sides(pkg, [("sphere", tuple(pp), 1.)]) == (0, 1.)
    assert floor_sides(pkg, [("sphere", tuple(pp + 0.9 * n), 1.)]) == (0, 1.)


def test_flag_clear_within_the_margin(pkg):
    n, pp = plane_of(FLOOR)
    # a sphere wholly above the plane, 5e-4 clear of it: within 1e-4 + shadow_rho (1e-3): the far side is not flagged
    assert floor_sides(pkg, [("sphere", tuple(pp + (1. + 5e-4) * n), 1.)]) == (0, 1.)
    assert floor_sides(pkg, [("sphere", tuple(pp + (1. + 5e-2) * n), 1.)]) == (NEG, 5.)
    # ... and a polygon by its vertices
    lifted = [tuple(np.asarray(p) + 5e-4 * n) for p in FLOOR]
    assert floor_sides(pkg, [("polygon", lifted)])[0] == 0
    lifted = [tuple(np.asarray(p) + 5e-2 * n) for p in FLOOR]
    assert floor_sides(pkg, [("polygon", lifted)])[0] == NEG


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_flags_clear_for_a_non_finite_vertex(pkg, bad):
    tri = [(0., 5., -10.), (3., 5., -10.), (0., 8., -12.)]
    assert floor_sides(pkg, [("polygon", tri)])[0] == NEG
    tri[1] = (3., bad, -10.)
    assert floor_sides(pkg, [("polygon", tri)])[0] == 0
    sides, _, _, _ = empty_sides(pkg, quad_scene(pkg, floor=[FLOOR[0], (bad, -3., -50.), FLOOR[2], FLOOR[3]]))
    assert sides == [0]


def test_flags_clear_for_coordinates_of_1e7(pkg):
    assert floor_sides(pkg, [("sphere", (0., 1e7, 0.), 1.)]) == (0, 1.)
    far = [tuple(1e7 * c for c in p) for p in FLOOR]
    sides, _, _, _ = empty_sides(pkg, quad_scene(pkg, floor=far))
    assert sides == [0]


def test_second_parallel_quad_on_that_side(pkg):
    lower = [(x, y - 2., z) for x, y, z in FLOOR]
    scene = quad_scene(pkg, [("sphere", (0., 0., -10.), 1.), ("polygon", lower)])
    sides, glass, shape_of, _ = empty_sides(pkg, scene)
    upper_pid, lower_pid = shape_of.index(0), shape_of.index(2)
    assert sides[upper_pid] == 0 and glass[upper_pid] == 1.
    assert sides[lower_pid] == NEG and glass[lower_pid] == 5.


def test_no_flags_beyond_64_primitives(pkg):
    s = quad_scene(pkg, [("sphere", (float(i % 13), float(i // 13), -20.), 0.3) for i in range(64)])
    sides, _, _, limit = empty_sides(pkg, s)
    assert sides is None and limit == 0.


def test_non_glass_primitive_keeps_its_word(pkg):
    plain = dict(GLASS, is_glass_like=False)
    sides, glass, _, limit = empty_sides(pkg, quad_scene(pkg, floor_material=plain))
    assert sides == [POS | NEG] and glass == [0.] and limit == 0.


# ------------------------------------------------------------------ random scenes
def _verts_of(shape):
    return np.asarray(shape[1], dtype=np.float64).reshape(-1, 3)


def fuzz_shapes(seed):
    """random_shapes' scene, an outlying triangle or quad of random orientation well to one side of it (its plane often misses
    everything else, so the fuzz meets flags on tilted planes of both signs), and the quad below everything."""
    shapes, lights = random_shapes(seed)
    rng = np.random.default_rng(20_000 + seed)
    ctr = _unit(rng.normal(size=3)) * rng.uniform(150., 200.)
    ctr[1] = abs(ctr[1]) * 0.15                                        # (above the quad below everything, below 1e6)
    nrm = _unit(_unit(ctr) * rng.choice([-1., 1.]) + 0.5 * rng.normal(size=3))   # (tilted, mostly facing the scene or away from it)
    e1 = _unit(np.cross(nrm, rng.normal(size=3)))
    e2 = np.cross(nrm, e1)
    ang = np.sort(rng.uniform(0., 2. * np.pi, int(rng.integers(3, 5))))
    rad = rng.uniform(1., 5.)
    outlier = [tuple(float(x) for x in ctr + rad * (np.cos(a) * e1 + np.sin(a) * e2)) for a in ang]
    return shapes + [("polygon", outlier), ("polygon", BELOW_ALL)], lights


def test_random_scenes_carry_flags_beyond_the_constructed_quad(pkg, O):
    flagged = 0
    for seed in range(200):
        shapes, lights = fuzz_shapes(seed)
        sides, _, _, _ = empty_sides(pkg, build_pair(pkg, O, shapes, lights)[0])
        flagged += sum(bin(b).count("1") for b in sides)
    print("flagged (P, side) pairs over 200 scenes: %d" % flagged)
    assert flagged > 300                                                 # (200 are the quad's; at least half of the outliers')


@pytest.mark.parametrize("seed", range(200))
def test_random_scenes_rays_into_flagged_sides_miss_everything(pkg, O, seed):
    shapes, lights = fuzz_shapes(seed)
    scene, oscene = build_pair(pkg, O, shapes, lights)
    sides, _, shape_of, _ = empty_sides(pkg, scene)
    assert sides is not None
    below = shape_of.index(len(shapes) - 1)
    assert sides[below] & NEG, "seed %d: the quad below everything has no flag" % seed
    L = O.lib()
    c = oscene.c
    rng = np.random.default_rng(10_000 + seed)
    for p, bits in enumerate(sides):
        for bit, sign in ((POS, 1.), (NEG, -1.)):
            if not bits & bit:
                continue
            verts = _verts_of(shapes[shape_of[p]])
            assert len(verts) >= 3
            n, _ = plane_of(verts)
            for k in range(N_RAYS):
                w = rng.dirichlet(np.ones(len(verts)) * (0.3 if k % 3 == 0 else 1.))    # (near edges and corners too)
                point = w @ verts
                orig = point + sign * 1e-4 * n
                if k % 2:                                                               # grazing: 1e-1 .. 1e-12 off the plane
                    t = _unit(np.cross(n, rng.normal(size=3)))
                    d = _unit(t + sign * n * 10. ** rng.uniform(-12., -1.))
                else:
                    d = _unit(rng.normal(size=3))
                    d = d if sign * (d @ n) > 0. else -d
                assert sign * (d @ n) > 0.
                its, which = O.Intersection(), C.c_uint8(0)
                hit = L.orc_find_closest_intersect(O.v3(orig), O.v3(d), c.shapes, c.n_shapes, C.byref(its), C.byref(which))
                assert not hit, ("seed %d: a ray from pid %d (shape %d), side %+d, origin %s direction %s hits shape %d"
                                 % (seed, p, shape_of[p], int(sign), orig, d, which.value))


# ------------------------------------------------------------------ the launch plan's bit
def test_plan_enables_near_the_scene_only(pkg, monkeypatch):
    for k in ("RM_DEAD_CHILDREN", "RM_SHADOW_MASKS"):
        monkeypatch.delenv(k, raising=False)
    _, _, _, limit = empty_sides(pkg, pkg.Scene.create_default())
    assert plan_bit(pkg, (0., 0., 0.), limit) == (1, 1)
    assert plan_bit(pkg, (0., -20., -20.), limit) == (1, 1)
    assert plan_bit(pkg, (0.3 * limit, 0.3 * limit, -0.3 * limit), limit) == (1, 1)
    assert plan_bit(pkg, (0.4 * limit, 0.4 * limit, -0.3 * limit), limit) == (0, 1)
    assert plan_bit(pkg, (0., 0., 2e9), limit) == (0, 1)
    assert plan_bit(pkg, (0., 0., float("nan")), limit) == (0, 1)
    assert plan_bit(pkg, (0., 0., 0.), 0.) == (0, 1)                      # an image without flags


def test_plan_knob_is_independent_of_the_masks_knob(pkg, monkeypatch):
    monkeypatch.setenv("RM_SHADOW_MASKS", "0")
    monkeypatch.delenv("RM_DEAD_CHILDREN", raising=False)
    assert plan_bit(pkg, (0., 0., 0.), 1e8) == (1, 1)
    monkeypatch.setenv("RM_DEAD_CHILDREN", "0")
    assert plan_bit(pkg, (0., 0., 0.), 1e8) == (0, 1)
    monkeypatch.delenv("RM_SHADOW_MASKS")
    assert plan_bit(pkg, (0., 0., 0.), 1e8) == (0, 1)
    monkeypatch.setenv("RM_DEAD_CHILDREN", "1")
    assert plan_bit(pkg, (0., 0., 0.), 1e8) == (1, 1)


def test_plan_bit_is_off_for_other_kernels(pkg, monkeypatch):
    monkeypatch.delenv("RM_DEAD_CHILDREN", raising=False)
    # a dozen primitives and more take the kernels with the bundle cull; scenes too long for an LDS copy too
    assert plan_bit(pkg, (0., 0., 0.), 1e8, n_spheres=20, n_polygons=1) == (0, 0)
    assert plan_bit(pkg, (0., 0., 0.), 1e8, total_words=4096) == (0, 0)
