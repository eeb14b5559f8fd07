"""CPU checks of the shadow rays' occluder masks (csrc/rm_image.cpp rm_build_shadow_masks, at upload, for the
plain-walk kernels): for random scenes, random hit points on every primitive and the reference's
shadow-ray construction (renderer.rs:163-174), every primitive the oracle's own intersection test
reports hit must have its bit in occ[P][light].  The demo scene's table is pinned, so that a looser
builder shows."""
import ctypes as C

import numpy as np
import pytest

import workloads

N_PER_PRIM = 48


def masks(pkg, scene):
    """-> (occ [pids][lights] as Python ints, shape index of each pid) of the image `scene` uploads to."""
    L = pkg.lib()
    f = L.rmi_shadow_masks
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]
    d = scene.flatten().desc()
    occ = (C.c_uint64 * 4096)()
    shape_of = (C.c_uint32 * 64)()
    dims = (C.c_uint32 * 3)()
    assert f(C.addressof(d), occ, shape_of, 4096, dims) == 0
    n, nl, has = dims[0], dims[1], dims[2]
    if not has:
        return None, None
    return [[occ[p * nl + l] for l in range(nl)] for p in range(n)], [shape_of[p] for p in range(n)]


def test_demo_table_is_pinned(pkg):
    occ, shape_of = masks(pkg, pkg.Scene.create_default())
    # pids: the four spheres (blue, green, red, white), the triangle, the floor; lights (0,0,0), (20,20,20)
    assert shape_of == [0, 1, 2, 3, 4, 5]
    assert occ == [[0b000001, 0b000001],
                   [0b010011, 0b010010],
                   [0b001101, 0b000100],
                   [0b001100, 0b001000],
                   [0b110010, 0b110010],
                   [0b111111, 0b111111]]


def test_no_table_beyond_64_primitives(pkg):
    s = pkg.Scene.new()
    for i in range(65):
        s.shapes.append(pkg.sphere.create(pkg.Vec3f(float(i % 13), float(i // 13), -20.), 0.3, pkg.Reflectance()))
    s.lights.append(pkg.create_light(pkg.Vec3f(0., 0., 0.), pkg.Vec3f(1., 1., 1.), 1.))
    assert masks(pkg, s) == (None, None)


# ------------------------------------------------------------------ random scenes
def _unit(v):
    return v / np.linalg.norm(v)


def random_shapes(seed, n=None):
    """-> (shapes, lights) in workloads' / test_gpu_query's form: up to 11 primitives -- spheres (some touching each
    other or the floor), triangles, quads, a floor, a one-triangle mesh, a polygon that can never be hit -- and one to
    three lights, some inside a sphere, on its surface or on a polygon's vertex."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 12)) if n is None else n
    shapes, spheres = [], []
    floor_y = float(rng.uniform(-6., -2.))
    for _ in range(n):
        kind = rng.choice(["sphere", "sphere", "tri", "quad", "floor", "mesh", "never", "touch"], p=[.3, .1, .15, .15, .08, .08, .06, .08])
        if kind in ("sphere", "touch") or (kind == "touch" and not spheres):
            r = float(rng.uniform(0.3, 3.))
            c = rng.uniform((-10., -5., -30.), (10., 5., -5.))
            if kind == "touch" and spheres:
                c0, r0 = spheres[int(rng.integers(len(spheres)))]
                c = np.asarray(c0) + _unit(rng.normal(size=3)) * (r0 + r)
            elif rng.uniform() < 0.3:
                c[1] = floor_y + r                                   # resting on the floor
            spheres.append((tuple(float(x) for x in c), r))
            shapes.append(("sphere", tuple(float(x) for x in c), r))
        elif kind in ("tri", "quad", "mesh"):
            ctr = rng.uniform((-10., -5., -30.), (10., 5., -5.))
            nrm = _unit(rng.normal(size=3))
            e1 = _unit(np.cross(nrm, rng.normal(size=3)))
            e2 = np.cross(nrm, e1)
            k = 3 if kind != "quad" else 4
            ang = np.sort(rng.uniform(0., 2. * np.pi, k))
            rad = rng.uniform(0.5, 5.)
            verts = [tuple(float(x) for x in ctr + rad * (np.cos(a) * e1 + np.sin(a) * e2)) for a in ang]
            if kind == "mesh":
                shapes.append(("mesh", np.array([sum(verts, ())], dtype=np.float64)))
            else:
                shapes.append(("polygon", verts))
        elif kind == "floor":
            x0, x1 = sorted(rng.uniform(-60., 60., 2))
            z0, z1 = sorted(rng.uniform(-80., -1., 2))
            shapes.append(("polygon", [(x0, floor_y, z1), (x1, floor_y, z1), (x1, floor_y, z0), (x0, floor_y, z0)]))
        else:                                                        # every vertex at one x: never hit (polygon.rs:54-56)
            x = float(rng.uniform(-10., 10.))
            shapes.append(("polygon", [(x, -2., -8.), (x, -2., -16.), (x, 3., -16.), (x, 3., -8.)]))
    lights = []
    for _ in range(int(rng.integers(1, 4))):
        u = rng.uniform()
        if u < 0.15 and spheres:
            pos = spheres[int(rng.integers(len(spheres)))][0]                                          # at a centre
        elif u < 0.3 and spheres:
            c, r = spheres[int(rng.integers(len(spheres)))]
            pos = tuple(float(x) for x in np.asarray(c) + _unit(rng.normal(size=3)) * r)                # on a surface
        elif u < 0.4 and any(s[0] == "polygon" for s in shapes):
            pos = [s for s in shapes if s[0] == "polygon"][0][1][0]                                     # on a vertex
        else:
            pos = tuple(float(x) for x in rng.uniform((-30., -10., -40.), (30., 30., 25.)))
        lights.append((pos, (1., 1., 1.), 1.))
    return shapes, lights


def build_pair(pkg, O, shapes, lights):
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


def _shape_ptr(O, oscene, i):
    c = oscene.c
    return C.cast(C.addressof(c.shapes.contents) + i * C.sizeof(O.Shape), C.POINTER(O.Shape))


def hit_points(O, rng, oscene, shape, i, n):
    """Points (and normals) where the oracle's own test says rays hit shape i: rays aimed at random points of it
    from outside, from inside (spheres), and at a slant."""
    L = O.lib()
    sp = _shape_ptr(O, oscene, i)
    out = []
    for k in range(n):
        if shape[0] == "sphere":
            c, r = np.asarray(shape[1]), shape[2]
            u = _unit(rng.normal(size=3))
            target = c + u * r
            if k % 4 == 3:
                orig = c + _unit(rng.normal(size=3)) * r * rng.uniform(0., 0.9)          # from inside (refracted rays)
            else:
                orig = target + _unit(u + rng.normal(size=3) * (0.2 if k % 4 else 3.)) * rng.uniform(0.1, 40.)
        else:
            verts = np.asarray(shape[1], dtype=np.float64).reshape(-1, 3)
            w = rng.dirichlet(np.ones(len(verts)) * (0.3 if k % 3 == 0 else 1.))   # (near edges and corners too)
            target = w @ verts
            nrm = _unit(np.cross(verts[1] - verts[0], verts[2] - verts[0]))
            side = 1. if rng.uniform() < 0.5 else -1.
            orig = target + side * _unit(nrm + rng.normal(size=3) * (0.3 if k % 3 else 5.)) * rng.uniform(0.1, 40.)
        o = O.v3(orig)
        d = L.orc_normalized(L.orc_sub(O.v3(target), o))
        its = O.Intersection()
        if L.orc_shape_intersect(sp, o, d, C.byref(its)):
            out.append((its.point, its.normal))
    return out


def check_scene(pkg, O, shapes, lights, seed, n_per_prim=N_PER_PRIM):
    scene, oscene = build_pair(pkg, O, shapes, lights)
    occ, shape_of = masks(pkg, scene)
    assert occ is not None
    L = O.lib()
    rng = np.random.default_rng(seed)
    n = len(occ)
    ptrs = [_shape_ptr(O, oscene, shape_of[q]) for q in range(n)]
    tested = hits = 0
    for p in range(n):
        assert all((occ[p][l] >> p) & 1 for l in range(len(lights))), "pid %d: own bit clear" % p
        for point, normal in hit_points(O, rng, oscene, shapes[shape_of[p]], shape_of[p], n_per_prim):
            for l, (pos, _, _) in enumerate(lights):
                # renderer.rs:163-174
                light_dir = L.orc_normalized(L.orc_sub(O.v3(pos), point))
                off = L.orc_scaled(normal, 1e-3)
                orig = L.orc_sub(point, off) if L.orc_dot(light_dir, normal) < 0. else L.orc_add(point, off)
                for q in range(n):
                    its = O.Intersection()
                    tested += 1
                    if L.orc_shape_intersect(ptrs[q], orig, light_dir, C.byref(its)):
                        hits += 1
                        assert (occ[p][l] >> q) & 1, ("seed %d: a shadow ray from pid %d (shape %d) towards light %d %s hits pid %d, "
                                                      "which its mask 0x%x leaves out" % (seed, p, shape_of[p], l, pos, q, occ[p][l]))
    return tested, hits


@pytest.mark.parametrize("seed", range(40))
def test_random_scenes_masks_hold_every_occluder(pkg, O, seed):
    shapes, lights = random_shapes(seed)
    check_scene(pkg, O, shapes, lights, seed)


def test_demo_scene_masks_hold_every_occluder(pkg, O):
    scene, oscene = workloads.product_scene(pkg, "demo"), workloads.oracle_scene(O, "demo")
    occ, shape_of = masks(pkg, scene)
    d = scene.flatten().desc()
    shapes = []
    for i in range(d.n_shapes):
        ref = d.shapes[i]
        if ref.kind == pkg._lib.RM_SHAPE_SPHERE:
            s = d.spheres[ref.first]
            shapes.append(("sphere", (s.center.x, s.center.y, s.center.z), s.radius_square ** 0.5))
        elif ref.kind == pkg._lib.RM_SHAPE_POLYGON:
            p = d.polygons[ref.first]
            shapes.append(("polygon", [(d.polygon_vertices[p.first_vertex + k].x, d.polygon_vertices[p.first_vertex + k].y,
                                        d.polygon_vertices[p.first_vertex + k].z) for k in range(p.n_vertices)]))
        else:
            v = d.triangles[ref.first].vertices
            shapes.append(("mesh", np.array([[v[0].x, v[0].y, v[0].z, v[1].x, v[1].y, v[1].z, v[2].x, v[2].y, v[2].z]])))
    lights = [((d.lights[i].position.x, d.lights[i].position.y, d.lights[i].position.z), (1., 1., 1.), 1.) for i in range(d.n_lights)]
    tested, hits = check_scene(pkg, O, shapes, lights, 7, n_per_prim=200)
    assert hits > 0 and tested > hits


def test_masks_are_tight_somewhere(pkg, O):
    """The random scenes do exercise the masks: many rows leave primitives out."""
    cleared = total = 0
    for seed in range(40):
        shapes, lights = random_shapes(seed)
        occ, _ = masks(pkg, build_pair(pkg, O, shapes, lights)[0])
        n = len(occ)
        for row in occ:
            for m in row:
                total += n
                cleared += n - bin(m).count("1")
    assert cleared > total // 4
