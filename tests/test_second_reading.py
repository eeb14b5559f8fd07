"""The CPU oracle held to a second, independent reading of the reference (tests/second_reading.py).  No GPU.

a. the second reading on its own: the reference's unit tests, and engine/out.ppm byte for byte;
b. function by function, both readings on the same inputs: every decision and every double equal AS BITS (== on each
   double, NaN equal to NaN in the same place) -- none of these functions calls pow, sqrt and / round correctly in both,
   so a difference is a different reading of the Rust, not rounding.  Every kind of input the comparison is meant to reach
   is COUNTED, by the second reading alone, and the count asserted non-zero;
c. whole frames, 32x32 and 64x39 (7 rows of remainder that must stay zero), depth caps 1-6, three cameras, of every kind of
   scene the suite renders: first-hit decision, shape index and glass flag of every pixel equal, every channel within
   radiance_reference.TIGHT (pow is the one operation two libraries may round differently);
d. moved shapes: polygon.rs:44-49 and triangle.rs:19-24 move the point of the plane and the vertices, never the normal.

Where the readings disagree, the Rust decides ("The trust chain").
"""
import ctypes as C
import hashlib
import math
import random
import time

import numpy as np
import pytest

import radiance_reference as RR
import second_reading as S
import second_reading_scenes as SC
import soft_reference as SR
import test_gpu_parity as TP
import workloads

TIGHT = RR.TIGHT
SIZES = [(32, 32), (64, 39)]
DEPTHS = [1, 2, 3, 4, 5, 6]
FUZZ_SEEDS = range(12)


# ---------------------------------------------------------------- comparing as bits
def same(a, b):
    return a == b or (a != a and b != b)


def same3(mine, theirs):
    return same(mine[0], theirs.x) and same(mine[1], theirs.y) and same(mine[2], theirs.z)


def same_reflectance(mine, theirs):
    return (same(mine.diffusion, theirs.diffusion) and same3(mine.diffuse_color, theirs.diffuse_color)
            and same(mine.specular, theirs.specular) and same(mine.specular_exponent, theirs.specular_exponent)
            and bool(mine.is_glass_like) == bool(theirs.is_glass_like) and same(mine.reflection, theirs.reflection)
            and same(mine.refractive_index, theirs.refractive_index))


def check_intersection(mine, flag, theirs, what=""):
    assert (mine is not None) == bool(flag), "hit/miss differs: %s" % (what,)
    if mine is not None:
        assert same3(mine.point, theirs.point), ("point", what, mine.point, theirs.point.tup())
        assert same3(mine.normal, theirs.normal), ("normal", what, mine.normal, theirs.normal.tup())
        assert same_reflectance(mine.reflectance, theirs.reflectance), ("reflectance", what)


def unit(rng):
    while True:
        v = (rng.uniform(-1., 1.), rng.uniform(-1., 1.), rng.uniform(-1., 1.))
        if 0.01 < S.squared_norm(v) <= 1.:
            return S.normalized(v)


def material(rng, glass=None):
    glass = (rng.random() < 0.4) if glass is None else glass
    return dict(diffusion=rng.uniform(0.1, 1.), diffuse_color=(rng.random(), rng.random(), rng.random()),
                specular=rng.uniform(0.2, 1.), specular_exponent=rng.choice([1., 8., 30., 100., 12.5]), is_glass_like=glass,
                reflection=rng.uniform(0.1, 0.9), refractive_index=rng.uniform(1.1, 1.8) if glass else 1.)


def ccw_polygon(rng, n, tilt_range=2.):
    """n vertices counter-clockwise in xy, on a plane tilted by up to `tilt_range` in z per unit of x and of y"""
    ang = sorted(rng.uniform(0., 2. * math.pi) for _ in range(n))
    cx, cy, cz, rad = rng.uniform(-8., 8.), rng.uniform(-6., 6.), rng.uniform(-30., -8.), rng.uniform(2., 7.)
    t0, t1 = rng.uniform(-tilt_range, tilt_range), rng.uniform(-tilt_range, tilt_range)
    return [(cx + rad * math.cos(a), cy + rad * math.sin(a), cz + t0 * rad * math.cos(a) + t1 * rad * math.sin(a)) for a in ang]


def point_in(rng, verts):
    w = [rng.random() + 0.05 for _ in verts]
    s = sum(w)
    return tuple(sum(w[k] * verts[k][c] for k in range(len(verts))) / s for c in range(3))


class Pair:
    """One list of shapes, in both readings."""

    def __init__(self, O):
        self.O, self.L, self.so, self.mine = O, O.lib(), O.OracleScene(), []

    def sphere(self, c, r, m):
        self.mine.append(S.Sphere(c, r, SC._second_material(m)))
        self.so.add_sphere(c, r, self.O.reflectance(**m))
        return len(self.mine) - 1

    def polygon(self, verts, m):
        self.mine.append(S.ConvexPolygon(verts, SC._second_material(m)))
        self.so.add_polygon(verts, self.O.reflectance(**m))
        return len(self.mine) - 1

    def mesh(self, tris, off=(0., 0., 0.)):
        positions = [x for t in tris for v in t for x in v]
        obj = S.Obj(positions, list(range(len(positions) // 3)), widen=float)
        obj.offset(off)
        self.mine.append(obj)
        self.so.add_obj(np.array(tris, dtype=np.float64).reshape(-1, 9), off)
        return len(self.mine) - 1

    def theirs(self, i):
        return self.so.ptr.contents.shapes[i]

    def intersect(self, i, o, d, what=""):
        """both readings' Shape::intersect of shape i; asserts they agree, returns the second reading's"""
        mine = self.mine[i].intersect(o, d)
        out = self.O.Intersection()
        flag = self.L.orc_shape_intersect(C.byref(self.theirs(i)), self.O.v3(o), self.O.v3(d), C.byref(out))
        check_intersection(mine, flag, out, what)
        return mine

    def closest(self, o, d, what=""):
        """both readings' find_closest_intersect and intersect_shape_set over the whole list"""
        mine = S.find_closest_intersect(o, d, self.mine)
        out, index = self.O.Intersection(), C.c_uint8(0)
        n = len(self.mine)
        flag = self.L.orc_find_closest_intersect(self.O.v3(o), self.O.v3(d), self.so.ptr.contents.shapes, n, C.byref(out), C.byref(index))
        check_intersection(None if mine is None else mine[0], flag, out, what)
        if mine is not None:
            assert mine[1] == index.value, ("shape index", what, mine[1], index.value)
        anything = S.intersect_shape_set(o, d, self.mine)
        assert anything == bool(self.L.orc_intersect_shape_set(self.O.v3(o), self.O.v3(d), self.so.ptr.contents.shapes, n))
        assert anything == (mine is not None)
        return mine


@pytest.fixture(scope="module")
def Y(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("second_reading"))


# ================================================================ a. the second reading on its own
def test_second_reading_imports_nothing_of_the_project():
    import ast
    names = set()
    for node in ast.walk(ast.parse(open(S.__file__).read())):
        if isinstance(node, ast.Import):
            names.update(a.name.split(".")[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or ".").split(".")[0])
    assert names <= {"math", "os", "struct", "collections", "multiprocessing"}, names
    assert "written from the Rust source alone" in " ".join(S.__doc__.split())


def test_kat_geometry():                                  # geometry.rs:188-408
    assert S.ONES == (1., 1., 1.)
    assert S.scaled(S.ONES, 1.36) == (1.36, 1.36, 1.36)
    assert S.scaled((1., 2., 3.), 1.36) == (1.36, 2.72, 4.08)
    assert S.dot((0., 1., 0.), (1., 0., 0.)) == 0.
    assert S.dot((0., 1., 0.), (0., 1., 0.)) == 1.
    assert S.dot((0., 1., 0.), (0., -1., 0.)) == -1.
    assert S.dot((1., 1., 0.), (1., -1., 0.)) == 0.
    a = (42., 1., 0.)
    assert S.squared_norm(a) == 42. * 42. + 1.
    assert S.squared_norm(S.normalized(a)) == 1.
    assert S.normalized_l0(a)[0] == 1.
    assert S.squared_norm(S.cross(a, a)) == 0.
    assert S.squared_norm(S.cross(a, S.neg(a))) == 0.
    a, b = (1., 1., 0.), (1., -1., 0.)
    assert S.dot(S.cross(a, b), a) == 0.
    assert S.squared_norm(S.cross(a, b)) == S.squared_norm(a) * S.squared_norm(b)
    b = (1., 0., 0.)
    assert S.squared_norm(S.cross(a, b)) - S.squared_norm(a) * S.squared_norm(b) * math.sin(math.pi / 4.) ** 2. < 1e-4
    assert S.squared_norm((1., -2., 3.)) == 14.
    assert S.add((1., -2., 3.), (4., -2., 2.)) == (5., -4., 5.)
    assert S.sub((1., -2., 3.), (1., -2., 3.)) == S.ZERO


def test_kat_reflection():                                # optics.rs:96-132
    incident = (0.5, -0.5, 0.)
    isec = S.Intersection(S.ZERO, (0., 1., 0.), S.default_reflectance())
    assert S.reflect(incident, isec.normal) == (0.5, 0.5, 0.)
    got = S.reflect_ray(incident, isec, 1.5)
    assert got is not None and got[1] == (0.5, 0.5, 0.)


def test_kat_triangle_intersect():                        # triangle.rs:88-138
    v = [(-1., 3., 2.2), (-3., 0.2, 2.1), (0., 1., 2.)]
    tris = [S.Triangle([v[0], v[1], v[2]]), S.Triangle([v[1], v[2], v[0]]), S.Triangle([v[2], v[0], v[1]])]
    orig, d = (-1., 2., 5.3), S.normalized((0.1, -0.2, -3.))
    hits = [t.intersect(orig, d) for t in tris]
    assert all(h is not None for h in hits)
    for h in hits[1:]:
        assert S.squared_norm(S.sub(hits[0].point, h.point)) < 1e-3
        assert S.squared_norm(S.sub(hits[0].normal, h.normal)) < 1e-3
    assert abs(S.squared_norm(tris[0].normal) - 1.) < 1e-3
    assert S.dot(tris[0].normal, d) < 0.


def test_kat_defaults_and_quantize():                     # shapes.rs:49-61, framebuffer.rs:80-82
    assert S.default_reflectance() == S.Reflectance(1., (1., 1., 1.), 1., 30., False, 0.95, 1.)
    assert [S.quantize(x) for x in (-1., 0., 0.5, 1., 2., math.nan, 0.999999)] == [0, 0, 127, 255, 255, 0, 254]


def test_directions_must_be_normalised():                 # sphere.rs:31, polygon.rs:62, triangle.rs:53
    shapes = [S.Sphere((0., 0., -5.), 1., S.default_reflectance()), S.Triangle([(0., 0., -5.), (1., 0., -5.), (0., 1., -5.)]),
              S.ConvexPolygon([(0., 0., -5.), (1., 0., -5.), (0., 1., -5.)], S.default_reflectance())]
    for shape in shapes:
        for d in [(0., 0., -1.01), (0., 0., -0.99), (math.nan, 0., -1.), (0., 0., 0.)]:
            with pytest.raises(S.NotNormalised):
                shape.intersect(S.ZERO, d)
        shape.intersect(S.ZERO, (0., 0., -1.00004))         # |1.00008 - 1| < 1e-4: admitted, as in the reference


def test_second_reading_reproduces_out_ppm_byte_for_byte(golden_ppm):
    """scene.rs create_default at 800x600 (main.rs:368: fov 1.5), depth cap 3, normalize (the maximum is the second
    reading's own, over its own full frame), to_vec and the header.  Wall time: DESIGN.md, "The trust chain"."""
    t0 = time.time()
    frame, _ = S.render_frame(S.Scene.create_default(), 800, 600, max_depth=3, workers=S.pool_size())
    assert all(px == S.ZERO for row in frame.buffer[576:] for px in row)              # 600 % 32 = 24 rows never written
    assert any(px != S.ZERO for px in frame.buffer[575])
    assert max(max(px) for row in frame.buffer for px in row) == 2.3621674603868565   # test_oracle_golden's spot value
    frame.normalize()
    data = frame.ppm_bytes()
    print("second reading, 800x600 depth 3 on %d processes: %.1f s" % (S.pool_size(), time.time() - t0))
    assert len(data) == len(golden_ppm)
    assert sum(a != b for a, b in zip(data, golden_ppm)) == 0
    assert hashlib.sha256(data).hexdigest() == "82d51afaaf4a644547728dde89478e484c245d2e3eb1e40da8b928ebd7584797"


def test_patches_in_processes_equal_patches_in_a_loop():
    scene = S.Scene.create_default()
    a, _ = S.render_frame(scene, 96, 71, max_depth=4, workers=1)
    b, _ = S.render_frame(scene, 96, 71, max_depth=4, workers=3)
    assert a.buffer == b.buffer
    with pytest.raises(ValueError):
        S.render_frame(scene, 100, 64)


# ================================================================ b. function by function, bit for bit
def test_spheres_bit_for_bit(O):
    rng = random.Random(20261201)
    pair = Pair(O)
    cases = []
    for k in range(600):
        c = (rng.uniform(-10., 10.), rng.uniform(-10., 10.), rng.uniform(-30., -5.))
        if k % 5 == 0:
            c = tuple(float(round(x)) for x in c)
        r = rng.uniform(0.5, 4.)
        i = pair.sphere(c, r, material(rng))
        mode = k % 4
        if mode == 0:                                     # from inside
            o = S.add(c, S.scaled(unit(rng), 0.95 * r * rng.random()))
            d = unit(rng)
        elif mode == 1:                                   # from outside, aimed into the sphere
            o = (rng.uniform(-15., 15.), rng.uniform(-15., 15.), rng.uniform(-5., 10.))
            d = S.normalized(S.sub(S.add(c, S.scaled(unit(rng), r * rng.random())), o))
        elif mode == 2:                                   # from outside, aimed away: the sphere is behind the origin
            o = (rng.uniform(-15., 15.), rng.uniform(-15., 15.), rng.uniform(-5., 10.))
            d = S.neg(S.normalized(S.sub(S.add(c, S.scaled(unit(rng), r * rng.random())), o)))
        else:
            o, d = (rng.uniform(-15., 15.), rng.uniform(-15., 15.), rng.uniform(-5., 10.)), unit(rng)
        cases.append((i, o, d))
    # tangent within an ulp: centre (0, 0, -10), radius r, the ray down -z from (r, 0, 0) or (0, r, 0) and its neighbours:
    # d2 == radius_square exactly at the middle one (a hit, `d2 > radius_square` is false), a miss one ulp further out
    for r in (2., 3., 0.5, 1.25):
        i = pair.sphere((0., 0., -10.), r, material(rng, glass=False))
        for x in (math.nextafter(r, 0.), r, math.nextafter(r, 10.)):
            cases += [(i, (x, 0., 0.), (0., 0., -1.)), (i, (0., x, 0.), (0., 0., -1.)), (i, (-x, 0., 3.), (0., 0., -1.))]
        # ... and close enough to the sphere that the ulp is not lost in the sum (x * x + z * z) - tca * tca
        j = pair.sphere((0., 0., 0.), r, material(rng, glass=False))
        for x in (math.nextafter(r, 0.), r, math.nextafter(r, 10.)):
            cases += [(j, (x, 0., 0.), (0., 0., -1.)), (j, (x, 0., 1.), (0., 0., -1.)), (j, (0., -x, 0.5), (0., 0., -1.))]
    found = dict(outside_hit=0, inside=0, behind=0, miss=0, tangent_hit=0, tangent_miss=0)
    for i, o, d in cases:
        mine = pair.intersect(i, o, d, ("sphere", i, o, d))
        sphere = pair.mine[i]
        line = S.sub(sphere.center, o)
        tca = S.dot(line, d)
        d2 = S.dot(line, line) - tca * tca
        inside = S.dot(line, line) < sphere.radius_square
        if abs(d2 - sphere.radius_square) <= 4. * math.ulp(sphere.radius_square):
            found["tangent_hit" if mine is not None else "tangent_miss"] += 1
        if inside:
            assert mine is not None
            found["inside"] += 1
        elif tca < 0.:
            assert mine is None
            found["behind"] += 1
        else:
            found["outside_hit" if mine is not None else "miss"] += 1
    assert all(v > 0 for v in found.values()), found
    print("spheres:", found)


def geometric_hit(poly, o, d):
    """What geometry would accept: the plane point on the inner side of every edge, measured ALONG THE NORMAL -- the
    reference (polygon.rs:54-56) looks at the z of the cross product only."""
    dotprod = S.dot(d, poly.plane_normal)
    if dotprod == 0.:
        return False
    dist = S.dot(S.sub(poly.plane_point, o), poly.plane_normal) / dotprod
    if dist < 0.:
        return False
    p = S.add(o, S.scaled(d, dist))
    n = len(poly.vertices)
    return all(S.dot(S.cross(S.sub(poly.vertices[k], p), S.sub(poly.vertices[(k + 1) % n], p)), poly.plane_normal) > 0. for k in range(n))


def test_polygons_bit_for_bit(O):
    rng = random.Random(20261202)
    pair = Pair(O)
    cases = []
    for n in range(3, 9):
        for winding in ("ccw", "cw"):
            for k in range(40):
                verts = ccw_polygon(rng, n, tilt_range=(2.5 if k % 2 else 0.5))
                if winding == "cw":
                    verts = verts[::-1]                   # the normal's z turns negative
                i = pair.polygon(verts, material(rng))
                target = point_in(rng, verts)
                o = (rng.uniform(-12., 12.), rng.uniform(-10., 10.), rng.uniform(-45., 10.))    # in front of it or behind
                d = S.normalized(S.sub(target, o)) if k % 4 else unit(rng)
                cases.append((i, n, winding, o, d))
    # flat polygons, z = -5: the normal's x and y are exactly zero, so a direction with no z is EXACTLY parallel
    # (`dotprod == 0.`, polygon.rs:66), and an origin with z = -5 lies ON the plane (`dist == 0.`: a hit, polygon.rs:74)
    flat = {4: [(0., 0., -5.), (4., 0., -5.), (4., 4., -5.), (0., 4., -5.)],
            8: [(2., 0., -5.), (4., 0., -5.), (6., 2., -5.), (6., 4., -5.), (4., 6., -5.), (2., 6., -5.), (0., 4., -5.), (0., 2., -5.)]}
    for n, verts in flat.items():
        i = pair.polygon(verts, material(rng))
        assert pair.mine[i].plane_normal[:2] == (0., 0.) and pair.mine[i].plane_point[2] == -5.
        for d in [(1., 0., 0.), (0., 1., 0.), (0.6, 0.8, 0.), (-1., 0., 0.)]:
            cases += [(i, n, "flat", (2.5, 2.5, -5.), d), (i, n, "flat", (-3., 1., -4.), d)]
        for d in [(0., 0., -1.), (0., 0., 1.), S.normalized((0.3, -0.2, -1.)), S.normalized((0.1, 0.1, 1.))]:
            cases += [(i, n, "flat", (2.5, 2.5, -5.), d), (i, n, "flat", (3., 1., -5.), d), (i, n, "flat", (9., 9., -5.), d)]
    found = dict(parallel=0, on_plane_hit=0, z_only_rejections=0, negative_normal_z=0)
    hits = {(n, w): 0 for n in range(3, 9) for w in ("ccw", "cw")}
    for i, n, winding, o, d in cases:
        mine = pair.intersect(i, o, d, ("polygon", n, winding, o, d))
        poly = pair.mine[i]
        dotprod = S.dot(d, poly.plane_normal)
        if dotprod == 0.:
            assert mine is None
            found["parallel"] += 1
            continue
        if S.dot(S.sub(poly.plane_point, o), poly.plane_normal) / dotprod == 0. and mine is not None:
            found["on_plane_hit"] += 1
        if poly.plane_normal[2] < 0.:
            found["negative_normal_z"] += 1
            assert mine is None                           # nothing passes inside() against a polygon clockwise in xy
            if geometric_hit(poly, o, d):
                found["z_only_rejections"] += 1
        if winding in ("ccw", "cw") and mine is not None:
            hits[(n, winding)] += 1
    assert all(v > 0 for v in found.values()), found
    assert all(hits[(n, "ccw")] > 0 and hits[(n, "cw")] == 0 for n in range(3, 9)), hits
    print("polygons:", found, hits)


def same_triangle(mine, theirs):
    return (all(same3(mine.vertices[k], theirs.vertices[k]) for k in range(3)) and same3(mine.normal, theirs.normal)
            and same3(mine.center, theirs.center))


def triangle_intersect(O, mine, theirs, o, d, what=""):
    got, out = mine.intersect(o, d), O.Intersection()
    flag = O.lib().orc_triangle_intersect(C.byref(theirs), O.v3(o), O.v3(d), C.byref(out))
    check_intersection(got, flag, out, what)
    return got


def test_triangles_bit_for_bit(O):
    L, rng = O.lib(), random.Random(20261203)
    found = dict(rotations_hit=0, reversed_rejected=0, reversed_would_hit=0, under_1e_6=0, over_1e_6_hit=0, on_plane_hit=0, moved=0)
    for k in range(300):
        v = ccw_polygon(rng, 3, tilt_range=(2.5 if k % 2 else 0.5))
        target = point_in(rng, v)
        o = (rng.uniform(-12., 12.), rng.uniform(-10., 10.), rng.uniform(-45., 10.))
        d = S.normalized(S.sub(target, o)) if k % 4 else unit(rng)
        off = (rng.uniform(-5., 5.), rng.uniform(-5., 5.), rng.uniform(-5., 5.))
        for order in ([0, 1, 2], [1, 2, 0], [2, 0, 1], [2, 1, 0]):
            w = [v[j] for j in order]
            mine, theirs = S.Triangle(w), L.orc_triangle_create(O.v3(w[0]), O.v3(w[1]), O.v3(w[2]))
            assert same_triangle(mine, theirs), ("create", w)
            got = triangle_intersect(O, mine, theirs, o, d, ("triangle", w, o, d))
            if order == [2, 1, 0]:
                assert got is None
                found["reversed_rejected"] += 1
                forward = S.Triangle(v).intersect(o, d)
                found["reversed_would_hit"] += forward is not None
            else:
                found["rotations_hit"] += got is not None
            # triangle.rs:19-24: the centre and the vertices move, the normal stays
            normal_before = mine.normal
            mine.offset(off)
            L.orc_triangle_offset(C.byref(theirs), O.v3(off))
            assert same_triangle(mine, theirs) and mine.normal == normal_before, ("offset", w, off)
            triangle_intersect(O, mine, theirs, o, d, ("moved triangle", w, off, o, d))
            found["moved"] += 1
    # |dot| just under and just over 1e-6 (triangle.rs:57): the normal is (0, 0, 1) exactly, so dot == -e exactly
    v = [(0., 0., 0.), (4., 0., 0.), (0., 4., 0.)]
    mine, theirs = S.Triangle(v), L.orc_triangle_create(O.v3(v[0]), O.v3(v[1]), O.v3(v[2]))
    assert mine.normal == (0., 0., 1.) and mine.center[2] == 0.
    for e in (0.9999e-6, math.nextafter(1e-6, 0.), 1e-6, math.nextafter(1e-6, 1.), 1.0001e-6):
        for sign in (1., -1.):
            d = (math.sqrt(1. - e * e), 0., -sign * e)
            got = triangle_intersect(O, mine, theirs, (1., 1., sign * 1e-7), d, ("near parallel", e, sign))
            if abs(S.dot(d, mine.normal)) < 1e-6:
                assert got is None
                found["under_1e_6"] += 1
            else:
                found["over_1e_6_hit"] += got is not None
    for d in [(0., 0., -1.), (0., 0., 1.), S.normalized((0.2, 0.1, -1.))]:          # dist == 0.: the origin on the plane
        got = triangle_intersect(O, mine, theirs, (1., 1., 0.), d, ("on plane", d))
        found["on_plane_hit"] += got is not None and got.point == (1., 1., 0.)
    assert all(x > 0 for x in found.values()), found
    assert found["under_1e_6"] == 4 and found["over_1e_6_hit"] == 6 and found["on_plane_hit"] == 3
    print("triangles:", found)


def test_obj_first_triangle_wins_a_tie(O):
    """obj.rs:198: `dist_hit < dist_closest` is strict, so of two coplanar duplicates the FIRST keeps the hit -- and with
    it the colour of the ramp (obj.rs:125-138), which is how the winner shows."""
    rng = random.Random(20261204)
    pair = Pair(O)
    found = dict(ties=0, first_won=0, hits=0, misses=0)
    for k in range(60):
        t = ccw_polygon(rng, 3, tilt_range=1.)
        other = ccw_polygon(rng, 3, tilt_range=1.)
        tris = [[t, t, other], [other, t, t], [t, other, t], [t, t]][k % 4]
        off = (0., float(rng.randint(-2, 2)), float(rng.randint(-5, 0)))
        i = pair.mesh(tris, off)
        obj = pair.mine[i]
        assert [r.diffuse_color for r in obj.reflectances] == [(1. - j / len(tris), j / len(tris), 1.) for j in range(len(tris))]
        for j in range(6):
            o = (rng.uniform(-12., 12.), rng.uniform(-10., 10.), rng.uniform(0., 10.))
            d = S.normalized(S.sub(S.add(point_in(rng, t), off), o)) if j else unit(rng)
            mine = pair.intersect(i, o, d, ("obj", k, j))
            singles = [tri.intersect(o, d) for tri in obj.triangles]
            dists = [None if s is None else S.squared_norm(S.sub(s.point, o)) for s in singles]
            found["hits" if mine is not None else "misses"] += 1
            if mine is None:
                continue
            best = min(x for x in dists if x is not None)
            tied = [j2 for j2, x in enumerate(dists) if x == best]
            if len(tied) > 1:
                found["ties"] += 1
                assert mine.reflectance.diffuse_color == obj.reflectances[tied[0]].diffuse_color
                found["first_won"] += 1
    assert all(v > 0 for v in found.values()), found
    print("obj ties:", found)


def test_scene_first_shape_wins_a_tie_and_the_index_wraps(O):
    rng = random.Random(20261205)
    found = dict(ties=0, wrapped=0, hits=0, misses=0)
    # duplicates under different materials: shapes.rs:130 is a strict `<`, the first of the two keeps the hit
    pair = Pair(O)
    dup = []
    for k in range(6):
        c, r = (rng.uniform(-8., 8.), rng.uniform(-6., 6.), rng.uniform(-30., -10.)), rng.uniform(1., 3.)
        dup.append((pair.sphere(c, r, material(rng)), pair.sphere(c, r, material(rng)), ("s", c, r)))
        verts = ccw_polygon(rng, 3 + k, tilt_range=0.5)
        dup.append((pair.polygon(verts, material(rng)), pair.polygon(verts, material(rng)), ("p", verts)))
    for k in range(400):
        a, b, geom = dup[k % len(dup)]
        target = S.add(geom[1], S.scaled(unit(rng), 0.9 * geom[2] * rng.random())) if geom[0] == "s" else point_in(rng, geom[1])
        o = (rng.uniform(-4., 4.), rng.uniform(-4., 4.), rng.uniform(0., 8.))
        d = S.normalized(S.sub(target, o)) if k % 5 else unit(rng)
        mine = pair.closest(o, d, ("tie", k))
        found["hits" if mine is not None else "misses"] += 1
        if mine is None:
            continue
        singles = [s.intersect(o, d) for s in pair.mine]
        dists = [None if s is None else S.squared_norm(S.sub(s.point, o)) for s in singles]
        best = min(x for x in dists if x is not None)
        tied = [j for j, x in enumerate(dists) if x == best]
        assert mine[1] == tied[0]
        if len(tied) > 1:
            found["ties"] += 1
            assert same_reflectance(mine[0].reflectance, pair.so.ptr.contents.shapes[tied[0]].reflectance)
    # 300 spheres in a plane, a ray at the centre of each: `shape_hit as u8` (shapes.rs:140) wraps from the 257th on
    wrap = Pair(O)
    centres = [((col - 9.5) * 3., (row - 7.) * 3., -60.) for row in range(15) for col in range(20)]
    for c in centres:
        wrap.sphere(c, 1., material(rng))
    for k, c in enumerate(centres):
        mine = wrap.closest(S.ZERO, S.normalized(c), ("wrap", k))
        assert mine is not None and mine[1] == k % 256 and mine[0].reflectance == wrap.mine[k].reflectance
        found["wrapped"] += k >= 256
    assert all(v > 0 for v in found.values()), found
    assert found["wrapped"] == 44
    print("scene ties and wrap:", found)


def test_optics_bit_for_bit(O):
    L, rng = O.lib(), random.Random(20261206)
    found = dict(c_neg=0, c_pos=0, c_zero=0, reflected=0, not_reflected=0, refracted=0, total_internal_reflection=0,
                 cos_theta_2_zero=0, index_below_one=0)
    cases = []
    for k in range(2000):
        ri = rng.uniform(1.05, 2.) if k % 4 else rng.uniform(0.5, 0.95)
        cases.append((unit(rng), unit(rng), (rng.uniform(-5., 5.), rng.uniform(-5., 5.), rng.uniform(-20., 0.)), ri))
    # c == 0.: the ray lies in the surface.  With index 1 that makes cos_theta_2 = 1 - 1 * (1 - 0) == 0. exactly -- the one
    # value at which reflect_ray (`> 0.` leaves) and refract_ray (`< 0.` leaves) BOTH produce a ray (optics.rs:33, 74).
    # (At normal incidence, c == 1, cos_theta_2 is 1 for every index: those cases are here as well.)
    for normal, incident in [((0., 1., 0.), (1., 0., 0.)), ((0., 1., 0.), (0., 0., -1.)), ((0., 0., 1.), (0.6, 0.8, 0.)),
                             ((0., 1., 0.), (0., -1., 0.)), ((0., 1., 0.), (0., 1., 0.))]:
        for ri in (1., 1.5, 0.75, 2.):
            cases.append((incident, normal, (1., 2., 3.), ri))
    for incident, normal, point, ri in cases:
        mine_isec = S.Intersection(point, normal, S.default_reflectance())
        theirs = O.Intersection(O.v3(point), O.v3(normal), L.orc_reflectance_default())
        assert same3(S.reflect(incident, normal), L.orc_reflect(O.v3(incident), O.v3(normal)))
        got = {}
        for name, fn, orc in (("reflect", S.reflect_ray, L.orc_reflect_ray), ("refract", S.refract_ray, L.orc_refract_ray)):
            mine, o, d = fn(incident, mine_isec, ri), O.Vec3(), O.Vec3()
            flag = orc(O.v3(incident), C.byref(theirs), ri, C.byref(o), C.byref(d))
            assert (mine is not None) == bool(flag), (name, incident, normal, ri)
            if mine is not None:
                assert same3(mine[0], o) and same3(mine[1], d), (name, incident, normal, ri, mine, o.tup(), d.tup())
            got[name] = mine
        c = S.dot(normal, incident)
        found["c_neg" if c < 0. else "c_pos" if c > 0. else "c_zero"] += 1
        found["reflected" if got["reflect"] is not None else "not_reflected"] += 1
        found["refracted" if got["refract"] is not None else "total_internal_reflection"] += 1
        for sign in (1., -1.):                            # reflect_ray's c is normal.incident, refract_ray's its negative
            cc = sign * c
            r = ri if cc < 0. else 1. / ri
            if 1. - r * r * (1. - cc * cc) == 0.:
                found["cos_theta_2_zero"] += 1
                assert got["reflect" if sign > 0. else "refract"] is not None
        found["index_below_one"] += ri < 1.
    assert all(v > 0 for v in found.values()), found
    print("optics:", found)


@pytest.mark.parametrize("w,h", [(32, 32), (96, 64), (800, 600)])
def test_backproject_every_pixel(O, Y, w, h):
    mine, theirs = S.Renderer(1.5, h, w), Y.renderer(w, h, 1.5)
    assert (mine.fov, mine.half_fov, mine.height, mine.width, mine.ratio) == (theirs.fov, theirs.half_fov, theirs.height, theirs.width, theirs.ratio)
    rays = np.array([[mine.backproject(x, y) for x in range(w)] for y in range(h)])
    assert np.array_equal(rays, Y.backproject(w, h, 1.5))
    assert rays.shape == (h, w, 3) and np.all(rays[..., 2] < 0.)


def test_normalized_bit_for_bit(O):
    L, rng = O.lib(), random.Random(20261207)
    vectors = [(rng.uniform(-9., 9.), rng.uniform(-9., 9.), rng.uniform(-9., 9.)) for _ in range(2000)]
    vectors += [S.ZERO, (0., 0., -0.), (5e-324, 0., 0.), (1e-200, 1e-200, 0.), (1e200, 1e200, 1.), (3., 4., 0.), (0., 0., -1.),
                (math.inf, 1., 1.), (math.nan, 1., 1.)]
    for v in vectors:
        assert same3(S.normalized(v), L.orc_normalized(O.v3(v))), v
        assert same3(S.normalized_l0(v), L.orc_normalized_l0(O.v3(v))), v
    assert S.normalized(S.ZERO) == S.ZERO                                  # geometry.rs:106: `norm > 0.` guards the division


# ================================================================ c. whole rays and frames
def descriptions():
    d = {"demo": {"default": True}, "cornell": SC.obj_description("cornell_box.obj"), "dodecahedron": SC.obj_description("dodecahedron.obj"),
         "manygons": SC.manygons_description()}
    d["synthetic256"] = dict(
        shapes=[("sphere", sp["center"], sp["radius"], workloads._synthetic_material(sp)) for sp in workloads.load_synthetic()]
        + [("polygon", workloads.FLOOR_QUAD, workloads.FLOOR_MATERIAL)], lights=workloads.DEMO_LIGHTS, camera=(0., 0., 0.))
    d["penumbra"] = dict(shapes=[("polygon", SR.PENUMBRA_FLOOR, SR.PENUMBRA_FLOOR_MATERIAL), ("sphere",) + SR.PENUMBRA_SPHERE + (RR.GLASS,)],
                         lights=SR.PENUMBRA_LIGHTS, camera=(0., 0., 0.))
    for seed in FUZZ_SEEDS:
        d["fuzz%d" % seed] = TP.fuzz_recipe(seed)
    return d


SCENES = ["demo", "cornell", "dodecahedron", "synthetic256", "penumbra", "manygons"] + ["fuzz%d" % s for s in FUZZ_SEEDS]

# What the second reading alone finds in the 64x39 frames at depth cap 6, per camera (origin, off, inside): pixels that hit,
# pixels whose first hit is shadowed from at least one light, pixels whose first hit is glass, and refract_ray calls that
# ended in total internal reflection anywhere in the pixel's tree.  Committed so that a scene cannot quietly go vacuous.
FOUND = {
    "demo": {"origin": (864, 73, 458, 0), "off": (611, 119, 319, 0), "inside": (2048, 2048, 2048, 1188)},
    "cornell": {"origin": (303, 0, 0, 0), "off": (1013, 293, 0, 0), "inside": (309, 0, 0, 0)},
    "dodecahedron": {"origin": (40, 0, 0, 0), "off": (237, 12, 0, 0), "inside": (47, 0, 0, 0)},
    "synthetic256": {"origin": (739, 75, 533, 1), "off": (587, 67, 434, 0), "inside": (922, 153, 674, 0)},
    "penumbra": {"origin": (376, 149, 76, 0), "off": (299, 102, 46, 0), "inside": (693, 502, 413, 0)},
    "manygons": {"origin": (1014, 382, 329, 187), "off": (708, 299, 119, 29), "inside": (1343, 704, 618, 120)},
    "fuzz0": {"origin": (450, 107, 347, 0), "off": (290, 76, 214, 0), "inside": (543, 150, 396, 0)},
    "fuzz1": {"origin": (154, 16, 3, 0), "off": (128, 17, 1, 0), "inside": (128, 30, 5, 0)},
    "fuzz2": {"origin": (741, 649, 433, 1), "off": (483, 423, 274, 0), "inside": (876, 740, 303, 1)},
    "fuzz3": {"origin": (71, 38, 47, 0), "off": (52, 27, 35, 0), "inside": (127, 71, 92, 0)},
    "fuzz4": {"origin": (791, 647, 322, 30), "off": (622, 518, 321, 25), "inside": (993, 789, 508, 6)},
    "fuzz5": {"origin": (176, 15, 40, 0), "off": (131, 12, 32, 0), "inside": (179, 20, 84, 0)},
    "fuzz6": {"origin": (445, 308, 195, 0), "off": (335, 231, 136, 0), "inside": (706, 587, 409, 0)},
    "fuzz7": {"origin": (98, 17, 0, 0), "off": (67, 12, 0, 0), "inside": (239, 20, 0, 0)},
    "fuzz8": {"origin": (437, 108, 251, 1), "off": (285, 78, 167, 1), "inside": (563, 233, 296, 1)},
    "fuzz9": {"origin": (339, 39, 20, 0), "off": (263, 26, 15, 1), "inside": (380, 193, 38, 0)},
    "fuzz10": {"origin": (1374, 451, 359, 15), "off": (918, 348, 270, 14), "inside": (2026, 1808, 222, 0)},
    "fuzz11": {"origin": (166, 5, 2, 0), "off": (107, 7, 7, 0), "inside": (301, 124, 127, 0)},
}

# The counters a scene is there to exercise, non-zero in the sum over its cameras: hits and shadows in every scene (the
# Cornell box among them), glass first hits wherever the scene holds glass (fuzz7 holds none, the .obj scenes cannot), total
# internal reflection in the demo -- from the camera inside its sphere -- and among the glass polygons.  A glass sphere seen
# from outside never reflects totally (the ray leaves at the angle it came in by), hence no such demand on the penumbra scene.
NEEDS_GLASS = ["demo", "manygons", "synthetic256", "penumbra"] + ["fuzz%d" % s for s in FUZZ_SEEDS if s != 7]
NEEDS_TIR = ["demo", "manygons"]


@pytest.fixture(scope="module")
def second_frames():
    """Every frame of part c, read by the second reading once: {(scene, camera, (w, h), depth): (rgb, probes)}"""
    desc = descriptions()
    keys = [(name, cam, size, depth) for name in SCENES for cam in SC.CAMERAS for size in SIZES for depth in DEPTHS]
    t0 = time.time()
    results = SC.render_jobs([(desc[name], SC.cameras_of(name)[cam], size[0], size[1], depth) for name, cam, size, depth in keys])
    print("second reading: %d frames in %.1f s" % (len(keys), time.time() - t0))
    return desc, dict(zip(keys, results))


def counters(probes):
    return (sum(1 for p in probes.values() if p[0]), sum(1 for p in probes.values() if p[3] > 0),
            sum(1 for p in probes.values() if p[2]), sum(p[4] for p in probes.values()))


def hold_frames(O, Y, desc, frames, name, cameras, sizes, depths, label=None):
    """The oracle's frames of one scene against the second reading's: decisions equal at every pixel, every channel within
    TIGHT, the remainder rows zero in both.  -> the largest deviation seen"""
    worst = 0.
    for cam in cameras:
        eye = SC.cameras_of(name)[cam]
        so = SC.oracle_scene(O, desc, eye)
        for w, h in sizes:
            rows = h - h % 32
            dirs = Y.backproject(w, h)[:rows].reshape(-1, 3)
            _, first, shape = Y.cast(so, eye, dirs, 1, want_first=True)
            first, shape = first.reshape(rows, w), shape.reshape(rows, w)
            for depth in depths:
                rgb, probes = frames[(label or name, cam, (w, h), depth)]
                mine = np.array(rgb, dtype=np.float64)
                assert mine.shape == (h, w, 3) and len(probes) == rows * w
                theirs = O.render(so, w, h, max_depth=depth)
                assert np.all(mine[rows:] == 0.) and np.all(theirs[rows:] == 0.)
                for (y, x), (hit, index, glass, _, _, _) in probes.items():
                    assert hit == (first[y, x] != -1), ("first hit", name, cam, (w, h), y, x)
                    assert index == shape[y, x], ("shape index", name, cam, (w, h), y, x, index, shape[y, x])
                    assert glass == (first[y, x] == 1), ("glass", name, cam, (w, h), y, x)
                dev = float(np.abs(mine - theirs).max())
                assert dev < TIGHT, (name, cam, (w, h), depth, dev)
                worst = max(worst, dev)
    return worst


@pytest.mark.parametrize("name", SCENES)
def test_frames_of_both_readings(O, Y, second_frames, name):
    desc, frames = second_frames
    worst = hold_frames(O, Y, desc[name], frames, name, list(SC.CAMERAS), SIZES, DEPTHS)
    found = {cam: counters(frames[(name, cam, (64, 39), 6)][1]) for cam in SC.CAMERAS}
    print("%s: largest |second reading - oracle| %.3e; found %r" % (name, worst, found))
    total = [sum(found[cam][k] for cam in found) for k in range(4)]
    assert total[0] > 0 and total[1] > 0, found
    assert total[2] > 0 or name not in NEEDS_GLASS, found
    assert total[3] > 0 or name not in NEEDS_TIR, found
    if name == "cornell":
        assert found["off"][0] > 0 and found["off"][1] > 0, found             # inside the box: hits, and the blocks' shadows
    if name == "demo":
        assert found["inside"][2] > 0 and found["inside"][3] > 0, found      # from inside the glass sphere
    assert found == FOUND[name], (name, found)


def test_the_fuzz_recipe_draws_what_the_fuzz_always_drew():
    """tests/test_gpu_parity.py's _fuzz_scene was rebuilt on fuzz_recipe.  Before and after, the oracle's frames of seeds
    0-11 were byte-identical (sha256 of every frame compared on the CPU when the recipe was lifted out).  What is pinned
    here for good is the part of the recipe no library can round differently -- every draw that reaches the scene
    without passing through cos or sin: a draw added, dropped or moved shifts every later one."""
    h = hashlib.sha256()
    for seed in FUZZ_SEEDS:
        r = TP.fuzz_recipe(seed)
        for shape in r["shapes"]:
            if shape[0] == "sphere":
                h.update(repr(("s", shape[1], shape[2], sorted(shape[3].items()))).encode())
            elif shape[0] == "polygon":
                h.update(repr(("p", len(shape[1]), sorted(shape[2].items()))).encode())
            else:
                h.update(repr(("m", np.asarray(shape[1]).tolist(), shape[2])).encode())
        h.update(repr((r["lights"], r["camera"], r["width"], r["height"], r["depth"])).encode())
    assert h.hexdigest() == FUZZ_RECIPE_SHA256


FUZZ_RECIPE_SHA256 = "1e4a2397d77a37bd30b01931285d2604f227d542393f313bab41f43de2071e4c"


# ================================================================ d. moved shapes
# the Cornell box's first wall and its two blocks (models 6 and 7, ten triangles each), seen from inside the box; the demo's
# triangle and floor (scene.rs:200-207: shapes 4 and 5), seen from the origin
MOVES = {"cornell": {1: (1.25, -0.5, 3.), 6: (-20., 0.75, -15.5), 7: (30.125, 4., 12.)},
         "demo": {4: (-1.5, 0.25, -2.), 5: (0.5, -0.75, 1.)}}
MOVED_CAMERA = {"cornell": "off", "demo": "origin"}


@pytest.mark.parametrize("name", ["cornell", "demo"])
def test_moved_records_of_the_product(pkg, name):
    """rm_scene_offset_shape, the host half (no GPU): the flattened scene's records after offset() equal the second
    reading's as bits.  The demo is built by the library (Scene.create_default) and moved IN PLACE, shapes[i].offset(..):
    flatten() once handed back the prebuilt handle there and the move was lost."""
    moved = dict(descriptions()[name], moves=MOVES[name])
    mine = SC.second_scene(moved)
    d = SC.product_scene(pkg, moved).flatten().desc()
    assert d.n_shapes == len(mine.shapes)
    for index in MOVES[name]:
        ref, b = d.shapes[index], mine.shapes[index]
        if isinstance(b, S.Obj):
            assert ref.count == len(b.triangles)
            for t in range(ref.count):
                assert same_triangle(b.triangles[t], d.triangles[ref.first + t]), (name, index, t)
        else:
            p = d.polygons[ref.first]
            assert p.n_vertices == len(b.vertices)
            assert all(same3(b.vertices[k], d.polygon_vertices[p.first_vertex + k]) for k in range(p.n_vertices)), (name, index)
            assert same3(b.plane_normal, p.plane_normal) and same3(b.plane_point, p.plane_point), (name, index)


@pytest.mark.parametrize("name", ["cornell", "demo"])
def test_moved_shapes(O, Y, name):
    """offset() on the Cornell box's meshes and on the demo's two polygons: the records of both readings stay equal as bits,
    the normals are those of before the move, and the 32x32 frames of the moved scenes agree as in part c."""
    base = descriptions()[name]
    moved = dict(base, moves=MOVES[name])
    cam = MOVED_CAMERA[name]
    eye = SC.cameras_of(name)[cam]
    before, mine, so = SC.second_scene(base, eye), SC.second_scene(moved, eye), SC.oracle_scene(O, moved)
    records = 0
    for index, off in MOVES[name].items():
        a, b, theirs = before.shapes[index], mine.shapes[index], so.ptr.contents.shapes[index]
        if isinstance(b, S.Obj):
            assert theirs.kind == 2 and theirs.n_triangles == len(b.triangles)
            for t in range(len(b.triangles)):
                assert same_triangle(b.triangles[t], theirs.triangles[t]), (name, index, t)
                assert b.triangles[t].normal == a.triangles[t].normal
                assert b.triangles[t].center == S.add(a.triangles[t].center, off)
                assert b.triangles[t].vertices == [S.add(v, off) for v in a.triangles[t].vertices]
                records += 1
        else:
            assert theirs.kind == 1 and theirs.n_vertices == len(b.vertices)
            assert all(same3(b.vertices[k], theirs.vertices[k]) for k in range(len(b.vertices)))
            assert same3(b.plane_normal, theirs.plane_normal) and same3(b.plane_point, theirs.plane_point)
            assert b.plane_normal == a.plane_normal and b.plane_point == S.add(a.plane_point, off)
            assert b.vertices == [S.add(v, off) for v in a.vertices]
            records += 1
    assert records > 0
    frames = {}
    for depth in (1, 3, 6):
        frame, probes = S.render_frame(mine, 32, 32, max_depth=depth, probe=True)
        frames[(name, cam, (32, 32), depth)] = (frame.buffer, probes)
    worst = hold_frames(O, Y, moved, frames, name, [cam], [(32, 32)], [1, 3, 6])
    still, _ = S.render_frame(before, 32, 32, max_depth=3)
    assert still.buffer != frames[(name, cam, (32, 32), 3)][0]                 # the move shows in the frame
    assert counters(frames[(name, cam, (32, 32), 3)][1])[0] > 0
    print("%s moved: largest |second reading - oracle| %.3e" % (name, worst))
