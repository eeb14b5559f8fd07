"""The scenes and ray sets of the variant matrix: recipes that make every template argument of radiance_steps<BVH, POW, STACK,
LIGHTS> (csrc/rm_radiance_step.inc) matter, built as a product scene and an oracle scene through their own APIs, and the
structured rays of the hierarchy walks.  No GPU and no fixtures: tests/test_variant_matrix.py pins on the CPU that a cell takes
the kernel it claims and that the oracle alone tells the variants apart; tests/test_gpu_variant_matrix.py and
tests/test_gpu_structured_rays.py hold the GPU to the oracle.

A cell is (bvh, generic, depth):
  bvh      "flat": the core alone -- a zig-zag of glass panes in front of lit opaque spheres, 5 spheres and no mesh, so the scene
           image carries no hierarchy; "spheres": + 20 small spheres (a third glass, some on integer centres): a sphere
           hierarchy; "mesh": + a mesh of 14 triangles instead: a triangle hierarchy.
  generic  two opaque materials and one pane material get the exponents 12.5 and 0.5: the image's integer_exponents verdict
           falls and the launchers take POW_GENERIC.  The integer cells keep exponents 0 and 1000 among theirs.
  depth    5: the last depth with STACK = 4, which a primary ray through the panes fills to the brim; 6: the first with 32.

The panes: optics.rs gives a glass surface both children only where the ray meets its front at more than asin(1 / ri) off
the normal, so the panes are tilted +-30 degrees in turn about the y axis and have ri = 3.5 (16.6 degrees): a ray down the z
axis zig-zags through them at 30 to 50 degrees of incidence and parks a reflected sibling at every pane."""
import ctypes as C

import numpy as np

import radiance_reference as RR
import test_gpu_query as GQ

TIGHT = RR.TIGHT
RESOLVE = 1e-6                       # a thousand TIGHT: what two variants' answers must differ by to count as told apart
SHARE = 0.05                         # ... on at least this share of the rays or pixels
W = H = 32
N_RAYS = 1100                        # 17 waves and 12 lanes: the last wave has idle lanes
EYE = (0., 0., 0.)
LIGHTS = [((0.5, 1., 0.), (1., 1., 1.), 1.), ((6., 8., -6.), (1., 0.6, 0.4), 0.7), ((-5., 9., -14.), (0.5, 0.6, 1.), 0.6)]
RADII = (3., 2., 1.5)                # the area lights of the soft and the converging cells, one radius a light
APERTURE, FOCUS = 0.5, 12.           # the third pane (z = -12) lies in the plane in focus
REFINE_N, REFINE_THRESHOLD = 2, 0.25
LENS_SAMPLES = 5                     # 12 pixels a wave, four idle lanes
CONVERGE = (4, 0.1, 8, 32)           # samples a pass, tolerance, min_samples, max_samples
BOUNCE_FIRST, BOUNCE_ROWS = 3, 10    # the bounce cells' rows of the three sequences: two passes of 5
# Pixels of the 32 x 32 frame on which the bounce's share of it (the frame at strength 1 less the frame at strength 0, through
# the lens, under the area lights) differs by more than RESOLVE, counted with the oracle alone (tests/test_variant_matrix.py):
# scene -> (from no bounce at all, depth 5 against 4, depth 6 against 5 -- None: no such cell --, exponent 12.5 against 12)
BOUNCE_SHARE = {"flat": (103, 9, 7, 26), "spheres": (150, 15, 10, 37), "mesh": (129, 8, None, None)}

CELLS = [(bvh, generic, depth) for bvh in ("flat", "spheres") for generic in (False, True) for depth in (5, 6)] + [("mesh", False, 5)]
SCENES = sorted({c[:2] for c in CELLS})
HALF = 12.5                          # the exponent the resolving-power pin replaces by 12


def cell_id(cell):
    return "%s-%s-%d" % (cell[0], "generic" if cell[1] else "integer", cell[2])


def claims(cell):
    """What the launchers must see for the cell: (a sphere hierarchy, a triangle hierarchy, integer exponents, max_depth <= 5)."""
    bvh, generic, depth = cell
    return bvh == "spheres", bvh == "mesh", not generic, depth <= 5


# ---------------------------------------------------------------- the recipe
def _material(exponent, glass=False, colour=(0.8, 0.8, 0.8), ri=1.5, reflection=0.4, diffusion=0.7, specular=0.9):
    return dict(diffusion=diffusion, diffuse_color=colour, specular=specular, specular_exponent=float(exponent), is_glass_like=glass,
                reflection=reflection if glass else 0., refractive_index=ri if glass else 1.)


def materials(generic, half=HALF):
    """name -> Reflectance fields.  generic: opaque `back` and pane `even` get `half` (12.5), opaque `right` 0.5."""
    return {
        "even": _material(half if generic else 20., True, (0.9, 0.8, 0.7), ri=PANE_RI, diffusion=0.3),
        "odd": _material(0., True, (0.7, 0.8, 0.9), ri=PANE_RI, diffusion=0.2, specular=0.6),
        "back": _material(half if generic else 50., colour=(0.9, 0.3, 0.2)),
        "right": _material(0.5 if generic else 30., colour=(0.2, 0.8, 0.3)),
        "left": _material(1000., colour=(0.3, 0.4, 0.9), specular=1.),
        "below": _material(0., colour=(0.8, 0.8, 0.3), diffusion=0.5, specular=0.5),
        "marble": _material(8., True, (0.9, 0.9, 0.9), ri=1.5, diffusion=0.3),
        "small": _material(30., colour=(0.6, 0.5, 0.7)),
    }


PANE_Z = (-4., -8., -12., -16., -20., -24.)
PANE_TILT, PANE_RI = 30., 3.5


def panes():
    """Six quads about the z axis, tilted +30 and -30 degrees about y in turn, facing the camera, counter-clockwise in xy."""
    out = []
    for k, z in enumerate(PANE_Z):
        a = np.deg2rad(PANE_TILT if k % 2 == 0 else -PANE_TILT)
        u = np.array([np.cos(a), 0., -np.sin(a)]) * 4.
        v = np.array([0., 3.5, 0.])
        c = np.array([0., 0., z])
        out.append([tuple(float(x) for x in c + su * u + sv * v) for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1))])
    return out


CORE_SPHERES = [((0., 0., -34.), 6., "back"), ((8., 0., -9.), 3., "right"), ((-8., 1., -12.), 3., "left"), ((0., -8., -10.), 3.5, "below"),
                ((2.5, 3.75, -7.), 1., "marble")]


def small_spheres():
    """20 spheres off the panes' axis: every third glass, every fourth on an integer centre."""
    rng = np.random.default_rng(20261301)
    out = []
    while len(out) < 20:
        c = rng.uniform((-5., -4., -20.), (5., 4., -3.))
        if np.hypot(c[0], c[1]) < 1.5:
            continue
        k = len(out)
        if k % 4 == 0:
            c = np.round(c)
        out.append((tuple(float(x) for x in c), float(rng.uniform(0.3, 0.9)), "marble" if k % 3 == 0 else "small"))
    return out


def mesh_triangles():
    """14 triangles, counter-clockwise in xy, in two rows beside the panes."""
    tri = np.empty((14, 9))
    for t in range(14):
        x, y, z = (-4.5 if t % 2 else 2.75), -3. + 0.875 * (t // 2), -5. - 1.5 * (t // 2)
        tri[t] = [x, y, z, x + 1.75, y + 0.25 * (t % 3), z - 0.5, x + 0.5, y + 1.5, z + 0.25 * (t % 2)]
    return tri


def scene_pair(pkg, O, bvh, generic, half=HALF):
    """-> (product Scene -- None without `pkg` --, oracle scene) of the parts (bvh, generic), from the one recipe above."""
    s, o = (pkg.Scene.new() if pkg is not None else None), O.OracleScene()
    M = materials(generic, half)

    def sphere(c, r, m):
        if s is not None:
            s.shapes.append(pkg.sphere.create(pkg.Vec3f(*c), r, pkg.Reflectance(**M[m])))
        o.add_sphere(c, r, O.reflectance(**M[m]))

    for k, q in enumerate(panes()):
        m = M["even" if k % 2 == 0 else "odd"]
        if s is not None:
            s.shapes.append(pkg.polygon.ConvexPolygon.create([pkg.Vec3f(*p) for p in q], pkg.Reflectance(**m)))
        o.add_polygon(q, O.reflectance(**m))
    for c, r, m in CORE_SPHERES:
        sphere(c, r, m)
    if bvh == "spheres":
        for c, r, m in small_spheres():
            sphere(c, r, m)
    elif bvh == "mesh":
        tri = mesh_triangles()
        if s is not None:
            s.shapes.append(pkg.obj.Obj(tri))
        o.add_obj(tri)
    else:
        assert bvh == "flat"
    for pos, col, inten in LIGHTS:
        if s is not None:
            s.lights.append(pkg.create_light(pkg.Vec3f(*pos), pkg.Vec3f(*col), inten))
        o.add_light(pos, col, inten)
    if s is not None:
        s.camera = pkg.Vec3f(*EYE)
    o.set_camera(EYE)
    return s, o


def ray_list(n=N_RAYS):
    """n rays: three quarters from about the camera down the panes, up to 0.3 off the axis in x and 0.45 in y per unit of z;
    an eighth from anywhere in the scene in any direction; an eighth from about the camera into the sky."""
    rng = np.random.default_rng(20261302)
    o = np.column_stack([rng.uniform(-1., 1., n), rng.uniform(-1.5, 1.5, n), rng.uniform(-1., 1., n)])
    d = GQ.unit(np.column_stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.45, 0.45, n), -np.ones(n)]))
    k = n // 8
    o[:k], d[:k] = GQ.random_rays(rng, k, (-9., -9., -30.), (9., 9., 2.))
    d[k:2 * k] = GQ.unit(np.column_stack([rng.uniform(-0.3, 0.3, k), np.ones(k), rng.uniform(0.2, 0.8, k)]))
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def sample_positions(n=N_RAYS):
    """n real-valued sample positions of the W x H frame."""
    return np.random.default_rng(20261303).uniform((0., 0.), (W, H), size=(n, 2))


def register(yardstick, name, pair):
    """Makes `pair` the scene `name` of one of the references' Yardsticks (they look scenes up by name, each made once)."""
    yardstick._scene[name] = pair
    return name


class Matrix:
    """The scenes of the matrix, the rays and the oracle's answers, each made once and shared (never written to)."""

    def __init__(self, pkg, O, orc):
        self.pkg, self.O, self.orc = pkg, O, orc
        self._pair, self._ref = {}, {}
        self.o, self.d = ray_list()
        self.xy = sample_positions()
        for a in (self.o, self.d, self.xy):
            a.setflags(write=False)

    def pair(self, bvh, generic, half=HALF):
        key = (bvh, generic, half)
        if key not in self._pair:
            self._pair[key] = scene_pair(self.pkg if half == HALF else None, self.O, bvh, generic, half)
        return self._pair[key]

    def name(self, bvh, generic):
        return "matrix-%s-%s" % (bvh, "generic" if generic else "integer")

    def rays(self, bvh, generic, depth, half=HALF):
        """orc_cast_ray along the ray list."""
        key = ("rays", bvh, generic, depth, half)
        if key not in self._ref:
            self._ref[key] = self.orc.cast(self.pair(bvh, generic, half)[1], self.o, self.d, depth)
            self._ref[key].setflags(write=False)
        return self._ref[key]

    def samples(self, bvh, generic, depth, xy=None, half=HALF):
        """orc_cast_ray along the sample rays of `xy` (the real-valued positions by default) from the camera, fixed view."""
        key = ("samples", bvh, generic, depth, half, None if xy is None else xy.tobytes())
        if key not in self._ref:
            d = RR.sample_directions(self.xy if xy is None else xy, self.orc.renderer(W, H))
            self._ref[key] = self.orc.cast(self.pair(bvh, generic, half)[1], EYE, d, depth, normalize=True)
            self._ref[key].setflags(write=False)
        return self._ref[key]

    def pixels(self, bvh, generic, depth, half=HALF):
        """The W x H frame of primary rays, [H * W][3]."""
        return self.samples(bvh, generic, depth, RR.pixel_positions(W, H), half)


def told_apart(a, b):
    """The share of rows of which some channel differs by more than RESOLVE."""
    return float((np.abs(a - b) > RESOLVE).any(axis=1).mean())


# ---------------------------------------------------------------- cast_ray's tree, replayed
def parked_at_once(O, oscene, o, d, max_depth):
    """cast_ray (renderer.rs:254-309) along one ray with the oracle's own pieces, walked as a lane walks it -- into the
    refracted child first, the reflected sibling waiting -- -> the largest number of live siblings waiting at once."""
    L, sc = O.lib(), oscene.c
    stack, most = [], 0
    ray = (O.v3(o), O.v3(d), 1)
    while ray is not None:
        orig, dirn, depth = ray
        ray = None
        hit = O.Intersection()
        if L.orc_find_closest_intersect(orig, dirn, sc.shapes, sc.n_shapes, C.byref(hit), None) and hit.reflectance.is_glass_like \
                and depth + 1 <= max_depth:
            ro, rd, to, td = O.Vec3(), O.Vec3(), O.Vec3(), O.Vec3()
            has_r = L.orc_reflect_ray(dirn, C.byref(hit), hit.reflectance.refractive_index, C.byref(ro), C.byref(rd))
            has_t = L.orc_refract_ray(dirn, C.byref(hit), hit.reflectance.refractive_index, C.byref(to), C.byref(td))
            if has_r and has_t:
                stack.append((ro, rd, depth + 1))
                most = max(most, len(stack))
            if has_t:
                ray = (to, td, depth + 1)
            elif has_r:
                ray = (ro, rd, depth + 1)
        if ray is None and stack:
            ray = stack.pop()
    return most


# ---------------------------------------------------------------- structured rays for the hierarchy walks
LATTICE = [(float(x), float(y), float(z)) for z in (-4, -6, -8, -10) for y in (-3, -1, 1, 3) for x in (-3, -1, 1, 3)]


def lattice_triangles():
    """16 triangles with legs along x and y, counter-clockwise in xy, eight in the plane z = -12 and eight in z = -2.5."""
    tri = []
    for z in (-12., -2.5):
        for k in range(8):
            x, y = -4. + 2. * (k % 4), -2. + 2. * (k // 4)
            tri.append([x, y, z, x + 2., y, z, x, y + 2., z] if k % 2 == 0 else [x + 2., y + 2., z, x, y + 2., z, x + 2., y, z])
    return np.array(tri)


def lattice_shapes():
    """4 x 4 x 4 unit spheres on odd integer centres, so that neighbours touch in a point; the mesh; the first sphere again."""
    return [("sphere", c, 1.) for c in LATTICE] + [("mesh", lattice_triangles()), ("sphere", LATTICE[0], 1.)]


def structured_directions():
    """The six axis directions and the twelve (+-1, +-1, 0) / sqrt(2), with both 0. and -0. in every zero component: (48, 3)."""
    out = []
    r = 1. / np.sqrt(2.)
    for axis in range(3):
        a, b = [k for k in range(3) if k != axis]
        for s in (1., -1.):
            for za in (0., -0.):
                for zb in (0., -0.):
                    v = [0., 0., 0.]
                    v[axis], v[a], v[b] = s, za, zb
                    out.append(v)
        for sa in (r, -r):                                            # `axis` is the zero component of a diagonal
            for sb in (r, -r):
                for z in (0., -0.):
                    v = [0., 0., 0.]
                    v[axis], v[a], v[b] = z, sa, sb
                    out.append(v)
    return np.array(out)


ORIGIN_X = (-7., -4., -3., -2.5, -1., 0., 1., 2., 3.5)
ORIGIN_Y = (-7., -3., -2., -1., 0., 0.5, 1., 3.)
ORIGIN_Z = (1., 0., -2.5, -4., -5., -6.5, -7., -12., -16.)


def structured_rays(shift=0.):
    """Every direction from every origin of an integer and half-integer lattice: sphere centres, points inside the spheres, on
    them, between them and outside the scene's bounds.  shift: written into one zero component of every direction (+-, as the
    zero's sign says) -- 1e-160 is below the slab test's threshold and leaves the length as it is."""
    d0 = structured_directions()
    if shift:
        for v in d0:
            k = int(np.flatnonzero(v == 0.)[0])
            v[k] = np.copysign(shift, v[k])
    origins = np.array([(x, y, z) for z in ORIGIN_Z for y in ORIGIN_Y for x in ORIGIN_X])
    o = np.repeat(origins, len(d0), axis=0)
    d = np.tile(d0, (len(origins), 1))
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def incidences(ref_scene, o, d):
    """With tests/ranged_reference.py's Scene over [0, inf] -> (rays exactly tangent to a sphere they hit: both roots equal,
    rays whose closest distance two primitives share exactly, rays that hit, the shape first in list order at that
    distance or -1)."""
    lo, hi = np.zeros(len(o)), np.full(len(o), np.inf)
    tangent, hit = np.zeros(len(o), bool), np.zeros(len(o), bool)
    best, ties, shape = np.full(len(o), np.inf), np.zeros(len(o), np.int64), np.full(len(o), -1, np.int64)
    for kind, si, el, data, ok, t, _ in ref_scene._accepted(o, d, lo, hi):
        if kind == "sphere":
            alive, t0, t1 = ref_scene._sphere(data, o, d)
            tangent |= ok & alive & (t0 == t1)
        with np.errstate(all="ignore"):
            dp = d * t[:, None]                                       # (p - o, with p = o + d t rounded as the reference does)
            p = o + dp
            dp = p - o
            dist = dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1] + dp[:, 2] * dp[:, 2]
        nearer, same = ok & (dist < best), ok & (dist == best)
        ties = np.where(nearer, 1, ties + same)
        best = np.where(nearer, dist, best)
        shape = np.where(nearer, si, shape)
        hit |= ok
    return tangent, hit & (ties > 1), hit, shape
