"""Probe builder of tests/test_gpu_grazing.py (plain Python, CPU only; checked by tests/test_grazing_probes.py).

A probe is a primitive smaller than a pixel, placed where a culling bound is at its edge: on the ray of a tile's corner
pixel (centred), or beside it so that only that ray grazes it (tangent).  Every ray used here comes from the oracle --
orc_backproject (or, for the oriented camera, the rays of test_gpu_camera.OracleCamera), orc_normalized,
orc_find_closest_intersect, orc_reflect_ray / orc_refract_ray -- and what is done with them is placement only (a point on a
ray, a step perpendicular to it): no formula of a kernel, a cone or a bound is restated.

Every list is fixed by its seed.  `live_*` are the checks that keep a list honest: they run on the CPU, with the oracle
alone, and tests/test_grazing_probes.py runs them for every list the GPU tests use."""
import ctypes as C
import math

import numpy as np

import workloads

TILE_W, TILE_H, PATCH = 16, 4, 32
T_VALUES = (3., 40., 4000.)
# The tangent probes' inset: the centre is r (1 - EPS) off the ray.  2^-29 is the power of two closest to a true tangent
# for which every tangent probe of every list below is live in the oracle: at 2^-30 the t = 4000 probes of the 512x448
# frames die (the reference's d2 = |line|^2 - tca^2 is ~1.6e7 there and its rounding, ~4e-9, reaches the inset 2 EPS r^2).
EPS = 2. ** -29

LIGHTS = [((0., 10., 0.), (1., 1., 1.), 1.), ((10., 15., 5.), (1., 0.8, 0.6), 0.7)]
MATERIALS = [
    dict(),
    dict(diffusion=0.7, diffuse_color=(0.9, 0.3, 0.2), specular=0.8, specular_exponent=12.5, reflection=0.5),
    dict(diffusion=0.4, diffuse_color=(0.6, 0.9, 0.7), specular=0.9, specular_exponent=20., is_glass_like=True, reflection=0.4,
         refractive_index=1.5),
    dict(diffusion=0.9, diffuse_color=(0.2, 0.5, 1.), specular=0.3, specular_exponent=100.),
]


# ---------------------------------------------------------------- rays
def unit(O, v):
    return np.array(O.lib().orc_normalized(O.v3(v)).tup())


def norm(O, v):
    """(the oracle's dot product, one rounding an operation, so that a list is the same list on every machine)"""
    return math.sqrt(O.lib().orc_squared_norm(O.v3(v)))


class View:
    """The primary rays of a frame as the oracle forms them: fixed view (orc_backproject) or, with `basis` and the
    OracleCamera `cam`, the oriented one (the helper's directions, normalised by orc_normalized)."""

    def __init__(self, O, w, h, eye=(0., 0., 0.), basis=None, cam=None, fov=workloads.FOV):
        self.O, self.w, self.h, self.rows = O, w, h, (h // PATCH) * PATCH
        self.eye = np.array(eye, dtype=np.float64)
        self.basis = basis
        self._r = O.lib().orc_create_renderer(float(fov), float(h), float(w))
        self._d = cam.directions(basis, w, h, fov) if basis is not None else None
        self._rays = {}

    def inside(self, x, y):
        return 0 <= x < self.w and 0 <= y < self.rows

    def ray(self, x, y):
        if (x, y) not in self._rays:
            if self._d is None:
                self._rays[(x, y)] = np.array(self.O.lib().orc_backproject(C.byref(self._r), x, y).tup())
            else:
                self._rays[(x, y)] = unit(self.O, self._d[y, x])
        return self._rays[(x, y)]

    def neighbours(self, x, y):
        return [(x + dx, y + dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx or dy) and self.inside(x + dx, y + dy)]

    def tile_pixels(self, x, y):
        x0, y0 = x // TILE_W * TILE_W, y // TILE_H * TILE_H
        return [(x0, y0), (x0 + TILE_W - 1, y0), (x0, y0 + TILE_H - 1), (x0 + TILE_W - 1, y0 + TILE_H - 1)]


def perpendicular_away(O, d, here, middle):
    """Unit vector perpendicular to the unit direction d, pointing from `middle` towards `here`."""
    v = np.asarray(here) - np.asarray(middle)
    return unit(O, v - d * float(O.lib().orc_dot(O.v3(v), O.v3(d))))


# ---------------------------------------------------------------- which pixels
def probe_pixels(w, h, n, seed):
    """n pixels, each a corner pixel of its 16x4 tile, no two closer than three pixels (their 3x3 neighbourhoods are
    disjoint): the four frame corners, the frame's centre pixel (both ray components exactly 0), tiles on the centre
    column and the centre row, corners of 32x32 patches, then tile corners anywhere."""
    rows = (h // PATCH) * PATCH
    rng = np.random.default_rng(seed)
    xs = [x for x in range(w) if x % TILE_W in (0, TILE_W - 1)]
    ys = [y for y in range(rows) if y % TILE_H in (0, TILE_H - 1)]
    shuffled = lambda items: [items[i] for i in rng.permutation(len(items))]
    frame_corners = [(0, 0), (w - 1, 0), (0, rows - 1), (w - 1, rows - 1)]
    centre = [(w // 2, h // 2)] if h // 2 < rows else []
    column = shuffled([(w // 2, y) for y in ys])[:2]
    row = shuffled([(x, h // 2) for x in xs])[:2] if h // 2 < rows else []
    patch_corners = shuffled([(x, y) for x in xs for y in ys if x % PATCH in (0, PATCH - 1) and y % PATCH in (0, PATCH - 1)])[:4]
    rest = shuffled([(x, y) for x in xs for y in ys])
    picked = []
    for p in frame_corners + centre + column + row + patch_corners + rest:
        if len(picked) == n:
            break
        if all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) >= 3 for q in picked):
            picked.append(p)
    assert len(picked) == n, "only %d of %d probe pixels fit a %dx%d frame" % (len(picked), n, w, h)
    return picked


# ---------------------------------------------------------------- probes on primary rays
def _on_ray(view, x, y, t):
    """-> the point at parameter t of the pixel's ray, a quarter of its distance to the nearest neighbour's point at t,
    the unit vector perpendicular to the ray that points away from the middle of the pixel's tile."""
    d = view.ray(x, y)
    c = view.eye + d * t
    spacing = min(norm(view.O, (view.eye + view.ray(*q) * t - c)) for q in view.neighbours(x, y))
    middle = sum(view.ray(*q) for q in view.tile_pixels(x, y)) * 0.25
    return d, c, 0.25 * spacing, perpendicular_away(view.O, d, d, middle)


def sphere_probe(view, x, y, t, tangent, eps=EPS):
    d, c, r, away = _on_ray(view, x, y, t)
    if tangent:
        c = c + away * (r * (1. - eps))
    return tuple(float(v) for v in c), float(r)


def triangle_probe(view, x, y, t, tangent, eps=EPS):
    """A counter-clockwise triangle in the plane z = const through the ray's point at t, circumradius r.  Centred: its
    centre is that point.  Tangent: one vertex takes the place of the sphere's rim -- the ray passes r eps inside it,
    the triangle lies away from the middle of the tile."""
    d, c, r, away = _on_ray(view, x, y, t)
    tip = np.array([0., 1., 0.])
    centre = c
    if tangent:
        a2 = unit(view.O, (away[0], away[1], 0.))
        tip = -a2
        centre = c + a2 * (r * (1. - eps))
    verts = []
    for k in range(3):
        co, si = math.cos(2. * math.pi * k / 3.), math.sin(2. * math.pi * k / 3.)
        verts.append(tuple(float(v) for v in centre + r * np.array([co * tip[0] - si * tip[1], si * tip[0] + co * tip[1], 0.])))
    return verts


def primary_recipe(view, n_spheres, n_polygons=0, n_mesh=0, seed=0, eps=EPS):
    """-> (recipe, probes): spheres, then small polygons, then one mesh of n_mesh triangles, all of them probes, and the
    two lights.  probes: one (x, y, kind, t) per primitive in recipe order, kind 'centred' or 'tangent'."""
    n = n_spheres + n_polygons + n_mesh
    pixels = probe_pixels(view.w, view.h, n, seed)
    recipe, probes, mesh = [], [], []
    for i, (x, y) in enumerate(pixels):
        k = i + seed
        tangent, t, mat = bool(k % 2), T_VALUES[(k // 2) % 3], MATERIALS[(k // 3) % len(MATERIALS)]
        if i < n_spheres:
            c, r = sphere_probe(view, x, y, t, tangent, eps)
            recipe.append(("sphere", c, r, mat))
        elif i < n_spheres + n_polygons:
            recipe.append(("polygon", triangle_probe(view, x, y, t, tangent, eps), mat))
        else:
            mesh.append([v for p in triangle_probe(view, x, y, t, tangent, eps) for v in p])
        probes.append((x, y, "tangent" if tangent else "centred", t))
    if mesh:
        recipe.append(("obj", np.array(mesh), (0., 0., 0.)))
    return recipe, probes


# ---------------------------------------------------------------- scenes from recipes
def oracle_scene(O, recipe, eye=(0., 0., 0.), lights=LIGHTS, skip=()):
    so = O.OracleScene()
    for i, item in enumerate(recipe):
        if i in skip:
            continue
        if item[0] == "sphere":
            so.add_sphere(item[1], item[2], O.reflectance(**item[3]))
        elif item[0] == "polygon":
            so.add_polygon(item[1], O.reflectance(**item[2]))
        else:
            so.add_obj(item[1], item[2])
    for pos, col, inten in lights:
        so.add_light(pos, col, inten)
    so.set_camera(eye)
    return so


def product_scene(pkg, recipe, eye=(0., 0., 0.), lights=LIGHTS):
    s, V = pkg.Scene.new(), pkg.Vec3f
    for item in recipe:
        if item[0] == "sphere":
            s.shapes.append(pkg.sphere.create(V(*item[1]), item[2], pkg.Reflectance(**item[3])))
        elif item[0] == "polygon":
            s.shapes.append(pkg.polygon.ConvexPolygon.create([V(*p) for p in item[1]], pkg.Reflectance(**item[2])))
        else:
            mesh = pkg.obj.Obj(item[1])
            mesh.offset(V(*item[2]))
            s.shapes.append(mesh)
    for pos, col, inten in lights:
        s.lights.append(pkg.create_light(V(*pos), V(*col), inten))
    s.camera = V(*eye)
    return s


def oracle_frame(O, recipe, view, depth, cam=None, skip=(), lights=LIGHTS):
    """The oracle's frame of the rendered rows of `view`."""
    so = oracle_scene(O, recipe, tuple(view.eye), lights, skip)
    if view.basis is None:
        return O.render(so, view.w, view.h, max_depth=depth)[:view.rows]
    rgb, _, _, _ = cam._rays(so, view.eye, cam.directions(view.basis, view.w, view.h), depth, True, False)
    return rgb.reshape(view.rows, view.w, 3)


# ---------------------------------------------------------------- liveness of primary probes
def live_primary(O, recipe, probes, view, depth=2, cam=None):
    """The oracle's frame with and without the probes: every probe's pixel differs, and no pixel differs that is not a
    probe's pixel or one of its 8 neighbours.  -> {kind: live count}; raises AssertionError for a dead list."""
    with_probes = oracle_frame(O, recipe, view, depth, cam)
    without = oracle_frame(O, recipe, view, depth, cam, skip=set(range(len(recipe))))
    differs = (with_probes != without).any(axis=2)
    near = np.zeros_like(differs)
    count = {"centred": 0, "tangent": 0}
    for x, y, kind, _ in probes:
        assert differs[y, x], "dead %s probe at pixel (%d, %d) of %dx%d" % (kind, x, y, view.w, view.h)
        near[max(0, y - 1):y + 2, max(0, x - 1):x + 2] = True
        count[kind] += 1
    stray = np.argwhere(differs & ~near)
    assert stray.size == 0, "pixels away from every probe differ: %s" % stray[:8].tolist()
    return count


# ---------------------------------------------------------------- child rays
def child_ray(O, shapes, n_shapes, o, d):
    """The closest hit of the ray and the one child ray the reference spawns there (optics.rs: a reflection where it is
    total, the refraction otherwise) -> (hit point, child origin, child direction) or None."""
    L = O.lib()
    is_ = O.Intersection()
    idx = C.c_uint8(0)
    if not L.orc_find_closest_intersect(O.v3(o), O.v3(d), shapes, n_shapes, C.byref(is_), C.byref(idx)):
        return None
    if not is_.reflectance.is_glass_like:
        return None
    co, cd = O.Vec3(), O.Vec3()
    if not L.orc_reflect_ray(O.v3(d), C.byref(is_), is_.reflectance.refractive_index, C.byref(co), C.byref(cd)):
        if not L.orc_refract_ray(O.v3(d), C.byref(is_), is_.reflectance.refractive_index, C.byref(co), C.byref(cd)):
            return None
    return np.array(is_.point.tup()), np.array(co.tup()), np.array(cd.tup())


def free_length(O, shapes, n_shapes, o, d, default=6.):
    """Half the way along the ray to whatever it hits first (`default` where it hits nothing)."""
    is_ = O.Intersection()
    if O.lib().orc_find_closest_intersect(O.v3(o), O.v3(d), shapes, n_shapes, C.byref(is_), None):
        return 0.5 * norm(O, (np.array(is_.point.tup()) - o))
    return default


CHILD_BASE = [
    # a floor that rises to the back (its x, y must enclose area: the inside test reads nothing else), glass of a high
    # index: seen at a grazing angle its reflection is total
    ("polygon", [(-20., -4., -5.), (20., -4., -5.), (20., -1., -45.), (-20., -1., -45.)],
     dict(diffusion=0.5, diffuse_color=(0.7, 0.7, 0.8), specular=0.6, specular_exponent=30., is_glass_like=True, reflection=0.6,
          refractive_index=3.)),
    # a sphere whose rim reflects and whose middle refracts, and a glass one of a low index
    ("sphere", (-3.5, 0.5, -12.), 2.5, dict(diffusion=0.3, diffuse_color=(0.9, 0.8, 0.7), specular=0.9, specular_exponent=20.,
                                             is_glass_like=True, reflection=0.7, refractive_index=2.5)),
    ("sphere", (3.5, 0., -11.), 2.5, dict(diffusion=0.3, diffuse_color=(0.6, 0.9, 0.9), specular=0.9, specular_exponent=20.,
                                           is_glass_like=True, reflection=0.3, refractive_index=1.3)),
]


def child_pixels(O, view, sc, seed):
    """Tile-corner pixels (a wave's corners) in a seeded order whose primary ray spawns a child ray in the base scene."""
    rng = np.random.default_rng(seed)
    cand = [(x, y) for x in range(view.w) for y in range(view.rows) if x % TILE_W in (0, TILE_W - 1) and y % TILE_H in (0, TILE_H - 1)]
    for i in rng.permutation(len(cand)):
        if child_ray(O, sc.shapes, sc.n_shapes, view.eye, view.ray(*cand[i])) is not None:
            yield cand[i]


def child_recipe(O, view, n_probes, seed, padding=0, eps=EPS, depth=4):
    """-> (recipe, probes): CHILD_BASE, `padding` small spheres out of every probe's way (the hierarchy walk needs 16), then
    n_probes probes on child rays, centred and tangent in turn, three pixels apart.  A pixel whose probe no light reaches
    (a refraction through the floor ends below it) shows nothing and is passed over.  probes: (x, y, kind, index in the recipe)."""
    base = list(CHILD_BASE)
    for k in range(padding):
        base.append(("sphere", (-13. + 2. * k, 7. + 0.25 * (k % 3), -20. - 0.5 * k), 0.6, MATERIALS[k % len(MATERIALS)]))
    so = oracle_scene(O, base, tuple(view.eye))
    sc = so.c
    recipe, probes = list(base), []
    for x, y in child_pixels(O, view, sc, seed):
        if len(probes) == n_probes:
            break
        if not all(max(abs(x - q[0]), abs(y - q[1])) >= 3 for q in probes):
            continue
        _, o2, d2 = child_ray(O, sc.shapes, sc.n_shapes, view.eye, view.ray(x, y))
        s = free_length(O, sc.shapes, sc.n_shapes, o2, d2)
        c = o2 + d2 * s
        others = [child_ray(O, sc.shapes, sc.n_shapes, view.eye, view.ray(*q)) for q in view.neighbours(x, y)]
        others = [q[1] + q[2] * s for q in others if q is not None]
        if not others:
            continue
        r = 0.25 * min([norm(O, (q - c)) for q in others] + [s])
        tangent = bool(len(probes) % 2)
        if tangent:
            c = c + perpendicular_away(O, d2, c, sum(others) / len(others)) * (r * (1. - eps))
        probe = ("sphere", tuple(float(v) for v in c), float(r), MATERIALS[len(probes) % 2 * 3])
        if _pixel(O, oracle_scene(O, base + [probe], tuple(view.eye)), view, x, y, depth) == _pixel(O, so, view, x, y, depth):
            continue
        recipe.append(probe)
        probes.append((x, y, "tangent" if tangent else "centred", len(recipe) - 1))
    assert len(probes) == n_probes
    return recipe, probes


def _hits_shape(O, sc, index, o, d):
    is_ = O.Intersection()
    return bool(O.lib().orc_shape_intersect(C.byref(sc.shapes[index]), O.v3(o), O.v3(d), C.byref(is_)))


def _pixel(O, so, view, x, y, depth):
    return O.lib().orc_cast_ray(O.v3(view.eye), O.v3(view.ray(x, y)), so.ptr, O.v3(0.1, 0.1, 0.1), 1, depth).tup()


def live_children(O, recipe, probes, view, depth=4):
    """Every probe is the first thing its pixel's child ray meets, no neighbour's child ray meets it, and the pixel's
    colour differs from the scene without that probe.  (A probe in a lit scene casts a shadow and shows in other
    reflections, so pixels elsewhere may differ as well: the rays are checked one by one instead.)"""
    so = oracle_scene(O, recipe, tuple(view.eye))
    sc = so.c
    n_base = min(p[3] for p in probes)
    base = oracle_scene(O, recipe[:n_base], tuple(view.eye))
    bc = base.c
    count = {"centred": 0, "tangent": 0}
    for x, y, kind, index in probes:
        _, o2, d2 = child_ray(O, bc.shapes, bc.n_shapes, view.eye, view.ray(x, y))
        is_, idx = O.Intersection(), C.c_uint8(255)
        hit = O.lib().orc_find_closest_intersect(O.v3(o2), O.v3(d2), sc.shapes, sc.n_shapes, C.byref(is_), C.byref(idx))
        assert hit and idx.value == index, "dead %s child probe at pixel (%d, %d): the child ray meets shape %s" % (
            kind, x, y, idx.value if hit else None)
        for q in view.neighbours(x, y):
            other = child_ray(O, bc.shapes, bc.n_shapes, view.eye, view.ray(*q))
            assert other is None or not _hits_shape(O, sc, index, other[1], other[2]), "pixel %s next to (%d, %d) meets its probe" % (q, x, y)
        without = oracle_scene(O, recipe, tuple(view.eye), skip={index})
        assert _pixel(O, so, view, x, y, depth) != _pixel(O, without, view, x, y, depth), "pixel (%d, %d) does not show its probe" % (x, y)
        count[kind] += 1
    return count


# ---------------------------------------------------------------- shadow rays
SHADOW_BASE = [
    # Receivers whose bounding spheres do NOT hold the lights (a light inside a receiver's sphere sets every bit of its
    # row, and nothing of the masks' bounds is left to test): a small floor quad -- its corners lie ON its bounding
    # sphere -- and a sphere.
    ("polygon", [(-4., -3., -12.), (4., -3., -12.), (4., -2., -20.), (-4., -2., -20.)],
     dict(diffusion=0.9, diffuse_color=(0.8, 0.8, 0.7), specular=0.4, specular_exponent=30.)),
    ("sphere", (0., 0.5, -16.), 2., dict(diffusion=0.8, diffuse_color=(0.9, 0.4, 0.3), specular=0.7, specular_exponent=30.)),
]
SHADOW_LIGHTS = [((-6., 9., -8.), (1., 1., 1.), 1.), ((9., 6., -20.), (0.6, 0.8, 1.), 0.8)]
SHADOW_KINDS = ("between", "beyond", "tangent")


def shadow_ray(O, is_, light_pos):
    """renderer.rs:163-174: the shadow ray of a hit towards a light -> origin, unit direction."""
    L = O.lib()
    light_dir = L.orc_normalized(L.orc_sub(O.v3(light_pos), is_.point))
    step = L.orc_scaled(is_.normal, 1e-3)
    o = L.orc_sub(is_.point, step) if L.orc_dot(light_dir, is_.normal) < 0. else L.orc_add(is_.point, step)
    return np.array(o.tup()), np.array(light_dir.tup())


def _receiver_hit(O, sc, view, x, y, receiver):
    is_, idx = O.Intersection(), C.c_uint8(255)
    if O.lib().orc_find_closest_intersect(O.v3(view.eye), O.v3(view.ray(x, y)), sc.shapes, sc.n_shapes, C.byref(is_), C.byref(idx)) and idx.value == receiver:
        return is_
    return None


def _shadow_candidates(O, sc, view, receiver, light):
    """The receiver's pixels whose shadow ray towards the light is free, those first whose ray runs along the EDGE of what
    the masks bound -- the hull of the receiver's bounding sphere and the light, and the cone beyond the light: for the
    quad the pixels nearest its corners (the corners lie on its bounding sphere), for the sphere the lit pixels nearest
    the terminator (light direction . normal smallest: the ray leaves along the hull's surface)."""
    pos = SHADOW_LIGHTS[light][0]
    verts = np.array(SHADOW_BASE[0][1])
    middle = verts.mean(axis=0)
    scored = []
    for y in range(view.rows):
        for x in range(view.w):
            is_ = _receiver_hit(O, sc, view, x, y, receiver)
            if is_ is None:
                continue
            o, d = shadow_ray(O, is_, pos)
            if O.lib().orc_intersect_shape_set(O.v3(o), O.v3(d), sc.shapes, sc.n_shapes):
                continue
            p = np.array(is_.point.tup())
            score = -norm(O, p - middle) if receiver == 0 else abs(float(O.lib().orc_dot(O.v3(d), is_.normal)))
            scored.append((score, x, y))
    return [(x, y) for _, x, y in sorted(scored)]


def shadow_recipe(O, view, n_probes, seed, eps=EPS):
    """-> (recipe, probes): SHADOW_BASE and n_probes probes on shadow rays of the receivers' pixels, every combination of
    receiver (quad, sphere), light and kind -- between the hit point and the light, beyond the light (the reference counts
    that as blocked), tangent to the ray -- on the pixels _shadow_candidates puts first.  probes: (x, y, kind, index in the
    recipe, light, receiver).  (`seed` is not used: the choice is by geometry.)"""
    so = oracle_scene(O, SHADOW_BASE, tuple(view.eye), SHADOW_LIGHTS)
    sc = so.c
    recipe, probes = list(SHADOW_BASE), []
    for k in range(n_probes):
        kind, light, receiver = SHADOW_KINDS[k % 3], k % 2, (k // 6) % 2
        pos = np.array(SHADOW_LIGHTS[light][0])
        for x, y in _shadow_candidates(O, sc, view, receiver, light):
            if not all(max(abs(x - q[0]), abs(y - q[1])) >= 3 for q in probes):
                continue
            o, d = shadow_ray(O, _receiver_hit(O, sc, view, x, y, receiver), pos)
            dist = norm(O, pos - o)
            s = dist * (1.5 if kind == "beyond" else 0.5)
            c = o + d * s
            others = []
            for q in view.neighbours(x, y):
                qi = _receiver_hit(O, sc, view, q[0], q[1], receiver)
                if qi is not None:
                    qo, qd = shadow_ray(O, qi, pos)
                    others.append(qo + qd * (norm(O, pos - qo) * s / dist))
            if len(others) < 3:
                continue
            r = 0.25 * min(norm(O, q - c) for q in others)
            if kind == "tangent":
                c = c + perpendicular_away(O, d, c, sum(others) / len(others)) * (r * (1. - eps))
            recipe.append(("sphere", tuple(float(v) for v in c), float(r), MATERIALS[3]))
            probes.append((x, y, kind, len(recipe) - 1, light, receiver))
            break
        else:
            raise AssertionError("no pixel for shadow probe %d" % k)
    return recipe, probes


def live_shadows(O, recipe, probes, view, depth=2):
    """Every probe blocks its pixel's shadow ray towards its light, blocks no neighbour's, and the pixel's colour differs
    from the scene without that probe."""
    so = oracle_scene(O, recipe, tuple(view.eye), SHADOW_LIGHTS)
    sc = so.c
    count = {k: 0 for k in SHADOW_KINDS}
    for x, y, kind, index, light, receiver in probes:
        is_ = _receiver_hit(O, sc, view, x, y, receiver)
        assert is_ is not None, "pixel (%d, %d) no longer sees its receiver" % (x, y)
        o, d = shadow_ray(O, is_, SHADOW_LIGHTS[light][0])
        assert _hits_shape(O, sc, index, o, d), "dead %s shadow probe at pixel (%d, %d)" % (kind, x, y)
        for q in view.neighbours(x, y):
            qi = _receiver_hit(O, sc, view, q[0], q[1], receiver)
            if qi is not None:
                qo, qd = shadow_ray(O, qi, SHADOW_LIGHTS[light][0])
                assert not _hits_shape(O, sc, index, qo, qd), "pixel %s next to (%d, %d) is shadowed by its probe" % (q, x, y)
        without = oracle_scene(O, recipe, tuple(view.eye), SHADOW_LIGHTS, skip={index})
        assert _pixel(O, so, view, x, y, depth) != _pixel(O, without, view, x, y, depth), "pixel (%d, %d) does not show its probe's shadow" % (x, y)
        count[kind] += 1
    return count


# ---------------------------------------------------------------- vertex lists the hull argument was not written for
ODD_POLYGONS = {
    # (z varies so that each has a plane of its own; the inside test reads x and y only)
    "bow_tie": [(-3., -2., -12.), (3., 2., -11.), (3., -2., -12.), (-3., 2., -11.)],
    "bow_tie_other_way": [(-3., -2., -12.), (3., -2., -12.), (-3., 2., -11.), (3., 2., -11.)],
    # a dart: counter-clockwise, reflex at its second vertex; the mean of its vertices lies on the OUTER side of the two
    # edges that meet there, and it is hit between them and the far vertex
    "dart_quad": [(-4., -4., -12.), (0., -1., -11.5), (4., -4., -12.), (0., 4., -11.)],
    "non_convex_pentagon": [(-4., -3., -12.), (4., -3., -11.), (4., 3., -10.), (0., -1., -11.5), (-4., 3., -13.)],
    "clockwise_quad": [(-3., 2., -11.), (3., 2., -11.), (3., -2., -12.), (-3., -2., -12.)],
    "twin_vertex_quad": [(-3., -2., -12.), (3., -2., -12.), (3., -2., -9.), (-3., 2., -11.)],
    "twin_vertex_first": [(3., -2., -9.), (3., -2., -12.), (0., 3., -11.), (-3., -2., -12.)],
    "same_x": [(1.5, -2., -8.), (1.5, -2., -14.), (1.5, 2., -14.), (1.5, 2., -8.)],
    "same_y": [(-3., -1.5, -8.), (3., -1.5, -8.), (3., -1.5, -14.), (-3., -1.5, -14.)],
    "convex_ccw": [(-3., -2., -12.), (3., -2., -12.), (3., 2., -11.), (-3., 2., -11.)],        # the control: this one is hit
}
ODD_MATERIAL = dict(diffusion=0.8, diffuse_color=(0.5, 0.6, 0.7), specular=0.5, specular_exponent=30., is_glass_like=True, reflection=0.4,
                    refractive_index=1.4)
ODD_OFFSET = (0.1, -0.3, 3.3)          # not representable: the moved vertices are rounded sums


def odd_recipe(name, among_spheres, as_mesh):
    verts = ODD_POLYGONS[name]
    if as_mesh:
        # the same vertex list as a fan of triangles around its first vertex, built where the offset will move it from
        back = [tuple(v[c] - ODD_OFFSET[c] for c in range(3)) for v in verts]
        tri = np.array([[c for p in (back[0], back[k], back[k + 1]) for c in p] for k in range(1, len(back) - 1)])
        recipe = [("obj", tri, ODD_OFFSET)]
    else:
        recipe = [("polygon", verts, ODD_MATERIAL)]
    if among_spheres:
        rng = np.random.default_rng(7)
        for k in range(12):
            c = (float(rng.uniform(-6., 6.)), float(rng.uniform(-4., 4.)), float(rng.uniform(-18., -6.)))
            recipe.append(("sphere", c, float(rng.uniform(0.3, 1.2)), MATERIALS[k % len(MATERIALS)]))
        # (and three small counter-clockwise triangles: the cull's edge test is compiled in from four planar primitives on)
        for k in range(3):
            x, y, z = -5. + 4. * k, 3.5 - 0.5 * k, -9. - k
            recipe.append(("polygon", [(x, y, z), (x + 1.5, y + 0.2, z - 0.5), (x + 0.6, y + 1.2, z + 0.3)], MATERIALS[k + 1]))
    return recipe


# ---------------------------------------------------------------- the lists the GPU tests use
# name -> (spheres, small polygons, triangles of one mesh): every primitive is a probe
PRIMARY_SCENES = {"poly": (10, 4, 0), "s14": (14, 0, 0), "s40": (40, 0, 0), "s60": (60, 0, 0), "s70": (70, 0, 0), "s132": (132, 0, 0),
                  "mesh12": (0, 0, 12), "mesh30": (0, 0, 30)}
SMALL_FRAMES = [(128, 96), (96, 64)]
BIG_FRAME = (512, 448)                  # 3,584 tiles: the smallest launch that classifies by the project's own rule
MOVED = (0.5, 0.25, -0.5)               # the second of a sequence's three views: the camera moved, then back
ORIENTED_EYE, ORIENTED_TURN = (0.5, 0.25, 1.), (0.3, -0.1, 0.2)      # yaw, pitch, roll
ORIENTED_SCENE = "s40"
CHILD_FRAME, CHILD_PROBES, CHILD_PADDING, CHILD_DEPTH = (128, 96), 12, 14, 4
SHADOW_FRAME, SHADOW_PROBES, SHADOW_DEPTH = (128, 96), 12, 2


def frames_for(name):
    """(132 probes, three cull steps -- the fewest that get group spheres -- do not fit the 96x64 frame three pixels apart)"""
    return [f for f in SMALL_FRAMES + [BIG_FRAME] if name != "s132" or f != (96, 64)]


def primary_case(O, name, w, h, eye=(0., 0., 0.), basis=None, cam=None, eps=EPS):
    view = View(O, w, h, eye, basis, cam)
    ns, npoly, nm = PRIMARY_SCENES[name]
    seed = 100 * sorted(PRIMARY_SCENES).index(name) + w // 32
    recipe, probes = primary_recipe(view, ns, npoly, nm, seed, eps)
    return view, recipe, probes


def oriented_basis(pkg):
    return pkg.backend.basis_turn(pkg.backend.FIXED_VIEW, *ORIENTED_TURN)


def basis_rows(b):
    return tuple((v.x, v.y, v.z) for v in (b.right, b.up, b.forward))


def oracle_camera(O, tmp_dir):
    """test_gpu_camera's oriented oracle helper around the oracle `O`, compiled into tmp_dir (the recipe of that module's
    `cam` fixture, which only pytest can call)."""
    import os
    import subprocess
    import test_gpu_camera as TC
    src, so = os.path.join(str(tmp_dir), "orc_camera.c"), os.path.join(str(tmp_dir), "orc_camera.so")
    with open(src, "w") as f:
        f.write(TC.CAMERA_C)
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-shared", "-fPIC", "-pthread",
                           "-I", os.path.dirname(os.path.abspath(O.__file__)), src, "-o", so])
    return TC.OracleCamera(O, C.CDLL(so))


def check_every_list(O, pkg, cam, eps=EPS):
    """Builds every probe list of tests/test_gpu_grazing.py and checks that it is live -> {list: {kind: live count}}."""
    counts = {}
    for name in PRIMARY_SCENES:
        for w, h in frames_for(name):
            view, recipe, probes = primary_case(O, name, w, h, eps=eps)
            counts["%s %dx%d" % (name, w, h)] = live_primary(O, recipe, probes, view)
    basis = basis_rows(oriented_basis(pkg))
    w, h = SMALL_FRAMES[0]
    view, recipe, probes = primary_case(O, ORIENTED_SCENE, w, h, ORIENTED_EYE, basis, cam, eps)
    counts["oriented %s" % ORIENTED_SCENE] = live_primary(O, recipe, probes, view, cam=cam)
    for label, view in (("child", View(O, *CHILD_FRAME)), ("oriented child", View(O, *CHILD_FRAME, eye=ORIENTED_EYE, basis=basis, cam=cam))):
        for padding in (0, CHILD_PADDING):
            recipe, probes = child_recipe(O, view, CHILD_PROBES, 5 + padding, padding, eps)
            counts["%s +%d" % (label, padding)] = live_children(O, recipe, probes, view, CHILD_DEPTH)
    view = View(O, *SHADOW_FRAME)
    recipe, probes = shadow_recipe(O, view, SHADOW_PROBES, 3, eps)
    counts["shadow"] = live_shadows(O, recipe, probes, view, SHADOW_DEPTH)
    return counts
