"""A plain model of the hierarchy walk (csrc/rm_trace.inc bvh_walk, box_hit) and the recipes of the tests that hold the walk
to the oracle where the suite never looked: directions that are admitted but not unit (|d.d - 1| < 1e-4) and trees as deep
as the builder makes them.  No GPU and no fixtures: tests/test_hierarchy_walk.py pins on the CPU that these inputs have
teeth, tests/test_gpu_hierarchy_walk.py holds the GPU to the oracle with them.

The model reads the nodes out of the host-only scene image (rmi_scene_image, as tests/test_scene_image.py does) and, for
every ray at once, gives
  reach         the primitives an UNPRUNED walk tests: a child is entered where the kernel's slab expressions say the ray
                meets its box (fused multiply-adds, the slab_rcp clamp, limit = +inf).  The kernel prunes on top, so its
                walk of the ray alone tests a subset of these.  A wave enters a child where ANY lane does: a primitive this
                walk does NOT reach for a ray is tested for that ray only where another lane of its wave drags it in.
  stack_height  the entries the near-first walk of the ray alone parks at once (both children met: the farther one waits).
  depth         inner nodes on the longest path from the root = the entries a walk can park.

Why non-unit rays bite: the reference's sphere rule (sphere.rs:27-45; tca = L.d, d2 = L.L - tca * tca, hit where d2 <= r^2)
is a geometric test for |d| = 1 only.  With d.d = 1 + e the sphere acts as one of r_eff^2 = r^2 + e * tca^2, while the
hierarchy's boxes hold the true sphere: the oracle reports hits on rays that pass outside the sphere's box."""
import numpy as np

import test_gpu_query as GQ
import test_scene_image as SI
import workloads

NODE_WORDS = 16
CLASSES = (0., 1e-9, -1e-9, 1e-6, -1e-6, 9e-5, -9e-5)            # d.d - 1 of the admitted-direction set
ADMITTED = 1e-4


# ---------------------------------------------------------------- the kernel's slab test
def _split(a):
    c = 134217729. * a                                              # Veltkamp: 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def fma(a, b, c):
    """round(a * b + c) for finite float64 arrays: the product's rounding error by Dekker's split, the sum's by two-sum.
    (Exact but for a double rounding in near-ties of the last step; where a step overflows, the plain a * b + c.)"""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    with np.errstate(all="ignore"):
        p = a * b
        ah, al = _split(a)
        bh, bl = _split(b)
        e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
        s = p + c
        v = s - p
        t = (p - (s - v)) + (c - v)
        out = s + (t + e)
        plain = p + c
    return np.where(np.isfinite(out) & np.isfinite(e) & np.isfinite(t), out, plain)


def slab_rcp(d):
    with np.errstate(divide="ignore"):
        return np.where(np.abs(d) < 1e-150, np.copysign(1e150, d), 1. / d)


class RayBox:
    def __init__(self, o, d):
        o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
        self.i = slab_rcp(d)                                        # (n, 3)
        self.a = -o * self.i
        self.n = len(o)


def box_hit(box, rb):
    """box_hit of rm_trace.inc with limit = +inf -> (met, entry distance)."""
    lo3, hi3 = np.asarray(box[:3]), np.asarray(box[3:6])
    t1, t2 = fma(lo3[None, :], rb.i, rb.a), fma(hi3[None, :], rb.i, rb.a)
    near, far = np.fmin(t1, t2), np.fmax(t1, t2)
    lo = np.fmax(np.fmax(near[:, 0], near[:, 1]), np.fmax(near[:, 2], 0.))
    hi = np.fmin(np.fmin(far[:, 0], far[:, 1]), far[:, 2])
    return ~(lo > hi), lo


# ---------------------------------------------------------------- the tree
class Tree:
    """The hierarchy of one kind ("spheres" | "triangles") of a scene image: nodes[k] = (left box, right box, left ref, right
    ref), a ref = (index, count): count 0 an inner node, else the leaf's primitives [index, index + count) of the kind."""

    def __init__(self, img, kind):
        H = img["H"]
        off = H["off_bvh_" + kind]
        assert off, "the scene image holds no hierarchy over its %s" % kind
        words = img["blob"]
        self.kind, self.count = kind, H["n_" + kind]
        self.first_pid = 0 if kind == "spheres" else H["n_spheres"] + H["n_polygons"]
        self.leaf_size = 4 if kind == "spheres" else 2
        self.nodes = {}
        todo, self.depth = [(0, 1)], 0
        covered = np.zeros(self.count, np.int64)
        while todo:
            k, level = todo.pop()
            assert k not in self.nodes
            w = words[off + NODE_WORDS * k:off + NODE_WORDS * (k + 1)]
            boxes = w[:12].view(np.float64)
            refs = w[12:14].view(np.uint32)
            left, right = (int(refs[0]), int(refs[1])), (int(refs[2]), int(refs[3]))
            self.nodes[k] = (boxes[:6].copy(), boxes[6:].copy(), left, right)
            self.depth = max(self.depth, level)
            for idx, cnt in (left, right):
                if cnt:
                    assert cnt <= self.leaf_size and idx + cnt <= self.count
                    covered[idx:idx + cnt] += 1
                else:
                    todo.append((idx, level + 1))
        assert (covered == 1).all(), "every primitive lies in exactly one leaf"

    def reach(self, o, d):
        """-> (n, count) bool: the primitives of the kind an unpruned walk tests for each ray."""
        rb = RayBox(o, d)
        out = np.zeros((rb.n, self.count), bool)
        todo = [(0, np.ones(rb.n, bool))]
        while todo:
            k, m = todo.pop()
            lbox, rbox, left, right = self.nodes[k]
            for box, (idx, cnt) in ((lbox, left), (rbox, right)):
                h = m & box_hit(box, rb)[0]
                if not h.any():
                    continue
                if cnt:
                    out[:, idx:idx + cnt] |= h[:, None]
                else:
                    todo.append((idx, h))
        return out

    def stack_height(self, o, d):
        """-> (n,) the most entries the near-first unpruned walk of each ray alone holds parked at once."""
        rb = RayBox(o, d)

        def below(ref):
            idx, cnt = ref
            return np.zeros(rb.n, np.int64) if cnt else at(idx)

        def at(k):
            lbox, rbox, left, right = self.nodes[k]
            hl, tl = box_hit(lbox, rb)
            hr, tr = box_hit(rbox, rb)
            ml, mr = below(left), below(right)
            left_first = tl <= tr
            near, far = np.where(left_first, ml, mr), np.where(left_first, mr, ml)
            return np.where(hl & hr, np.maximum(1 + near, far), np.where(hl, ml, np.where(hr, mr, 0)))

        return at(0)


def image_of(pkg, scene):
    """-> (desc, scene image with hierarchies and masks) of a product Scene; the handle stays alive on the image."""
    handle = scene.flatten()
    desc = handle.desc()
    st, img = SI.scene_image(pkg, desc, 1, 1)
    assert st == 0
    img["handle"] = handle
    return desc, img


def pid_of(img, shape, element):
    """The device primitive id of (shape, element) pairs, by the image's pid map; -1 where shape < 0."""
    back = {(int(s), int(e)): pid for pid, (s, e) in enumerate(img["pid_map"].tolist())}
    return np.array([back[(int(s), int(e))] if s >= 0 else -1 for s, e in zip(shape, element)], np.int64)


def unreached(img, o, d, pid):
    """-> bool per ray: the primitive `pid` (the oracle's closest hit; -1: none) belongs to a hierarchy of the image and the
    unpruned walk of the ray does not test it."""
    out = np.zeros(len(o), bool)
    for kind in ("spheres", "triangles"):
        if not img["H"]["off_bvh_" + kind]:
            continue
        tree = Tree(img, kind)
        k = pid - tree.first_pid
        mine = (pid >= 0) & (k >= 0) & (k < tree.count)
        if mine.any():
            reach = tree.reach(o[mine], d[mine])
            out[mine] = ~reach[np.arange(int(mine.sum())), k[mine]]
    return out


# ---------------------------------------------------------------- the suite's unit-ray sets
SCENES = ("demo", "cornell", "synthetic256", "matrix-spheres", "matrix-mesh")


def scene_pair(pkg, O, name):
    """-> (product Scene, oracle scene) of the five scenes the admitted directions are held on."""
    if name.startswith("matrix-"):
        import variant_matrix as VM
        return VM.scene_pair(pkg, O, name[len("matrix-"):], False)
    return workloads.product_scene(pkg, name), workloads.oracle_scene(O, name)


def unit_rays(name, desc):
    """The rays the suite already holds to the oracle on the scene: test_hierarchy_scenes_match_the_oracle's for the 256
    spheres, test_cornell_meshes_name_shape_and_triangle's for the box, the variant matrix's ray list for its cells."""
    lo, hi = GQ.bounds_of(desc)
    if name == "synthetic256":
        rng = np.random.default_rng(5)
        o1, d1 = GQ.random_rays(rng, 12000, lo, hi)
        o2 = GQ.inside_spheres(rng, desc, 3000)
        return np.concatenate([o1, o2, np.tile(0.5 * (lo + hi), (3000, 1))]), np.concatenate([d1, GQ.unit(rng.normal(size=(6000, 3)))])
    if name == "cornell":
        rng = np.random.default_rng(11)
        o1, d1 = GQ.random_rays(rng, 6000, lo, hi)
        tri = np.array([[[v.x, v.y, v.z] for v in desc.triangles[i].vertices] for i in range(desc.n_triangles)])
        k = rng.integers(0, len(tri), 6000)
        b = rng.dirichlet((1., 1., 1.), 6000)
        o2 = rng.uniform(lo, hi, size=(6000, 3))
        return np.concatenate([o1, o2]), np.concatenate([d1, GQ.unit((tri[k] * b[:, :, None]).sum(axis=1) - o2)])
    import variant_matrix as VM
    return VM.ray_list()


# ---------------------------------------------------------------- admitted directions
def length_squared(d):
    """The host check's expression: (x * x + y * y) + z * z in doubles."""
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def scaled_to(d, e):
    """Unit directions stretched so that d.d = 1 + e (to rounding)."""
    return GQ.unit(d) * np.sqrt(1. + e)


def _spheres_of(desc):
    c = np.array([[desc.spheres[i].center.x, desc.spheres[i].center.y, desc.spheres[i].center.z] for i in range(desc.n_spheres)])
    return c.reshape(-1, 3), np.sqrt(np.array([desc.spheres[i].radius_square for i in range(desc.n_spheres)]))


def silhouette_rays(desc, rng, n, origins):
    """n unit rays, each from one of `origins` towards a point 0.9 to 1.15 radii off the centre of a sphere, in the plane
    through the centre across the line of sight: about the silhouette, where r_eff decides."""
    c, r = _spheres_of(desc)
    o = np.asarray(origins, np.float64)[rng.integers(0, len(origins), n)]
    if not len(c):                                                  # a scene of triangles: towards points about their edges
        tri = np.array([[[v.x, v.y, v.z] for v in desc.triangles[i].vertices] for i in range(desc.n_triangles)])
        k = rng.integers(0, len(tri), n)
        b = rng.dirichlet((1., 1., 1.), n)
        b[np.arange(n), rng.integers(0, 3, n)] = rng.uniform(-0.05, 0.05, n)
        b /= b.sum(axis=1, keepdims=True)
        return o, GQ.unit((tri[k] * b[:, :, None]).sum(axis=1) - o)
    k = rng.integers(0, len(c), n)
    axis = c[k] - o
    across = GQ.unit(np.cross(axis, rng.normal(size=(n, 3))))
    aim = c[k] + across * (r[k] * rng.uniform(0.9, 1.15, n))[:, None]
    return o, GQ.unit(aim - o)


def overlap_rays(desc, rng, n, origin, e):
    """Rays from `origin` of d.d = 1 + e through the circles in which two spheres of the scene cut each other, kept where the
    reference's rule (tests/ranged_reference.py) gives the two spheres distances within 1e-4 relative: what the pruning
    distance of the one must not cut off the other.  -> (o, d), at most n, pairs in turn."""
    import ranged_reference
    c, r = _spheres_of(desc)
    pairs = [(i, j) for i in range(len(c)) for j in range(i + 1, len(c))
             if abs(r[i] - r[j]) < np.linalg.norm(c[i] - c[j]) < r[i] + r[j]]
    O_, D_ = [], []
    per = max(64, 8 * n // max(1, len(pairs)))
    for i, j in pairs:
        axis = c[j] - c[i]
        dist = np.linalg.norm(axis)
        a = (dist * dist + r[i] * r[i] - r[j] * r[j]) / (2. * dist)     # the circle's plane along the axis from c[i]
        rho = np.sqrt(max(r[i] * r[i] - a * a, 0.))
        u = GQ.unit(np.cross(axis, rng.normal(size=3)))
        v = GQ.unit(np.cross(axis, u))
        phi = rng.uniform(0., 2. * np.pi, per)
        p = c[i] + axis / dist * a + rho * (np.cos(phi)[:, None] * u + np.sin(phi)[:, None] * v)
        o = np.tile(np.asarray(origin, np.float64), (per, 1))

        def gap(s):
            """(both spheres met in front, t of i - t of j, the smaller t) aiming `s` along the axis off the circle"""
            d = scaled_to(p + s[:, None] * axis / dist - origin, e)
            ai, ti, _ = ranged_reference.Scene._sphere((c[i], r[i] * r[i]), o, d)
            aj, tj, _ = ranged_reference.Scene._sphere((c[j], r[j] * r[j]), o, d)
            with np.errstate(invalid="ignore"):
                return ai & aj & (ti > 0.) & (tj > 0.), ti - tj, np.minimum(ti, tj), d

        # a stretched ray meets the two where the circle was at distances that differ (each sphere shrinks by its own
        # e * tca^2): bisect along the axis for the aim at which they agree
        a, b = np.full(per, -0.2 * min(r[i], r[j])), np.full(per, 0.2 * min(r[i], r[j]))
        (oka, fa, _, _), (okb, fb, _, _) = gap(a), gap(b)
        with np.errstate(invalid="ignore"):
            live = oka & okb & (fa * fb < 0.)
        for _ in range(50):
            m = 0.5 * (a + b)
            okm, fm, _, _ = gap(m)
            with np.errstate(invalid="ignore"):
                left = okm & (fa * fm <= 0.)
            live &= okm
            b, fb = np.where(left, m, b), np.where(left, fm, fb)
            a, fa = np.where(left, a, m), np.where(left, fa, fm)
        okm, fm, t, d = gap(0.5 * (a + b))
        with np.errstate(invalid="ignore"):
            keep = live & okm & (np.abs(fm) < 1e-4 * t)
        O_.append(o[keep]); D_.append(d[keep])
    o, d = np.concatenate(O_ + [np.zeros((0, 3))]), np.concatenate(D_ + [np.zeros((0, 3))])
    pick = rng.permutation(len(o))[:n]
    return np.ascontiguousarray(o[pick]), np.ascontiguousarray(d[pick])


FAR_ORIGINS = {"demo": [(0., 0., 0.), (0., 0., 60.)],
               "cornell": [(0., 0., 0.), (20., 30., -50.)],
               "synthetic256": [(0., 0., 0.), (0., 0., 40.)],
               "matrix-spheres": [(0., 0., 0.), (0., 0., 60.), (30., 10., 40.)],
               "matrix-mesh": [(0., 0., 0.), (0., 0., 60.), (30., 10., 40.)]}
OVERLAP_ORIGIN = {"matrix-spheres": (0., 0., -10.), "matrix-mesh": (0., 0., -10.)}     # between two panes: the small spheres in plain sight
PER_CLASS = {9e-5: 9000}                                             # the class the model says bites; the others 1200 each
OVERLAPS = 600


QUERY_TEST_RAY = (0., 0., -1.00004)   # tests/test_gpu_query.py test_refusals: "within the assert: answered" -- from the origin; here compared


SILHOUETTE, STRETCHED, OVERLAP, QUERY = 0, 1, 2, 3                    # where a ray of an admitted set comes from


def admitted_set(name, desc, seed=20261500):
    """-> (o, d, e, kind): the admitted-direction set of the scene, at most 20,000 rays: for every class of CLASSES rays about
    the spheres' silhouettes stretched to d.d = 1 + e (SILHOUETTE), the suite's own (unit) rays of the scene stretched
    likewise in turn -- polygons and triangles are met too -- (STRETCHED), and at -9e-5 rays through the overlap of two
    spheres where the scene has any (OVERLAP).  The last ray is QUERY_TEST_RAY from the origin (QUERY).  `e` names each
    ray's class (d.d - 1), `kind` which of the four it is."""
    rng = np.random.default_rng(seed + sum(map(ord, name)))
    O_, D_, E_, K_ = [], [], [], []

    def add(o, d, e, kind):
        O_.append(o); D_.append(d); E_.append(np.full(len(o), e)); K_.append(np.full(len(o), kind))

    for e in CLASSES:
        o, d = silhouette_rays(desc, rng, PER_CLASS.get(e, 1200), FAR_ORIGINS[name])
        add(o, scaled_to(d, e), e, SILHOUETTE)
    uo, ud = unit_rays(name, desc)
    pick = rng.permutation(len(uo))[:1400]
    for k, i in enumerate(np.array_split(pick, len(CLASSES))):
        add(uo[i], scaled_to(ud[i], CLASSES[k]), CLASSES[k], STRETCHED)
    if desc.n_spheres >= 2:
        o, d = overlap_rays(desc, rng, OVERLAPS, np.array(OVERLAP_ORIGIN.get(name, FAR_ORIGINS[name][0])), -9e-5)
        add(o, d, -9e-5, OVERLAP)
    add(np.zeros((1, 3)), np.array([QUERY_TEST_RAY]), QUERY_TEST_RAY[2] ** 2 - 1., QUERY)
    o, d = np.ascontiguousarray(np.concatenate(O_)), np.ascontiguousarray(np.concatenate(D_))
    assert len(o) <= 20000 and (np.abs(length_squared(d) - 1.) < ADMITTED).all()
    return o, d, np.concatenate(E_), np.concatenate(K_)


# ---------------------------------------------------------------- chain scenes: deep trees
CHAIN_SPHERES = 100
CHAIN_TRIANGLES = 48
CHAIN_R0 = 2. ** -6
CHAIN_W = CHAIN_H = 64
CHAIN_FOV = 0.4                       # the frame's rays lie within 0.2 of the axis per unit of z: the middle rows inside every box
CHAIN_APERTURE, CHAIN_FOCUS = 0.004, 0.75
CHAIN_RADII = (0.02, 3., 1e19)        # the area lights of the soft and the converging frames, one radius a light
CHAIN_LIGHTS = [((0.5, 1., 0.25), (1., 1., 1.), 1.), ((-40., 60., 10.), (1., 0.6, 0.4), 0.7), ((3e20, 5e20, -1e20), (0.5, 0.6, 1.), 0.6)]


def _chain_material(k):
    """glass that transmits, glass that mostly reflects, opaque, in turn: a depth-6 ray tree passes through several."""
    colour = (0.2 + 0.007 * (k % 100), 0.9 - 0.007 * (k % 100), 0.5)
    if k % 3 == 0:
        return dict(diffusion=0.3, diffuse_color=colour, specular=0.9, specular_exponent=20., is_glass_like=True, reflection=0.2,
                    refractive_index=1.2)
    if k % 3 == 1:
        return dict(diffusion=0.4, diffuse_color=colour, specular=0.8, specular_exponent=8., is_glass_like=True, reflection=0.8,
                    refractive_index=1.5)
    return dict(diffusion=0.7, diffuse_color=colour, specular=0.9, specular_exponent=30., is_glass_like=False, reflection=0.,
                refractive_index=1.)


def chain_spheres(n=CHAIN_SPHERES):
    """Spheres whose radii double along the -z axis, the centre 6 radii from the origin and up to a radius off the axis: a
    surface-area split peels one off per level (rm_bvh.hpp), and seen from the origin every one of them covers the axis."""
    out, r = [], CHAIN_R0
    for k in range(n):
        out.append(((0.45 * r * (k % 3 - 1), 0.35 * r * (k % 5 - 2), -6. * r), r, k))
        r *= 2.
    return out


def chain_triangles(n=CHAIN_TRIANGLES):
    """Triangles that grow the same way (counter-clockwise in xy, facing the origin), each shifted off the axis by 0.4 of its
    size in a direction that turns with k, so that every one covers the axis and shows beside the ones in front."""
    tri, s = np.empty((n, 9)), CHAIN_R0
    for k in range(n):
        x, y, z = 0.4 * s * np.cos(2.4 * k), 0.4 * s * np.sin(2.4 * k), -6. * s
        tri[k] = [x - 1.5 * s, y - s, z, x + 1.5 * s, y - s, z - 0.25 * s * (k % 2), x, y + 1.5 * s, z + 0.125 * s * (k % 3)]
        s *= 2.
    return tri


# in front of the first triangle (z = -6), in units of CHAIN_R0: a ray down the axis passes through two glass spheres in turn
CHAIN_MESH_SPHERES = (((0.1, 0.05, -3.), 0.5), ((0., -0.2, -1.6), 0.25), ((0.3, -0.3, -9.), 0.2), ((-0.15, 0.1, -4.6), 0.6))


def chain_pair(pkg, O, which):
    """-> (product Scene -- None without pkg --, oracle scene).  "spheres": the sphere chain; "mesh": the triangle chain as
    one mesh behind four spheres of the three materials."""
    s, o = (pkg.Scene.new() if pkg is not None else None), O.OracleScene()

    def sphere(c, r, k):
        m = _chain_material(k)
        if s is not None:
            s.shapes.append(pkg.sphere.create(pkg.Vec3f(*c), r, pkg.Reflectance(**m)))
        o.add_sphere(c, r, O.reflectance(**m))

    if which == "spheres":
        for c, r, k in chain_spheres():
            sphere(c, r, k)
    else:
        assert which == "mesh"
        for k, (c, r) in enumerate(CHAIN_MESH_SPHERES):
            sphere(tuple(CHAIN_R0 * x for x in c), CHAIN_R0 * r, k)
        tri = chain_triangles()
        if s is not None:
            s.shapes.append(pkg.obj.Obj(tri))
        o.add_obj(tri)
    for pos, col, inten in CHAIN_LIGHTS:
        if s is not None:
            s.lights.append(pkg.create_light(pkg.Vec3f(*pos), pkg.Vec3f(*col), inten))
        o.add_light(pos, col, inten)
    if s is not None:
        s.camera = pkg.Vec3f(0., 0., 0.)
    o.set_camera((0., 0., 0.))
    return s, o


CHAIN_RAYS = 1100                     # 17 waves and 12 lanes


CHAIN_TOP = 60                        # the links up to which the query rays start between them
CHAIN_SHADED_TOP = 36                 # ... and the shaded rays: see chain_rays


def chain_rays(n=CHAIN_RAYS, top=CHAIN_TOP):
    """n unit rays: the first half from about the origin down the chain, within 0.12 of the axis per unit of z (inside every
    box); a quarter from points between the links in any direction; a quarter from the origin over the whole forward half.

    top: the points between the links lie at CHAIN_R0 * 2^k, k < top.  The reference starts a child or shadow ray 1e-3 of the
    normal off the hit point (renderer.rs:166-172).  Where the coordinates pass 1e12 one unit in the last place of a double is
    larger than that: the ray starts ON the surface, and whether it meets that surface again at t = +-rounding is no
    property of either implementation.  Rays that are SHADED therefore start below 2^36 * CHAIN_R0 = 1e9, where the offset is
    ten thousand units in the last place; they still walk the whole tree (the boxes of the far links hold them).  Closest
    hits and occlusion shade nothing and take the whole range."""
    rng = np.random.default_rng(20261501)
    h, q = n // 2, n // 4
    o = rng.uniform(-1e-4, 1e-4, size=(n, 3))
    d = GQ.unit(np.column_stack([rng.uniform(-0.12, 0.12, n), rng.uniform(-0.12, 0.12, n), -np.ones(n)]))
    scale = CHAIN_R0 * 2. ** rng.integers(0, top, q)
    o[h:h + q] = rng.uniform((-2., -2., -9.), (2., 2., -3.), size=(q, 3)) * scale[:, None]
    d[h:h + q] = GQ.unit(rng.normal(size=(q, 3)))
    d[h + q:] = GQ.unit(np.column_stack([rng.uniform(-1., 1., n - h - q), rng.uniform(-1., 1., n - h - q), -np.ones(n - h - q)]))
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def whole_groups(height, least, group=64):
    """How many groups of `group` consecutive rays hold `least` entries or more on every ray."""
    k = len(height) // group
    return int((height[:k * group].reshape(k, group) >= least).all(axis=1).sum())
