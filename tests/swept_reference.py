"""The yardstick of the swept hierarchies' tests (include/rusty_marcher_amd.h, "swept hierarchies").  No GPU.

A swept hierarchy is the scene image with the boxes of its hierarchies refitted (csrc/rm_swept_image.cpp).  Here: the hook that
builds one on the CPU (rmi_swept_image), the two scenes whose last leaf in device order is partial, the per-primitive boxes in
numpy (the builder's: a sphere's centre -+ sqrt(r^2) (1 + 1e-12), a triangle's vertices' minimum and maximum, at record + off),
random extents, and the moved scene of tests/ranged_reference.py for the walk model.  tests/test_swept_abi.py pins the refit on
these; tests/test_gpu_swept.py and tests/test_gpu_converge_swept.py hold the GPU to the flat passes and to tests/moving_reference.py."""
import ctypes as C

import numpy as np

import hierarchy_reference as HR
import moving_reference as MV
import ranged_reference
import workloads

# every scene the tests walk: a sphere hierarchy (matrix-spheres, synthetic256, chain-spheres, seventeen), a triangle hierarchy
# (matrix-mesh, cornell, dodecahedron, chain-mesh, thirteen), none at all (demo, pool)
SCENES = ("matrix-spheres", "matrix-mesh", "cornell", "dodecahedron", "pool", "chain-spheres", "chain-mesh", "demo", "seventeen", "thirteen")
HIERARCHY = {"matrix-spheres": "spheres", "synthetic256": "spheres", "chain-spheres": "spheres", "seventeen": "spheres",
             "matrix-mesh": "triangles", "cornell": "triangles", "dodecahedron": "triangles", "chain-mesh": "triangles", "thirteen": "triangles"}
INVALID_ARG = 1

SMALL_LIGHTS = [((2., 6., 2.), (1., 1., 1.), 1.), ((-6., 3., -2.), (0.9, 0.7, 0.5), 0.6)]
_OPAQUE = dict(diffusion=0.8, diffuse_color=(0.8, 0.5, 0.3), specular=0.6, specular_exponent=20., is_glass_like=False, reflection=0.,
               refractive_index=1.)
_GLASS = dict(diffusion=0.3, diffuse_color=(0.6, 0.8, 0.9), specular=0.8, specular_exponent=30., is_glass_like=True, reflection=0.3,
              refractive_index=1.5)


def seventeen_spheres():
    """17 spheres and nothing else: a 4 x 4 grid in the plane z = -12 and one sphere far to the right, which the first split
    peels off into a leaf of its own -- the last in device order, with one primitive of four."""
    out = [((-4.5 + 3. * (k % 4), -4.5 + 3. * (k // 4), -12. - 0.25 * (k % 3)), 1. + 0.125 * (k % 2)) for k in range(16)]
    return out + [((30., 0., -14.), 1.5)]


def thirteen_triangles():
    """A single mesh of 13 triangles, counter-clockwise in xy: twelve in a 4 x 3 grid about z = -10 and one far to the right."""
    tri = []
    for k in range(12):
        x, y, z = -5. + 2.5 * (k % 4), -3.5 + 2.5 * (k // 4), -10. - 0.5 * (k % 3)
        tri.append([x, y, z, x + 2., y + 0.25, z - 0.25, x + 0.5, y + 2., z + 0.25])
    tri.append([28., -1., -12., 31., -1., -12.5, 29., 2., -12.])
    return np.array(tri)


def small_pair(pkg, O, name):
    s, o = (pkg.Scene.new() if pkg is not None else None), O.OracleScene()
    if name == "seventeen":
        for k, (c, r) in enumerate(seventeen_spheres()):
            m = _GLASS if k % 5 == 0 else dict(_OPAQUE, diffuse_color=(0.2 + 0.04 * k, 0.9 - 0.04 * k, 0.5))
            if s is not None:
                s.shapes.append(pkg.sphere.create(pkg.Vec3f(*c), r, pkg.Reflectance(**m)))
            o.add_sphere(c, r, O.reflectance(**m))
    else:
        assert name == "thirteen"
        tri = thirteen_triangles()
        if s is not None:
            s.shapes.append(pkg.obj.Obj(tri))
        o.add_obj(tri)
    for pos, col, inten in SMALL_LIGHTS:
        if s is not None:
            s.lights.append(pkg.create_light(pkg.Vec3f(*pos), pkg.Vec3f(*col), inten))
        o.add_light(pos, col, inten)
    if s is not None:
        s.camera = pkg.Vec3f(0., 0., 0.)
    o.set_camera((0., 0., 0.))
    return s, o


def scene_pair(pkg, O, name):
    """-> (product Scene, oracle scene) of any scene of SCENES, and of synthetic256."""
    if name in ("seventeen", "thirteen"):
        return small_pair(pkg, O, name)
    if name.startswith("chain-"):
        return HR.chain_pair(pkg, O, name[len("chain-"):])
    if name.startswith("matrix-"):
        return HR.scene_pair(pkg, O, name)
    if name == "pool":
        return MV.pool_scenes(pkg, O)
    if name == "dodecahedron":
        return MV.dodecahedron_scenes(pkg, O)
    return workloads.product_scene(pkg, name), workloads.oracle_scene(O, name)


# ---------------------------------------------------------------- the refit, on the CPU
def hook(pkg):
    f = pkg.lib().rmi_swept_image
    f.restype = C.c_int
    D = C.POINTER(C.c_double)
    f.argtypes = [C.c_void_p, C.c_uint32, D, D, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint64]
    return f


def swept_image(pkg, desc, lo, hi, use_bvh=1, n_shapes=None):
    """-> (status, the swept blob of `desc`'s image as u64 words -- None where refused)."""
    f = hook(pkg)
    lo, hi = np.ascontiguousarray(lo, np.float64), np.ascontiguousarray(hi, np.float64)
    n = lo.shape[0] if n_shapes is None else n_shapes
    D = C.POINTER(C.c_double)
    words = C.c_uint64(0)
    st = f(C.addressof(desc), use_bvh, lo.ctypes.data_as(D), hi.ctypes.data_as(D), n, C.byref(words), None, 0)
    if st != 0:
        return st, None
    blob = np.zeros(words.value, dtype=np.uint64)
    st = f(C.addressof(desc), use_bvh, lo.ctypes.data_as(D), hi.ctypes.data_as(D), n, C.byref(words), blob.ctypes.data_as(C.POINTER(C.c_uint64)), blob.size)
    assert st == 0 and words.value == blob.size
    return 0, blob


def swept_of(img, blob):
    """The image with the swept blob in place of its own: what hierarchy_reference.Tree reads."""
    out = dict(img)
    out["blob"] = blob
    return out


def node_words(img):
    """-> (every word of a node of either hierarchy, the box words among them): index arrays into the blob."""
    nodes, boxes = [], []
    for kind in ("spheres", "triangles"):
        off = img["H"]["off_bvh_" + kind]
        if off:
            for k in HR.Tree(img, kind).nodes:
                nodes.extend(range(off + HR.NODE_WORDS * k, off + HR.NODE_WORDS * (k + 1)))
                boxes.extend(range(off + HR.NODE_WORDS * k, off + HR.NODE_WORDS * k + 12))
    return np.array(sorted(nodes), np.int64), np.array(sorted(boxes), np.int64)


def last_leaf(tree):
    """-> (first, count) of the leaf that holds the last primitive in device order."""
    for _, _, left, right in tree.nodes.values():
        for idx, cnt in (left, right):
            if cnt and idx + cnt == tree.count:
                return idx, cnt
    raise AssertionError("no leaf ends the device order")


def primitive_boxes(desc, img, kind, offsets):
    """(count, 6): lo xyz, hi xyz of every primitive of the kind in device order with shape k moved by offsets[k] -- the
    builder's own box (csrc/rm_image.cpp build_hierarchies) at record + offset, one addition a component."""
    H = img["H"]
    first = 0 if kind == "spheres" else H["n_spheres"] + H["n_polygons"]
    out = np.empty((H["n_" + kind], 6))
    offsets = np.asarray(offsets, np.float64)
    for j in range(H["n_" + kind]):
        shape, element = (int(x) for x in img["pid_map"][first + j])
        ref = desc.shapes[shape]
        if kind == "spheres":
            s = desc.spheres[ref.first]
            c = np.array([s.center.x, s.center.y, s.center.z]) + offsets[shape]
            r = np.sqrt(np.float64(s.radius_square)) * (1. + 1e-12)
            out[j] = np.concatenate([c - r, c + r])
        else:
            t = desc.triangles[ref.first + element]
            v = np.array([[p.x, p.y, p.z] for p in t.vertices]) + offsets[shape]
            out[j] = np.concatenate([v.min(axis=0), v.max(axis=0)])
    return out


def random_extents(rng, n_shapes, scale):
    """lo <= 0 <= hi per shape and component, by (3 k + 1) % 4: one-sided below, zero, two-sided and one-sided above in turn
    from shape 0 (the lone mesh of a scene moves; so does shape 11, the matrix's); every seventh a hundred times as large."""
    lo, hi = -rng.uniform(0., scale, (n_shapes, 3)), rng.uniform(0., scale, (n_shapes, 3))
    for k in range(n_shapes):
        c = (3 * k + 1) % 4
        if c == 0:
            lo[k] = hi[k] = 0.
        elif c == 1:
            hi[k] = 0.
        elif c == 2:
            lo[k] = 0.
        if k % 7 == 2:
            lo[k] *= 100.
            hi[k] *= 100.
    return lo, hi


def rows_within(rng, lo, hi, rows):
    """`rows` rows of a shape offset table within the extents: the two corners first, then uniform."""
    out = rng.uniform(lo, hi, (rows,) + lo.shape)
    out[0], out[1] = lo, hi
    return out


def scale_of(desc):
    """A length of the scene's own: a tenth of the median extent of its sphere centres and triangle vertices."""
    pts = [[desc.spheres[i].center.x, desc.spheres[i].center.y, desc.spheres[i].center.z] for i in range(desc.n_spheres)]
    pts += [[v.x, v.y, v.z] for i in range(desc.n_triangles) for v in desc.triangles[i].vertices]
    pts = np.array(pts)
    return 0.1 * float(np.median(np.abs(pts - np.median(pts, axis=0)))) if len(pts) else 1.


class MovedRanged(ranged_reference.Scene):
    """tests/ranged_reference.py's Scene with shape k moved by row[k]: a sphere's centre, a planar primitive's plane point and
    vertices, one addition a component; normals stay (as moving_reference.MovedScene moves the oracle's)."""

    def __init__(self, desc, row):
        super().__init__(desc)
        row = np.asarray(row, np.float64)
        moved = []
        for kind, si, el, data in self.prims:
            if kind == "sphere":
                moved.append((kind, si, el, (data[0] + row[si], data[1])))
            else:
                n, pp, verts, eps = data
                moved.append((kind, si, el, (n, pp + row[si], verts + row[si], eps)))
        self.prims = moved
