"""CPU checks of the device scene image (csrc/rm_image.cpp rm_build_image): header, blob and the queries' pid map of five
scenes, each built with the hierarchies and the occluder masks on, without the hierarchies, and without the masks.

Structure: every offset is even, the sections lie one behind the other inside total_words with the occluder masks behind
it, and the pid map is the permutation the keys say.  Content: one SHA-256 per section of the blob, one of the header's
field values (with the camera limits and the two verdicts) and one of the pid map, against tests/golden/scene_images.json.
That fixture was recorded from the commit BEFORE the builder moved into a unit of its own, through the same export applied
there as a throw-away patch (`RM_LIB_PATH=<that library> python tests/test_scene_image.py --record`); it is never
recorded from the code under test.  Descriptions the builder refuses come back as a status with the upload's text.

The export used here (rmi_scene_image) is not part of the ABI and needs no device."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "scene_images.json")
DODECAHEDRON = os.path.join(ROOT, "tests", "golden", "dodecahedron.obj")

SCENES = ["demo", "cornell", "dodecahedron", "synthetic256", "mixed"]
CONFIGS = {"bvh+masks": (1, 1), "flat+masks": (0, 1), "bvh": (1, 0)}        # (hierarchies, occluder masks)

HEADER_FIELDS = ["n_spheres", "n_polygons", "n_triangles", "n_lights", "off_spheres", "off_polygons", "off_pverts",
                 "off_triangles", "off_materials", "off_lights", "off_keys", "total_words", "list_ordered",
                 "off_bvh_spheres", "off_bvh_triangles", "off_bounds", "off_planar", "off_groups", "off_occ"]
INVALID_ARG = 1


def mixed_scene(pkg):
    """Both hierarchies (20 spheres, a mesh of 14 triangles), a pentagon, a wall along z (every vertex at x = 8), a dart
    and a triangle with one vertex at x = +inf; literal numbers and integer arithmetic only."""
    V, R = pkg.Vec3f, pkg.Reflectance
    s = pkg.Scene.new()
    for i in range(20):
        material = R(diffusion=0.5 + 0.025 * i, diffuse_color=(0.25 * (i % 5), 0.5, 1. - 0.125 * (i % 3)), specular=0.75,
                     specular_exponent=12.5 if i == 7 else float(10 + i), is_glass_like=(i % 6 == 0), reflection=0.125 * (i % 4),
                     refractive_index=1.5 if i % 6 == 0 else 1.)
        s.shapes.append(pkg.sphere.create(V(3. * i - 30., float(i * i % 7) - 3., -20. - 2. * i), 0.5 + 0.25 * (i % 3), material))
    s.shapes.append(pkg.polygon.ConvexPolygon.create(                                  # a pentagon in the plane z = -40
        [V(0., 6., -40.), V(-5., 2., -40.), V(-3., -4., -40.), V(3., -4., -40.), V(5., 2., -40.)], R(is_glass_like=True, refractive_index=1.25)))
    tri = np.empty((14, 9), dtype=np.float64)
    for t in range(14):
        x, y, z = -14. + 2. * t, float(t * t % 5) - 2., -30. - 1.5 * t
        tri[t] = [x, y, z, x + 1.5, y + 0.25 * (t % 3), z - 0.5, x + 0.5, y + 1.75, z + 0.25 * (t % 2)]
    s.shapes.append(pkg.obj.Obj(tri))
    s.shapes.append(pkg.polygon.ConvexPolygon.create(                                  # a wall along z: never hit
        [V(8., -2., -10.), V(8., 2., -10.), V(8., 2., -30.), V(8., -2., -30.)], R()))
    s.shapes.append(pkg.polygon.ConvexPolygon.create(                                  # a dart: reflex vertex at (0, -0.5)
        [V(0., 3., -25.), V(-2., -2., -25.), V(0., -0.5, -25.), V(2., -2., -25.)], R(is_glass_like=True, refractive_index=1.5)))
    s.shapes.append(pkg.sphere.create(V(0., 9., -15.), 1.25, R()))                     # a sphere behind the polygons in list order
    s.shapes.append(pkg.polygon.ConvexPolygon.create([V(-1., 0., -12.), V(float("inf"), 0., -12.), V(0., 1., -12.)], R()))
    s.lights.append(pkg.create_light(V(0., 0., 0.), V(1., 1., 1.), 1.))
    s.lights.append(pkg.create_light(V(20., 20., 20.), V(1., 0.5, 0.5), 0.75))
    s.lights.append(pkg.create_light(V(-6., 12., -35.), V(0.5, 1., 0.25), 0.5))
    return s


def build_scene(pkg, name):
    import workloads
    if name == "mixed":
        return mixed_scene(pkg)
    if name == "dodecahedron":
        return pkg.Scene.open_obj(DODECAHEDRON)
    return workloads.product_scene(pkg, name)


def hook(pkg):
    f = pkg.lib().rmi_scene_image
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_double),
                  C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint32), C.c_uint64]
    return f


def scene_image(pkg, desc, use_bvh, masks):
    """-> (status, image) of `desc`: header fields by name, reals, verdicts, the blob as u64 words, the pid map as [pid][2]."""
    f = hook(pkg)
    sizes, header, reals, verdicts = (C.c_uint64 * 2)(), (C.c_uint32 * 19)(), (C.c_double * 3)(), (C.c_uint32 * 2)()
    st = f(C.addressof(desc), use_bvh, masks, sizes, header, reals, verdicts, None, 0, None, 0)      # the sizes first
    if st != 0:
        return st, None
    blob, pid_map = np.zeros(sizes[0], dtype=np.uint64), np.zeros(max(sizes[1], 1), dtype=np.uint32)
    st = f(C.addressof(desc), use_bvh, masks, sizes, header, reals, verdicts, blob.ctypes.data_as(C.POINTER(C.c_uint64)), blob.size,
           pid_map.ctypes.data_as(C.POINTER(C.c_uint32)), pid_map.size)
    assert st == 0 and sizes[0] == blob.size
    return 0, dict(H=dict(zip(HEADER_FIELDS, [int(v) for v in header])), reals=np.array(reals[:], dtype=np.float64),
                   verdicts=np.array(verdicts[:], dtype=np.uint32), blob=blob, pid_map=pid_map[:sizes[1]].reshape(-1, 2))


def sections(img):
    """-> [(name, first word, words the layout gives it)] in blob order, and the (name, begin, end) slices the digests cover:
    every word of the blob belongs to exactly one slice (a section's padding, and the batch loads' tail, with it)."""
    H = img["H"]
    n = H["n_spheres"] + H["n_polygons"] + H["n_triangles"]
    planar = H["n_polygons"] + H["n_triangles"]
    n_pverts = None                                       # (the vertex count is not in the header: the section ends where the next begins)
    nominal = [("spheres", H["off_spheres"], 4 * H["n_spheres"]), ("polygons", H["off_polygons"], 16 * H["n_polygons"]),
               ("pverts", H["off_pverts"], n_pverts), ("triangles", H["off_triangles"], 12 * H["n_triangles"]),
               ("materials", H["off_materials"], 10 * n), ("lights", H["off_lights"], 8 * H["n_lights"]),
               ("keys", H["off_keys"], (n + 1) // 2), ("bounds", H["off_bounds"], 4 * n), ("planar", H["off_planar"], 16 * planar)]
    for name, words in (("groups", 4 * ((n + 63) // 64)), ("bvh_spheres", None), ("bvh_triangles", None)):
        if H["off_" + name]:
            nominal.append((name, H["off_" + name], words))
    ends = [first for _, first, _ in nominal[1:]] + [H["total_words"] - 64]
    slices = [(name, first, end) for (name, first, _), end in zip(nominal, ends)]
    slices.append(("tail", H["total_words"] - 64, H["total_words"]))
    if H["off_occ"]:
        slices.append(("occ", H["off_occ"], img["blob"].size))
    return nominal, slices


def digests(img):
    _, slices = sections(img)
    out = {name: hashlib.sha256(img["blob"][b:e].tobytes()).hexdigest() for name, b, e in slices}
    head = np.array([img["H"][k] for k in HEADER_FIELDS], dtype=np.uint32).tobytes() + img["reals"].tobytes() + img["verdicts"].tobytes()
    out["header"] = hashlib.sha256(head).hexdigest()
    out["pid_map"] = hashlib.sha256(np.ascontiguousarray(img["pid_map"]).tobytes()).hexdigest()
    return out


def check_structure(img, desc, use_bvh, masks, label):
    H, blob = img["H"], img["blob"]
    n = H["n_spheres"] + H["n_polygons"] + H["n_triangles"]
    for k in HEADER_FIELDS:
        if k.startswith("off_") or k == "total_words":
            assert H[k] % 2 == 0, (label, k, H[k])
    nominal, slices = sections(img)
    assert nominal[0][1] == 0, label
    for (name, first, words), (_, b, e) in zip(nominal, slices):
        assert first == b <= e <= H["total_words"] - 64, (label, name)
        if words is None:
            assert (e - b) % 16 == 0 and e > b if name.startswith("bvh") else e - b >= 2, (label, name)
        else:
            assert e - b in (words, words + 1), (label, name, words, e - b)         # its words, rounded up to an even count
    assert H["n_lights"] == desc.n_lights, label
    if not use_bvh:
        assert H["off_bvh_spheres"] == 0 and H["off_bvh_triangles"] == 0, label
    if H["off_occ"]:
        assert masks and 0 < n <= 64 and H["off_occ"] == H["total_words"], label
        assert blob.size == H["total_words"] + ((n * H["n_lights"] + 1) & ~1), label
    else:
        assert blob.size == max(H["total_words"], 2) and img["reals"][1] == 0., label
        assert not (masks and 0 < n <= 64 and H["n_lights"] > 0), label
    # the keys: each pid's ordinal in the flattened shape list; the pid map: the same way back, (shape, element)
    keys = blob[H["off_keys"]:H["off_keys"] + (n + 1) // 2].view(np.uint32)[:n]
    flat, kinds = [], []
    for i in range(desc.n_shapes):
        ref = desc.shapes[i]
        flat += [(i, t) for t in range(ref.count if ref.kind == 2 else 1)]
        kinds += [ref.kind] * (ref.count if ref.kind == 2 else 1)
    assert sorted(keys.tolist()) == list(range(len(flat))) and n == len(flat), label
    assert H["list_ordered"] == (1 if keys.tolist() == sorted(keys.tolist()) else 0), label
    assert img["pid_map"].shape == (n, 2), label
    assert [tuple(r) for r in img["pid_map"].tolist()] == [flat[k] for k in keys.tolist()], label
    assert [kinds[k] for k in keys.tolist()] == [0] * H["n_spheres"] + [1] * H["n_polygons"] + [2] * H["n_triangles"], label


@pytest.fixture(scope="module")
def expected():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", SCENES)
def test_image_is_the_recorded_one(pkg, expected, name, config):
    use_bvh, masks = CONFIGS[config]
    handle = build_scene(pkg, name).flatten()
    desc = handle.desc()
    st, img = scene_image(pkg, desc, use_bvh, masks)
    assert st == 0, (name, config, pkg.lib().rm_last_error(None))
    check_structure(img, desc, use_bvh, masks, (name, config))
    got, want = digests(img), expected[name][config]
    assert sorted(got) == sorted(want), (name, config)
    for section in sorted(want):
        assert got[section] == want[section], "scene %s (%s): section %s differs from the recorded image" % (name, config, section)


def test_mixed_scene_takes_every_path(pkg):
    """What the mixed scene is there for: both hierarchies, a polygon without an edge record (five vertices), one that is
    never hit (radius -1), a dart (bounds, no edge record), an unbounded primitive, a fractional exponent."""
    desc = mixed_scene(pkg).flatten().desc()
    _, img = scene_image(pkg, desc, 1, 1)
    H = img["H"]
    assert (H["n_spheres"], H["n_polygons"], H["n_triangles"], H["n_lights"]) == (21, 4, 14, 3)
    assert H["off_bvh_spheres"] and H["off_bvh_triangles"] and H["off_occ"] and not H["list_ordered"]
    words = img["blob"].view(np.float64)
    radius = words[H["off_bounds"] + 3:H["off_bounds"] + 4 * 39:4]
    count = words[H["off_planar"] + 12:H["off_planar"] + 16 * 18:16]
    by_shape = {int(img["pid_map"][pid][0]): pid for pid in range(21, 25)}
    pentagon, wall, dart, open_tri = (by_shape[s] for s in (20, 22, 23, 25))
    assert radius[pentagon] > 0. and count[pentagon - 21] == 0.
    assert radius[wall] == -1.
    assert np.isfinite(radius[dart]) and radius[dart] > 0. and count[dart - 21] == 0.
    assert radius[open_tri] == np.inf and count[open_tri - 21] == 0.
    assert (count[4:] == 3.).all()
    assert img["verdicts"].tolist() == [1, 0]             # exact only (the infinite vertex); an exponent of 12.5


def _desc(pkg, shapes, n_spheres=1, n_polygons=1, n_vertices=3, n_triangles=1, polygon=(0, 3)):
    L = pkg._lib
    d = L.rm_scene_desc()
    keep = [(L.rm_shape_ref * len(shapes))(*[L.rm_shape_ref(*s) for s in shapes]), (L.rm_sphere * 1)(), (L.rm_polygon * 1)(),
            (L.rm_vec3 * 3)(L.rm_vec3(0., 0., -5.), L.rm_vec3(1., 0., -5.), L.rm_vec3(0., 1., -5.)), (L.rm_triangle * 1)(), (L.rm_light * 1)()]
    keep[2][0].first_vertex, keep[2][0].n_vertices = polygon
    d.shapes, d.n_shapes = keep[0], len(shapes)
    d.spheres, d.n_spheres = keep[1], n_spheres
    d.polygons, d.n_polygons = keep[2], n_polygons
    d.polygon_vertices, d.n_polygon_vertices = keep[3], n_vertices
    d.triangles, d.n_triangles = keep[4], n_triangles
    d.lights, d.n_lights = keep[5], 1
    d._keep = keep
    return d


REFUSALS = [
    ("sphere ref past the array", dict(shapes=[(0, 1, 1)]), "rm_scene_upload: bad sphere ref"),
    ("sphere ref of two", dict(shapes=[(0, 0, 2)]), "rm_scene_upload: bad sphere ref"),
    ("polygon ref past the array", dict(shapes=[(1, 4, 1)]), "rm_scene_upload: bad polygon ref"),
    ("polygon ref of none", dict(shapes=[(1, 0, 0)]), "rm_scene_upload: bad polygon ref"),
    ("mesh ref past the array", dict(shapes=[(0, 0, 1), (2, 1, 1)]), "rm_scene_upload: bad mesh ref"),
    ("mesh ref that wraps", dict(shapes=[(2, 0xFFFFFFFF, 2)]), "rm_scene_upload: bad mesh ref"),
    ("unknown kind", dict(shapes=[(0, 0, 1), (7, 0, 1)]), "rm_scene_upload: unknown shape kind"),
    ("polygon of two vertices", dict(shapes=[(1, 0, 1)], polygon=(0, 2)), "rm_scene_upload: bad polygon vertex range"),
    ("polygon vertices past the array", dict(shapes=[(1, 0, 1)], polygon=(1, 3)), "rm_scene_upload: bad polygon vertex range"),
    ("polygon vertex range that wraps", dict(shapes=[(1, 0, 1)], polygon=(0xFFFFFFFF, 3)), "rm_scene_upload: bad polygon vertex range"),
]


@pytest.mark.parametrize("label,kw,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_back_as_a_status(pkg, label, kw, text):
    for use_bvh, masks in CONFIGS.values():
        st, _ = scene_image(pkg, _desc(pkg, **kw), use_bvh, masks)
        assert st == INVALID_ARG and pkg.lib().rm_last_error(None).decode() == text, label


@pytest.mark.parametrize("array", ["shapes", "spheres", "polygons", "polygon_vertices", "triangles", "lights"])
def test_null_array_with_a_count_is_refused_by_every_hook(pkg, array):
    text = "rm_scene_upload: NULL array with non-zero count"
    d = _desc(pkg, [(0, 0, 1), (1, 0, 1), (2, 0, 1)])
    setattr(d, array, None)
    assert scene_image(pkg, d, 1, 1)[0] == INVALID_ARG and pkg.lib().rm_last_error(None).decode() == text
    L = pkg.lib()
    dims = (C.c_uint32 * 3)()
    for f, args in ((L.rmi_shadow_masks, (None, None, C.c_uint32(0), dims)),
                    (L.rmi_empty_sides, (None, None, None, C.c_uint32(0), dims, None)),
                    (L.rmi_upload_numerics, (None, C.c_uint32(0), dims))):
        f.restype, f.argtypes = C.c_int, None
        assert f(C.c_void_p(C.addressof(d)), *args) == INVALID_ARG and L.rm_last_error(None).decode() == text, array
    st, img = scene_image(pkg, _desc(pkg, [(0, 0, 1), (1, 0, 1), (2, 0, 1)]), 1, 1)      # (the description itself is a good one)
    assert st == 0 and img["H"]["n_spheres"] == img["H"]["n_polygons"] == img["H"]["n_triangles"] == 1


def test_null_arguments_are_refused(pkg):
    f = hook(pkg)
    sizes = (C.c_uint64 * 2)()
    assert f(None, 1, 1, sizes, None, None, None, None, 0, None, 0) == INVALID_ARG
    assert pkg.lib().rm_last_error(None).decode() == "rmi_scene_image: NULL argument"


if __name__ == "__main__":                                # --record: write the fixture from the library RM_LIB_PATH names
    assert sys.argv[1:] == ["--record"] and os.environ.get("RM_LIB_PATH"), "RM_LIB_PATH=<the parent's library> ... --record"
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    package = G.load_package()
    recorded = {}
    for scene_name in SCENES:
        recorded[scene_name] = {}
        for config_name, (bvh, occ) in CONFIGS.items():
            status, image = scene_image(package, build_scene(package, scene_name).flatten().desc(), bvh, occ)
            assert status == 0
            recorded[scene_name][config_name] = digests(image)
    with open(FIXTURE, "w") as out:
        json.dump(recorded, out, indent=1, sort_keys=True)
        out.write("\n")
    print("recorded %s from %s" % (FIXTURE, package._lib.LIB_PATH))
