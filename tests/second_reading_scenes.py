"""Scenes as plain data, and the three builders that turn one description into the second reading's scene
(tests/second_reading.py), the oracle's and the product's -- each through its own constructors.  Used by
tests/test_second_reading.py (CPU) and tests/test_gpu_second_reading.py (GPU).

A description is the dict tests/test_gpu_parity.py::fuzz_recipe returns: shapes = [("sphere", centre, radius, material) |
("polygon", vertices, material) | ("mesh", triangles of 9 numbers, offset[, "f32"])] in scene order, lights = [(position,
colour, intensity)], camera.  {"default": True} stands for each side's own create_default (scene.rs:28-211).  A mesh marked
"f32" came out of an .obj file: its numbers are f32 values and the second reading widens them itself (obj.rs:103-105).

This module is imported by the worker processes that render the second reading's frames, so it imports nothing heavy at
module level: numpy, the oracle and the package are touched only inside the builders that need them."""
import os

import second_reading as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

OBJ_OFFSET = (0., 0., -500.)                                                            # main.rs:278-282
OBJ_LIGHTS = [((0., 0., 0.), (1., 1., 1.), 1.), ((20., 20., 20.), (1., 0.5, 0.5), 0.8)]  # main.rs:293-315

# the three cameras of the frame tests: the reference's own, a fractional one away from it, and one INSIDE the demo's blue
# glass sphere (centre (-0.5, -1.5, -5), radius 2: scene.rs:126-134), 1.7 from its centre -- close enough to the surface that
# rays near the frame's edge meet it from within beyond the critical angle (asin(1 / 1.5) = 41.8 degrees)
CAMERAS = {"origin": (0., 0., 0.), "off": (0.37, 1.21, 2.6), "inside": (1.2, -1.4, -4.9)}
# The .obj scenes stand 500 back (main.rs:278-282) under lights at and near the origin: seen from there every visible point is
# lit.  Their fractional camera is therefore one that sees shadows: inside the Cornell box (which spans x 0..556, y 0..549,
# z -500..59.2) in front of its two blocks, and well to the side of the dodecahedron (radius 100 about (0, 0, -500)).
OBJ_CAMERAS = {"cornell": dict(CAMERAS, off=(278.5, 273.25, -10.5)), "dodecahedron": dict(CAMERAS, off=(200.5, 0.25, -250.5))}


def cameras_of(name):
    return OBJ_CAMERAS.get(name, CAMERAS)


def plain(x):
    """numbers, tuples, lists and arrays -> nested lists of Python floats (cheap to hand to another process)"""
    if hasattr(x, "tolist"):
        return x.tolist()
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return x


def obj_description(filename):
    """main.rs:261-327: every model of the file one Obj, moved back by 500, under the two demo lights."""
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import obj_oracle
    shapes = [("mesh", [list(t) for t in tris], OBJ_OFFSET, "f32") for _, tris in obj_oracle.load_models(os.path.join(GOLDEN, filename))]
    return dict(shapes=shapes, lights=list(OBJ_LIGHTS), camera=(0., 0., 0.))


GLASS = dict(diffusion=0.3, diffuse_color=(0.9, 0.8, 0.7), specular=0.9, specular_exponent=20.,
             is_glass_like=True, reflection=0.4, refractive_index=1.5)
MATT = dict(diffusion=0.9, diffuse_color=(0.7, 0.4, 0.2), specular=0.5, specular_exponent=12.5,
            is_glass_like=False, reflection=0.3, refractive_index=1.)


def _ngon(n, centre, radius, tilt, phase=0.1):
    """n vertices, counter-clockwise in xy around `centre`, near the plane z = cz + tilt . (x - cx, y - cy): every coordinate
    is rounded to a multiple of 1/64, so the scene does not depend on the last bit of anybody's cos (and is planar only
    nearly, which polygon.rs never asks for)."""
    import math
    out = []
    for k in range(n):
        a = phase + 2. * math.pi * k / n
        dx, dy = radius * math.cos(a), radius * math.sin(a)
        out.append(tuple(round(64. * v) / 64. for v in (centre[0] + dx, centre[1] + dy, centre[2] + tilt[0] * dx + tilt[1] * dy)))
    return out


def manygons_description():
    """Polygons of 5 to 8 vertices, every second one glass.  A matt octagon closes the back; in front of it stand a pentagon,
    a hexagon and a heptagon that face the camera, and left and right of the view two glass polygons tilted so steeply
    (normal about 60 degrees off the view axis) that rays near the frame's edge meet them FROM BEHIND at grazing incidence:
    refract_ray's total internal reflection (optics.rs:74).  The glass heptagon's refracted children meet the octagon."""
    shapes = [
        ("polygon", _ngon(5, (-3., 1.5, -12.), 3., (0.2, -0.1)), GLASS),
        ("polygon", _ngon(6, (3.5, -1., -14.), 3.5, (-0.3, 0.25)), MATT),
        ("polygon", _ngon(7, (0.5, -3., -9.), 2.5, (0.1, 0.5)), dict(GLASS, refractive_index=1.33, reflection=0.25)),
        ("polygon", _ngon(8, (0., 0., -25.), 22., (0.05, -0.05)), MATT),
        ("polygon", _ngon(6, (7., 0.5, -8.), 2.5, (-1.8, 0.1)), GLASS),
        ("polygon", _ngon(8, (-7., -0.5, -8.), 2.5, (1.7, -0.2)), dict(GLASS, refractive_index=1.7)),
        ("polygon", _ngon(5, (1., 4., -11.), 2., (0., -0.4)), dict(MATT, diffuse_color=(0.2, 0.6, 0.9))),
    ]
    lights = [((0., 6., 0.), (1., 1., 1.), 1.), ((-10., 2., -4.), (0.4, 0.8, 1.), 0.7)]
    return dict(shapes=shapes, lights=lights, camera=(0., 0., 0.))


# ---------------------------------------------------------------- the builders
def second_scene(desc, camera=None):
    if desc.get("default"):
        scene = S.Scene.create_default()
    else:
        scene = S.Scene()
        for shape in desc["shapes"]:
            if shape[0] == "sphere":
                _, c, r, m = shape
                scene.shapes.append(S.Sphere(tuple(float(v) for v in c), float(r), _second_material(m)))
            elif shape[0] == "polygon":
                _, verts, m = shape
                scene.shapes.append(S.ConvexPolygon([tuple(float(x) for x in v) for v in verts], _second_material(m)))
            else:
                tris, off = shape[1], shape[2]
                positions = [float(x) for t in tris for x in t]
                mesh = S.Obj(positions, list(range(len(positions) // 3)),
                             widen=S.widen_f32 if len(shape) > 3 and shape[3] == "f32" else float)
                mesh.offset(tuple(float(v) for v in off))
                scene.shapes.append(mesh)
        for pos, col, inten in desc["lights"]:
            scene.lights.append(S.Light(tuple(float(v) for v in pos), tuple(float(v) for v in col), float(inten)))
        scene.camera = tuple(float(v) for v in desc["camera"])
    for index, off in sorted(desc.get("moves", {}).items()):
        scene.shapes[index].offset(tuple(float(v) for v in off))       # polygon.rs:44-49, obj.rs:24-29
    if camera is not None:
        scene.camera = S.ZERO
        scene.offset_camera(tuple(float(v) for v in camera))           # scene.rs:25-27, from the origin
    return scene


def _second_material(m):
    return S.Reflectance(diffusion=float(m["diffusion"]), diffuse_color=tuple(float(v) for v in m["diffuse_color"]),
                         specular=float(m["specular"]), specular_exponent=float(m["specular_exponent"]),
                         is_glass_like=bool(m["is_glass_like"]), reflection=float(m["reflection"]),
                         refractive_index=float(m["refractive_index"]))


def oracle_scene(O, desc, camera=None):
    import numpy as np
    if desc.get("default"):
        so = O.OracleScene.create_default()
    else:
        so = O.OracleScene()
        for shape in desc["shapes"]:
            if shape[0] == "sphere":
                so.add_sphere(shape[1], shape[2], O.reflectance(**shape[3]))
            elif shape[0] == "polygon":
                so.add_polygon(shape[1], O.reflectance(**shape[2]))
            else:
                so.add_obj(np.array(shape[1], dtype=np.float64), shape[2])
        for pos, col, inten in desc["lights"]:
            so.add_light(pos, col, inten)
        so.set_camera(desc["camera"])
    for index, off in sorted(desc.get("moves", {}).items()):
        oracle_move(O, so, index, off)
    if camera is not None:
        so.set_camera(camera)
    return so


def oracle_move(O, so, index, off):
    """The oracle has orc_triangle_offset and no other: a mesh is moved by it, triangle by triangle (obj.rs:24-29); a polygon
    the way tests/moving_reference.py moves one, plane_point and every vertex through orc_add, the normal left alone."""
    import ctypes as C
    L, shape, o = O.lib(), so.ptr.contents.shapes[index], O.v3(off)
    if shape.kind == 2:
        for t in range(shape.n_triangles):
            L.orc_triangle_offset(C.byref(shape.triangles[t]), o)
    elif shape.kind == 1:
        shape.plane_point = L.orc_add(shape.plane_point, o)
        for k in range(shape.n_vertices):
            shape.vertices[k] = L.orc_add(shape.vertices[k], o)
    else:
        raise ValueError("sphere.rs has no offset()")


def product_scene(pkg, desc, camera=None):
    import numpy as np
    V = pkg.Vec3f
    if desc.get("default"):
        s = pkg.Scene.create_default()
    else:
        s = pkg.Scene.new()
        for shape in desc["shapes"]:
            if shape[0] == "sphere":
                s.shapes.append(pkg.sphere.create(V(*shape[1]), shape[2], pkg.Reflectance(**shape[3])))
            elif shape[0] == "polygon":
                s.shapes.append(pkg.polygon.ConvexPolygon.create([V(*v) for v in shape[1]], pkg.Reflectance(**shape[2])))
            else:
                mesh = pkg.obj.Obj(np.array(shape[1], dtype=np.float64))
                mesh.offset(V(*shape[2]))
                s.shapes.append(mesh)
        for pos, col, inten in desc["lights"]:
            s.lights.append(pkg.create_light(V(*pos), V(*col), inten))
        s.camera = V(*desc["camera"])
    for index, off in sorted(desc.get("moves", {}).items()):
        s.shapes[index].offset(V(*off))                                 # -> rm_scene_offset_shape when the scene is flattened
    if camera is not None:
        s.camera = V(*camera)
    return s


# ---------------------------------------------------------------- frames of the second reading, one job a process
def render_job(job):
    """(description, camera, width, height, depth) -> (rgb rows as nested tuples, probes) of the second reading.
    probes: {(row, col): (hit, shape index as u8, glass, lights shadowed at the first hit, total internal reflections)}"""
    desc, camera, width, height, depth = job
    frame, probes = S.render_frame(second_scene(desc, camera), width, height, max_depth=depth, probe=True)
    return frame.buffer, probes


def rays_job(job):
    """(description, origins, directions, depths) -> per ray (first hit or None as (index as u8, point, normal),
    [cast_ray(origin, direction, ..., 1, depth) for depth in depths]) of the second reading"""
    desc, origins, directions, depths = job
    scene = second_scene(desc)
    out = []
    for o, d in zip(origins, directions):
        o, d = tuple(o), tuple(d)
        first = S.find_closest_intersect(o, d, scene.shapes)
        out.append((None if first is None else (first[1], first[0].point, first[0].normal),
                    [S.cast_ray(o, d, scene.shapes, scene.lights, S.BACKGROUND, 1, depth) for depth in depths]))
    return out


def run_job(job):
    return rays_job(job[1:]) if job[0] == "rays" else render_job(job[1:] if job[0] == "frame" else job)


def render_jobs(jobs, workers=None):
    """Every job's result, in order: ("frame", description, camera, width, height, depth) -- the tag may be left out -- or
    ("rays", description, origins, directions, depths).  The jobs are fanned out over min(16, cpus) fresh processes
    (spawned, so that nothing of the parent -- a GPU context, threads -- is carried over)."""
    workers = S.pool_size() if workers is None else workers
    jobs = [tuple(plain_description(v) if isinstance(v, dict) else plain(v) for v in j) for j in jobs]
    if workers <= 1 or len(jobs) <= 1:
        return [run_job(j) for j in jobs]
    import multiprocessing
    with multiprocessing.get_context("spawn").Pool(min(workers, len(jobs))) as pool:
        return pool.map(run_job, jobs, chunksize=1)


def plain_description(desc):
    if desc.get("default"):
        return desc
    shapes = []
    for shape in desc["shapes"]:
        if shape[0] == "mesh":
            shapes.append(("mesh", plain(shape[1]), plain(shape[2])) + tuple(shape[3:]))
        else:
            shapes.append(tuple(plain(v) if not isinstance(v, dict) else {k: plain(x) for k, x in v.items()} for v in shape))
    return dict(shapes=shapes, lights=plain(desc["lights"]), camera=plain(desc["camera"]), moves=dict(desc.get("moves", {})))
