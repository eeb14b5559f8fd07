"""Scenes of the scene-signature tests (tests/test_scene_sig.py, tests/test_gpu_scene_sig.py), as lists of shapes that build
the product's scene and the oracle's alike: the reference's default scene restated shape by shape (scene.rs:28-211: four
spheres, a triangle and a quad as polygons, two lights -- the signature the plain-walk kernels carry a body for), a seeded
scene of the same counts with everything else different, and the near misses: the default scene with exactly one of the
fields a signature pins changed."""
import ctypes as C

import numpy as np

import workloads

# scene.rs:32-171, the materials by what Reflectance() leaves at its default
RED = dict(diffuse_color=(0.8, 0., 0.), specular_exponent=100.)
PURPLE = dict(diffuse_color=(0.6, 0., 0.7), specular_exponent=100.)
BLUE = dict(diffusion=0.1, diffuse_color=(0., 0., 0.2), specular=1., specular_exponent=100., is_glass_like=True, reflection=0.2,
            refractive_index=1.5)
GREEN = dict(diffusion=1., diffuse_color=(0., 1., 0.), specular=0.8, specular_exponent=100., is_glass_like=False, reflection=1.,
             refractive_index=1.5)
WHITE = dict(GREEN, diffuse_color=(0.9, 0.9, 0.9))
FLOOR = dict(workloads.FLOOR_MATERIAL)
TRI = [(7., -4., -8.), (15., 0., -9.), (6., 3., -8.)]
QUAD = list(workloads.FLOOR_QUAD)
SPHERES = [("sphere", (-0.5, -1.5, -5.), 2., BLUE), ("sphere", (6., -0.5, -18.), 3., GREEN), ("sphere", (-5., 0., -16.), 4., RED),
           ("sphere", (-10., 6., -14.), 4., WHITE)]
POLYGONS = [("polygon", TRI, PURPLE), ("polygon", QUAD, FLOOR)]
LIGHTS = list(workloads.DEMO_LIGHTS)

# coplanar with the three / four vertices they join, and convex with them
TRI_AS_QUAD = TRI + [(-2., -1., -7.)]                                # v0 + v2 - v1: a parallelogram
QUAD_AS_PENTAGON = QUAD + [(22., -4.5, -26.5)]                       # on the floor's plane, outside the edge v3 -> v0
SMALL_TRI = [(-9., -3., -9.), (-5., -3., -10.), (-8., 1., -9.)]
MESH_TRIANGLE = [-9., -3., -9., -5., -3., -10., -8., 1., -9.]        # the same three points as a mesh of one triangle
EXTRA_SPHERE = ("sphere", (3., 3., -12.), 1.5, RED)
THIRD_LIGHT = ((-15., 10., 5.), (0.5, 1., 0.5), 0.6)


def demo(shapes=None, lights=None, camera=(0., 0., 0.)):
    return dict(shapes=SPHERES + POLYGONS if shapes is None else shapes, lights=LIGHTS if lights is None else lights, camera=camera)


def random_same_signature(seed=0x5167, camera=(0., 0., 0.)):
    """The signature's counts in the default scene's list order, nothing else of it: other centres, radii, polygons and lights;
    glass and opaque materials, other (integer) exponents."""
    rng = np.random.RandomState(seed)

    def material(glass):
        return dict(diffusion=float(rng.uniform(0.1, 1.)), diffuse_color=tuple(float(c) for c in rng.uniform(0., 1., 3)),
                    specular=float(rng.uniform(0.2, 1.)), specular_exponent=float(rng.choice([1., 8., 30., 64.])),
                    is_glass_like=bool(glass), reflection=float(rng.uniform(0.1, 0.9)),
                    refractive_index=float(rng.uniform(1.1, 1.8)) if glass else 1.)

    shapes = []
    for i in range(4):
        centre = (float(rng.uniform(-9., 9.)), float(rng.uniform(-2., 5.)), float(rng.uniform(-22., -8.)))
        shapes.append(("sphere", centre, float(rng.uniform(1., 3.)), material(i % 2 == 0)))
    z = float(rng.uniform(-12., -7.))
    shapes.append(("polygon", [(-3. + float(rng.uniform(-1., 1.)), -2., z), (4., -1. + float(rng.uniform(-1., 1.)), z - 1.),
                               (0.5, 4. + float(rng.uniform(-1., 1.)), z)], material(True)))
    tilt = float(rng.uniform(0., 2.))
    shapes.append(("polygon", [(25., -4., -60.), (-25., -4., -60.), (-18., -4. - tilt, -2.), (18., -4. - tilt, -2.)], material(True)))
    lights = [((float(rng.uniform(-5., 5.)), float(rng.uniform(0., 8.)), float(rng.uniform(0., 5.))), (1., 0.9, 0.8), 0.9),
              ((-20., 15., 10.), (0.6, 0.7, 1.), 0.7)]
    return dict(shapes=shapes, lights=lights, camera=camera)


def many_spheres():
    """Enough spheres for a hierarchy (sixteen and more: rm_image.cpp), in front of the default scene's floor."""
    rng = np.random.RandomState(0xB17)
    balls = [("sphere", (float(rng.uniform(-12., 12.)), float(rng.uniform(-2., 6.)), float(rng.uniform(-30., -10.))),
              float(rng.uniform(0.5, 1.5)), RED) for _ in range(20)]
    return demo(balls + POLYGONS)


# name -> the default scene with one pinned field changed (what the name says), in the order of the signature's fields
NEAR_MISSES = {
    "three_spheres": demo(SPHERES[:3] + POLYGONS),
    "five_spheres": demo(SPHERES + [EXTRA_SPHERE] + POLYGONS),
    "quad_as_triangle": demo(SPHERES + [POLYGONS[0], ("polygon", QUAD[:3], FLOOR)]),
    "quad_as_pentagon": demo(SPHERES + [POLYGONS[0], ("polygon", QUAD_AS_PENTAGON, FLOOR)]),
    "triangle_as_quad": demo(SPHERES + [("polygon", TRI_AS_QUAD, PURPLE), POLYGONS[1]]),
    "polygons_swapped": demo(SPHERES + [POLYGONS[1], POLYGONS[0]]),
    "no_triangle": demo(SPHERES + [POLYGONS[1]]),
    "two_triangles": demo(SPHERES + [POLYGONS[0], ("polygon", SMALL_TRI, PURPLE), POLYGONS[1]]),
    "a_mesh_triangle": demo(SPHERES + POLYGONS + [("mesh", MESH_TRIANGLE)]),
    "one_light": demo(lights=LIGHTS[:1]),
    "three_lights": demo(lights=LIGHTS + [THIRD_LIGHT]),
    "triangle_listed_first": demo([POLYGONS[0]] + SPHERES + [POLYGONS[1]]),     # pids regroup by kind: list_ordered is 0
    "a_hierarchy": many_spheres(),
}


def build(pkg, O, what):
    """-> (product scene, oracle scene) of a scene given as above; O may be None (no oracle scene then)."""
    s, o = pkg.Scene.new(), (O.OracleScene() if O is not None else None)
    for sh in what["shapes"]:
        if sh[0] == "sphere":
            s.shapes.append(pkg.sphere.create(pkg.Vec3f(*sh[1]), sh[2], pkg.Reflectance(**sh[3])))
            if o is not None:
                o.add_sphere(sh[1], sh[2], O.reflectance(**sh[3]))
        elif sh[0] == "polygon":
            s.shapes.append(pkg.polygon.ConvexPolygon.create([pkg.Vec3f(*v) for v in sh[1]], pkg.Reflectance(**sh[2])))
            if o is not None:
                o.add_polygon(sh[1], O.reflectance(**sh[2]))
        else:
            s.shapes.append(pkg.obj.Obj(np.array(sh[1], dtype=np.float64)))
            if o is not None:
                o.add_obj(np.array(sh[1], dtype=np.float64))
    for pos, col, inten in what["lights"]:
        s.lights.append(pkg.create_light(pkg.Vec3f(*pos), pkg.Vec3f(*col), inten))
        if o is not None:
            o.add_light(pos, col, inten)
    s.camera = pkg.Vec3f(*what["camera"])
    if o is not None:
        o.set_camera(what["camera"])
    return s, o


def plan_verdict(pkg, scene, depth=5, fast=False, use_bvh=True):
    """-> (the signature of the image `scene` uploads to, the signature its launch carries, the kernel has a body for
    signatures), planned with the environment's knobs (rmi_plan_scene_sig: an internal export, no device)."""
    f = pkg.lib().rmi_plan_scene_sig
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    handle = scene.flatten()
    d = handle.desc()
    out = (C.c_uint32 * 3)()
    assert f(C.addressof(d), 1 if use_bvh else 0, depth, 1 if fast else 0, out) == 0, pkg.lib().rm_last_error(None)
    return out[0], out[1], out[2]
