"""CPU checks of the checked numerics' routing (rm_trace.inc RM_CHECKED: the strict plain-walk kernels' range-free square
roots and reciprocals): which scenes the upload marks "exact only" (rm_image.cpp scene_exact_only), which cameras the launch
plan does (rm_plan.cpp rm_camera_exact_only, RM_CHECKED_NUMERICS=0 on top), and the material word that holds 1 / refractive_index
for reflect_child / refract_child.  The internal exports used here (rmi_upload_numerics, rmi_plan_exact_only) are not part of
the ABI and need no device.  Bounds, from rm_plan.hpp: every coordinate, radius and light word finite and at most 2^200 in
magnitude, every radius_square within [2^-600, 2^600]."""
import ctypes as C
import math

import numpy as np
import pytest

FIXED = ((1., 0., 0.), (0., 1., 0.), (0., 0., -1.))
NAN, INF = float("nan"), float("inf")


def upload_numerics(pkg, scene):
    """-> (exact only?, material words [pids][10]) of the image `scene` uploads to."""
    f = pkg.lib().rmi_upload_numerics
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_uint32)]
    d = scene.flatten().desc()
    mats = (C.c_double * 4096)()
    dims = (C.c_uint32 * 2)()
    assert f(C.addressof(d), mats, 4096, dims) == 0 and 10 * dims[0] <= 4096
    return bool(dims[1]), np.array(mats[:10 * dims[0]], dtype=np.float64).reshape(dims[0], 10)


def plan_exact_only(pkg, camera, basis=None, scene_exact_only=False):
    f = pkg.lib().rmi_plan_exact_only
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    cam = pkg._lib.vec3(camera)
    b = pkg._lib.camera_basis(FIXED if basis is None else basis)
    out = C.c_uint32(7)
    assert f(C.addressof(cam), C.addressof(b), 0 if basis is None else 1, 1 if scene_exact_only else 0, C.byref(out)) == 0
    assert out.value in (0, 3), "the plan's flag and the kernel argument disagree: %d" % out.value
    return out.value == 3


def scene_of(pkg, sphere=((0., 0., -10.), 2.), quad=None, light=(5., 5., 0.), intensity=1.):
    V = pkg.Vec3f
    s = pkg.Scene.new()
    if sphere is not None:
        s.shapes.append(pkg.sphere.create(V(*sphere[0]), sphere[1], pkg.Reflectance()))
    if quad is not None:
        s.shapes.append(pkg.polygon.ConvexPolygon.create([V(*p) for p in quad], pkg.Reflectance()))
    s.lights.append(pkg.create_light(V(*light), V(1., 1., 1.), intensity))
    return s


QUAD = [(-2., -2., -4.), (2., -2., -4.), (2., 2., -4.), (-2., 2., -4.)]

UPLOAD_TABLE = [
    ("plain", dict(), False),
    ("quad", dict(quad=QUAD), False),
    ("radius_square 2^-600", dict(sphere=((0., 0., -10.), 2. ** -300)), False),
    ("radius_square 2^-602", dict(sphere=((0., 0., -10.), 2. ** -301)), True),
    ("radius_square 2^-800", dict(sphere=((0., 0., -10.), 2. ** -400)), True),
    ("radius_square 2^200", dict(sphere=((0., 0., -10.), 2. ** 100)), False),
    ("radius_square 2^202", dict(sphere=((0., 0., -10.), 2. ** 101)), True),
    ("radius_square 0", dict(sphere=((0., 0., -10.), 0.)), True),
    ("radius NaN", dict(sphere=((0., 0., -10.), NAN)), True),
    ("centre 2^200", dict(sphere=((2. ** 200, 0., -10.), 2.)), False),
    ("centre 1e200", dict(sphere=((1e200, 0., -10.), 2.)), True),
    ("centre -1e200", dict(sphere=((0., -1e200, -10.), 2.)), True),
    ("centre inf", dict(sphere=((0., 0., INF), 2.)), True),
    ("centre NaN", dict(sphere=((NAN, 0., -10.), 2.)), True),
    ("vertex 1e200", dict(quad=[(-2., -2., -4.), (1e200, -2., -4.), (2., 2., -4.), (-2., 2., -4.)]), True),
    ("light 1e60", dict(light=(1e60, 0., 0.)), False),
    ("light 1e200", dict(light=(0., 1e200, 0.)), True),
    ("light NaN", dict(light=(0., 0., NAN)), True),
    ("intensity inf", dict(intensity=INF), True),
]


@pytest.mark.parametrize("label,kw,expected", UPLOAD_TABLE, ids=[t[0] for t in UPLOAD_TABLE])
def test_upload_decision(pkg, label, kw, expected):
    assert upload_numerics(pkg, scene_of(pkg, **kw))[0] == expected, label


def test_reference_scenes_are_checked(pkg):
    import workloads
    for name in ("demo", "cornell", "synthetic256"):
        assert not upload_numerics(pkg, workloads.product_scene(pkg, name))[0], name


CAMERA_TABLE = [
    ((0., 0., 0.), None, False),
    ((5., 10., 15.), None, False),
    ((1e60, 0., 0.), None, False),
    ((2. ** 200, 0., 0.), None, False),
    ((1e200, 0., 0.), None, True),
    ((0., -1e200, 0.), None, True),
    ((0., 0., INF), None, True),
    ((NAN, 0., 0.), None, True),
    ((0., NAN, 0.), None, True),
    ((0., 0., 0.), ((0., 0., -1.), (0., 1., 0.), (-1., 0., 0.)), False),
    ((0., 0., 0.), ((0., 0., -1.), (0., NAN, 0.), (-1., 0., 0.)), True),
    ((0., 0., 0.), ((0., 0., -1.), (0., 1., 0.), (-1e200, 0., 0.)), True),
]


@pytest.mark.parametrize("camera,basis,expected", CAMERA_TABLE)
def test_plan_camera_decision(pkg, monkeypatch, camera, basis, expected):
    monkeypatch.delenv("RM_CHECKED_NUMERICS", raising=False)
    assert plan_exact_only(pkg, camera, basis) == expected
    # the scene's verdict and the knob decide on top of the camera's
    assert plan_exact_only(pkg, camera, basis, scene_exact_only=True)
    monkeypatch.setenv("RM_CHECKED_NUMERICS", "0")
    assert plan_exact_only(pkg, camera, basis)
    monkeypatch.setenv("RM_CHECKED_NUMERICS", "1")
    assert plan_exact_only(pkg, camera, basis) == expected


def test_material_word_holds_reciprocal_index(pkg):
    V = pkg.Vec3f
    s = pkg.Scene.new()
    indices = [1.5, 1.3, 1., 1. / 3., 2.4175, 1e-300, 0.]
    for k, ri in enumerate(indices):
        s.shapes.append(pkg.sphere.create(V(3. * k, 0., -20.), 1., pkg.Reflectance(is_glass_like=(k % 2 == 0), refractive_index=ri)))
    s.lights.append(pkg.create_light(V(0., 0., 0.), V(1., 1., 1.), 1.))
    _, mats = upload_numerics(pkg, s)
    assert mats.shape == (len(indices), 10)
    for m, ri in zip(mats, indices):
        assert m[7] == ri
        want = np.float64(1.) / np.float64(ri) if ri != 0. else math.inf
        assert m[9] == want and np.float64(m[9]).view(np.uint64) == np.float64(want).view(np.uint64)
    # the reference's own scene: every primitive's word, glass or not
    _, demo = upload_numerics(pkg, pkg.Scene.create_default())
    assert len(demo) == 6 and (demo[:, 8] != 0.).any()
    with np.errstate(divide="ignore"):
        assert np.array_equal((1. / demo[:, 7]).view(np.uint64), demo[:, 9].view(np.uint64))
