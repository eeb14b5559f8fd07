"""CPU checks of the scene signature (csrc/rm_plan.cpp rm_scene_signature and the bits plan_launch puts into
KernelArgs::dead_children): the plain-walk kernels carry a second tile body compiled for the shape counts of the reference's
default scene, and a launch takes it only where the resident image's counts, every polygon's vertex count, list_ordered and
the absence of a hierarchy are that signature's, word for word.  On for the default scene and for a seeded scene of the same
counts; off under RM_SCENE_SIG=0; off for every near miss, one pinned field changed at a time; on in every plain-walk kernel
(both powers, every ray stack), off where the launch takes a kernel with the bundle cull.  The export used here (rmi_plan_scene_sig) is not part of the ABI
and needs no device."""
import ctypes as C

import pytest

import scene_sig_scenes as S
from test_scene_image import scene_image as image_of

DEFAULT_SCENE = 1                      # the signature's number: its place in RM_SCENE_SIGNATURES, from 1


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    for k in ("RM_SCENE_SIG", "RM_FORCE_GENERIC_POW", "RM_FORCE_STACK", "RM_FORCE_UNSTAGED", "RM_DISABLE_BVH", "RM_CULL_MIN"):
        monkeypatch.delenv(k, raising=False)


def test_the_signature_is_the_default_scenes_image(pkg):
    """The compiled-in counts, read off the image the library's own default scene uploads to -- not off anybody's description."""
    handle = pkg.Scene.create_default().flatten()
    st, img = image_of(pkg, handle.desc(), use_bvh=1, masks=1)
    assert st == 0
    H = img["H"]
    assert (H["n_spheres"], H["n_polygons"], H["n_triangles"], H["n_lights"], H["list_ordered"]) == (4, 2, 0, 2, 1)
    assert (H["off_bvh_spheres"], H["off_bvh_triangles"]) == (0, 0)
    # every polygon's vertex count: the second half of its record's seventh word
    nv = [int(img["blob"][H["off_polygons"] + 16 * g + 6] >> 32) for g in range(H["n_polygons"])]
    assert nv == [3, 4]


@pytest.mark.parametrize("depth", [1, 2, 3, 5, 8, 9, 10, 17, 18, 32])
@pytest.mark.parametrize("fast", [False, True])
def test_on_for_the_default_scene(pkg, depth, fast):
    assert S.plan_verdict(pkg, pkg.Scene.create_default(), depth, fast) == (DEFAULT_SCENE, DEFAULT_SCENE, 1)


def test_on_for_the_default_scene_restated_and_moved(pkg):
    assert S.plan_verdict(pkg, S.build(pkg, None, S.demo())[0]) == (DEFAULT_SCENE, DEFAULT_SCENE, 1)
    assert S.plan_verdict(pkg, S.build(pkg, None, S.demo(camera=(3., 2., 6.)))[0]) == (DEFAULT_SCENE, DEFAULT_SCENE, 1)


@pytest.mark.parametrize("seed", [0x5167, 1, 2])
def test_on_for_another_scene_of_the_same_counts(pkg, seed):
    assert S.plan_verdict(pkg, S.build(pkg, None, S.random_same_signature(seed))[0]) == (DEFAULT_SCENE, DEFAULT_SCENE, 1)


def test_off_by_the_knob(pkg, monkeypatch):
    monkeypatch.setenv("RM_SCENE_SIG", "0")
    assert S.plan_verdict(pkg, pkg.Scene.create_default()) == (DEFAULT_SCENE, 0, 1)
    monkeypatch.setenv("RM_SCENE_SIG", "1")
    assert S.plan_verdict(pkg, pkg.Scene.create_default()) == (DEFAULT_SCENE, DEFAULT_SCENE, 1)


@pytest.mark.parametrize("name", list(S.NEAR_MISSES))
def test_off_for_every_near_miss(pkg, name):
    image_sig, launch_sig, _ = S.plan_verdict(pkg, S.build(pkg, None, S.NEAR_MISSES[name])[0])
    assert (image_sig, launch_sig) == (0, 0), name


def test_the_near_misses_miss_by_the_field_they_name(pkg):
    """One pinned field differs from the default scene's image, the others do not."""
    def pinned(what):
        st, img = image_of(pkg, S.build(pkg, None, what)[0].flatten().desc(), use_bvh=1, masks=1)
        assert st == 0
        H = img["H"]
        nv = tuple(int(img["blob"][H["off_polygons"] + 16 * g + 6] >> 32) for g in range(H["n_polygons"]))
        return dict(n_spheres=H["n_spheres"], n_polygons=H["n_polygons"], n_triangles=H["n_triangles"], n_lights=H["n_lights"],
                    list_ordered=H["list_ordered"], hierarchy=int(H["off_bvh_spheres"] != 0 or H["off_bvh_triangles"] != 0), nv=nv)

    base = pinned(S.demo())
    differs = {name: sorted(k for k, v in pinned(what).items() if v != base[k]) for name, what in S.NEAR_MISSES.items()}
    assert differs == {
        "three_spheres": ["n_spheres"], "five_spheres": ["n_spheres"],
        "quad_as_triangle": ["nv"], "quad_as_pentagon": ["nv"], "triangle_as_quad": ["nv"], "polygons_swapped": ["nv"],
        "no_triangle": ["n_polygons", "nv"], "two_triangles": ["n_polygons", "nv"],
        "a_mesh_triangle": ["n_triangles"],
        "one_light": ["n_lights"], "three_lights": ["n_lights"],
        "triangle_listed_first": ["list_ordered"],
        "a_hierarchy": ["hierarchy", "list_ordered", "n_spheres"],          # (its spheres are stored in leaf order)
    }


def test_on_in_every_plain_walk_kernel_and_off_in_the_others(pkg, monkeypatch):
    """Both powers and every ray stack of the plain-walk kernels carry the body; the kernels with the bundle cull do not."""
    scene = pkg.Scene.create_default()
    monkeypatch.setenv("RM_FORCE_STACK", "16")
    assert S.plan_verdict(pkg, scene, depth=5) == (DEFAULT_SCENE, DEFAULT_SCENE, 1)
    monkeypatch.delenv("RM_FORCE_STACK")
    monkeypatch.setenv("RM_FORCE_GENERIC_POW", "1")
    assert S.plan_verdict(pkg, scene) == (DEFAULT_SCENE, DEFAULT_SCENE, 1)
    monkeypatch.delenv("RM_FORCE_GENERIC_POW")
    # an exponent that is no integer: the image's verdict sends the launch to the generic power
    what = S.demo()
    what["shapes"] = [("sphere",) + what["shapes"][0][1:3] + (dict(S.BLUE, specular_exponent=12.5),)] + what["shapes"][1:]
    assert S.plan_verdict(pkg, S.build(pkg, None, what)[0]) == (DEFAULT_SCENE, DEFAULT_SCENE, 1)
    monkeypatch.setenv("RM_FORCE_UNSTAGED", "1")                                 # no LDS copy: the kernels with the bundle cull
    assert S.plan_verdict(pkg, scene) == (DEFAULT_SCENE, 0, 0)
    monkeypatch.delenv("RM_FORCE_UNSTAGED")
    monkeypatch.setenv("RM_CULL_MIN", "4")
    assert S.plan_verdict(pkg, scene) == (DEFAULT_SCENE, 0, 0)


def test_the_other_bits_of_the_word_stay(pkg, monkeypatch):
    """The signature shares its word with the dead children's two bits: neither moves the other (rmi_plan_dead_children
    reports the word's low bit as before, with and without the knob)."""
    from test_dead_children import empty_sides, plan_bit
    limit = empty_sides(pkg, pkg.Scene.create_default())[3]
    for v in (None, "0"):
        if v is not None:
            monkeypatch.setenv("RM_SCENE_SIG", v)
        assert plan_bit(pkg, (0., 0., 0.), limit) == (1, 1)
        assert plan_bit(pkg, (0., 0., 2e9), limit) == (0, 1)


def test_a_null_argument_is_refused(pkg):
    f = pkg.lib().rmi_plan_scene_sig
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    assert f(None, 1, 5, 0, (C.c_uint32 * 3)()) != 0
