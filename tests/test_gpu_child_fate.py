"""GPU: deciding a refracted child's fate before its ray is formed (render_tile, DESIGN.md section 4 "early child fates")
spares the root, the normalisation and the offset origin of children that are never walked -- beyond the depth cap, or
into a flagged empty half-space for certain -- and never changes a picture.  Frames of 128x64 rendered with
RM_DEAD_CHILDREN=0 (everything walked), =1 (the fate from the computed ray) and unset (the early fate) are bit-equal in
the f64 frame and in the display bytes, strict and fast flavours, and the strict ones lie within 1e-9 of the oracle:
the demo scene from above the floor, from below it (the flip side; and a floor of index 0.7, whose refracted children
exist there), from inside the blue sphere and from a height at which the floor's far edge crosses tiles; depth caps 1, 2, 3 and 5 (capped children at every level, beside uncapped
lanes of the same wave); a floor flagged on both sides, on one, on none; a camera beyond the launch plan's limit (plan
bit off).  That a scene's waves do mix the kinds of hit is counted on the CPU with the oracle, not assumed: tiles whose
rays -- primary rays and, below the cap, their refracted children -- hit both the floor and a sphere (the floor and the
sky where the scene can hold no sphere, or shows none)."""
import ctypes as C
import os

import numpy as np
import pytest

import workloads
import test_dead_children as flags
import test_gpu_dead_children as scenes

pytestmark = pytest.mark.gpu

W, H = 128, 64
TILE_W, TILE_H = 16, 4
FLOOR, GLASS = scenes.FLOOR, scenes.GLASS
BLUE = (-0.5, -1.5, -5.)                                            # the demo scene's glass sphere, radius 2
THROUGH = [("polygon", FLOOR, GLASS), ("sphere", (0., -4.5, -20.), 3., None), ("sphere", (4., 0., -14.), 2., None)]
# From below, the demo floor (index 1.5) reflects every ray of the fixed view totally: the flip side with no refracted child.
# A floor of index 0.7 seen from below refracts them all (r = 0.7): the flip side with a child -- into the side its normal points
# to, empty where the floor is alone (dead by the flip's certificate), full where spheres stand on it (walked).  From above
# its r is 1 / 0.7 and the rays towards the horizon pass the critical angle.
THIN = dict(GLASS, refractive_index=0.7)
UNDER = [("polygon", FLOOR, THIN), ("sphere", (0., -0.5, -38.), 3., None), ("sphere", (-7., 0.5, -32.), 4., None)]

# name -> (scene, depth cap, what the mixed tiles are counted over: "floor+sphere", or "floor+sky" where the scene cannot
# hold a sphere -- a floor with both sides empty has nothing beside it -- or None: a camera that sees next to nothing)
CASES = {
    "above_d1": (scenes._demo(), 1, "floor+sphere"),
    "above_d2": (scenes._demo(), 2, "floor+sphere"),
    "above_d3": (scenes._demo(), 3, "floor+sphere"),
    "above_d5": (scenes._demo(), 5, "floor+sphere"),
    "below_d2": (scenes._demo((0., -20., -20.)), 2, "floor+sky"),
    "below_d5": (scenes._demo((0., -20., -20.)), 5, "floor+sky"),
    "thin_alone_from_below_d3": (scenes._custom([("polygon", FLOOR, THIN)], (0., -20., -20.)), 3, "floor+sky"),
    "thin_from_below_d2": (scenes._custom(UNDER, (0., -10., -10.)), 2, "floor+sphere"),
    "thin_from_below_d5": (scenes._custom(UNDER, (0., -10., -10.)), 5, "floor+sphere"),
    "thin_from_above_d5": (scenes._custom(UNDER), 5, "floor+sphere"),
    "inside_blue_d3": (scenes._demo((-0.5, -1.5, -4.5)), 3, "floor+sphere"),
    "inside_blue_d5": (scenes._demo((-0.5, -1.5, -4.5)), 5, "floor+sphere"),
    "horizon_d5": (scenes._demo((0., -2.9, 0.)), 5, "floor+sphere"),
    "horizon_d2": (scenes._demo((0., -2.9, 0.)), 2, "floor+sphere"),
    "both_sides_from_above_d5": (scenes._custom([("polygon", FLOOR, GLASS)], (0., -3.2, 0.)), 5, "floor+sky"),
    "both_sides_from_below_d3": (scenes._custom([("polygon", FLOOR, GLASS)], (0., -20., -20.)), 3, "floor+sky"),
    "no_side_d5": (scenes._custom(THROUGH), 5, "floor+sphere"),
    "no_side_d2": (scenes._custom(THROUGH), 2, "floor+sphere"),
    "stacked_quads_d5": (scenes._custom(scenes.CASES["stacked_quads"][0]["scene"]), 5, "floor+sphere"),
    "camera_beyond_the_limit_d5": (scenes._demo(scenes.FAR_CAMERA), 5, None),
}
SIDES = {"above_d5": flags.NEG, "both_sides_from_above_d5": flags.POS | flags.NEG, "no_side_d5": 0}


@pytest.fixture(scope="module")
def ctxs(pkg):
    """Contexts with RM_DEAD_CHILDREN=0, =1 and unset (the knob is read at rm_init)."""
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    old = os.environ.get("RM_DEAD_CHILDREN")
    made = []
    try:
        for v in ("0", "1", None):
            if v is None:
                os.environ.pop("RM_DEAD_CHILDREN", None)
            else:
                os.environ["RM_DEAD_CHILDREN"] = v
            made.append(pkg.backend.Context(0))
    finally:
        if old is None:
            os.environ.pop("RM_DEAD_CHILDREN", None)
        else:
            os.environ["RM_DEAD_CHILDREN"] = old
    yield made
    for c in made:
        c.close()


def renders(pkg, ctxs, scene, depth, fast):
    """-> [(f64 frame, display bytes)] of the three contexts."""
    out = []
    for c in ctxs:
        c.upload(scene.flatten())
        p = pkg.backend.make_params(workloads.FOV, float(H), float(W), depth)
        p.flags = pkg._lib.RM_FLAG_FAST_FP if fast else 0
        frame = np.zeros((H, W, 3), dtype=np.float64)
        c.render(p, frame)
        disp = np.zeros(H * W * 3, dtype=np.uint8)
        c.render_display(p, disp)
        out.append((frame, disp))
    return out


def assert_all_equal(rs, label):
    for k, which in ((0, "RM_DEAD_CHILDREN=0"), (1, "RM_DEAD_CHILDREN=1")):
        scenes.assert_same(rs[2][0], rs[k][0], "%s: default against %s" % (label, which))
        assert np.array_equal(rs[2][1], rs[k][1]), "%s: display bytes, default against %s" % (label, which)


@pytest.mark.parametrize("name", list(CASES))
def test_strict_frames_bit_equal_and_match_the_oracle(pkg, O, ctxs, name):
    what, depth, _ = CASES[name]
    scene, oscene = scenes.build(pkg, O, what)
    rs = renders(pkg, ctxs, scene, depth, fast=False)
    assert_all_equal(rs, name)
    ref = scenes.oracle_frame(O, "child_fate_" + name, oscene, W, H, depth)
    err = float(np.abs(rs[2][0] - ref).max())
    print("%s: max |delta| vs oracle %.3e, lit %d" % (name, err, int((rs[2][0].sum(axis=2) > 0).sum())))
    assert err <= 1e-9, "%s: %g off the oracle" % (name, err)
    if CASES[name][2]:
        assert rs[2][0].any()


@pytest.mark.parametrize("name", list(CASES))
def test_fast_frames_bit_equal(pkg, O, ctxs, name):
    what, depth, _ = CASES[name]
    scene, _ = scenes.build(pkg, O, what)
    assert_all_equal(renders(pkg, ctxs, scene, depth, fast=True), name + " (fast)")


def hits_by_tile(O, oscene, depth):
    """-> per tile, the sets of shapes (indices; -1: a miss) its primary rays and -- below the cap -- their refracted children
    hit, by the oracle's own closest-hit search and refraction."""
    L = O.lib()
    c = oscene.c
    r = L.orc_create_renderer(workloads.FOV, float(H), float(W))
    tiles = {}
    for y in range(H):
        for x in range(W):
            seen = tiles.setdefault((x // TILE_W, y // TILE_H), set())
            d = L.orc_normalized(L.orc_backproject(C.byref(r), x, y))
            its, which = O.Intersection(), C.c_uint8(0)
            if not L.orc_find_closest_intersect(c.camera, d, c.shapes, c.n_shapes, C.byref(its), C.byref(which)):
                seen.add(-1)
                continue
            seen.add(int(which.value))
            if depth < 2 or not its.reflectance.is_glass_like:
                continue
            o2, d2 = O.Vec3(), O.Vec3()
            if L.orc_refract_ray(d, C.byref(its), its.reflectance.refractive_index, C.byref(o2), C.byref(d2)):
                its2 = O.Intersection()
                hit = L.orc_find_closest_intersect(o2, d2, c.shapes, c.n_shapes, C.byref(its2), C.byref(which))
                seen.add(int(which.value) if hit else -1)
    return tiles


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][2]])
def test_scenes_mix_the_kinds_of_hit_within_a_tile(pkg, O, name):
    what, depth, kind = CASES[name]
    scene, oscene = scenes.build(pkg, O, what)
    c = oscene.c
    floors = {i for i in range(c.n_shapes) if c.shapes[i].n_vertices == 4}
    spheres = {i for i in range(c.n_shapes) if c.shapes[i].n_vertices == 0 and c.shapes[i].n_triangles == 0}
    other = spheres if kind == "floor+sphere" else {-1}
    tiles = hits_by_tile(O, oscene, depth)
    mixed = sum(1 for seen in tiles.values() if seen & floors and seen & other)
    print("%s: %d of %d tiles mix %s" % (name, mixed, len(tiles), kind))
    assert mixed >= 1, "%s: no tile mixes %s" % (name, kind)


def test_scenes_carry_the_flags_they_are_about(pkg, O):
    """The floor flagged on both sides, on one side and on none (CPU side: the flags from the upload), and the far camera's
    launch with the plan's bit off."""
    for name, want in SIDES.items():
        sides, _, shape_of, _ = flags.empty_sides(pkg, scenes.build(pkg, O, CASES[name][0])[0])
        floor = 5 if name == "above_d5" else 0
        assert sides[shape_of.index(floor)] == want, name
    _, _, _, limit = flags.empty_sides(pkg, scenes.build(pkg, O, CASES["camera_beyond_the_limit_d5"][0])[0])
    assert 0. < limit < sum(abs(v) for v in scenes.FAR_CAMERA)
    assert flags.plan_bit(pkg, scenes.FAR_CAMERA, limit) == (0, 1)
    assert flags.plan_bit(pkg, (0., -20., -20.), limit) == (1, 1)
