"""GPU: dropping the child rays that leave a glass-like polygon into an empty half-space (rm_build_empty_sides) spares
ray steps, never changes a picture.  Frames rendered with it (the default) and without (RM_DEAD_CHILDREN=0, read at
rm_init) are bit-equal in both numeric flavours, and the strict ones lie within 1e-9 of the oracle: the demo scene at
three depths, views of workloads.camera_walk, the camera below the floor (children go up into the full side and stay
alive), the floor alone seen grazing from above and from below (both sides empty: the reflected child of a total
reflection is dropped too), two stacked glass quads, a glass triangle with one empty side, and a camera beyond the
limit at which the launch plan switches the bit off."""
import os

import numpy as np
import pytest

import workloads
from test_dead_children import FLOOR, GLASS, empty_sides, plan_bit

pytestmark = pytest.mark.gpu

LOWER = [(x, y - 2., z) for x, y, z in FLOOR]
TRIANGLE = [(-6., -2., -14.), (6., -2., -14.), (0., 5., -11.)]       # its normal points towards the camera (+z, a little -y)
FAR_CAMERA = (0., 0., 2e9)


def _demo(camera=(0., 0., 0.)):
    return dict(scene="demo", camera=camera)


def _custom(shapes, camera=(0., 0., 0.)):
    return dict(scene=shapes, camera=camera)


WALK = workloads.camera_walk(n=48)
CASES = {
    "demo_320x240_d2": (_demo(), 320, 240, 2),
    "demo_256x128_d5": (_demo(), 256, 128, 5),
    "demo_128x64_d8": (_demo(), 128, 64, 8),
    "walk_0": (_demo(WALK[5]), 160, 96, 5),
    "walk_1": (_demo(WALK[21]), 160, 96, 5),
    "walk_2": (_demo(WALK[40]), 160, 96, 5),
    "below_the_floor": (_demo((0., -20., -20.)), 160, 96, 5),
    "floor_alone_grazing_from_above": (_custom([("polygon", FLOOR, GLASS)], (0., -3.2, 0.)), 160, 96, 5),
    "floor_alone_grazing_from_below": (_custom([("polygon", FLOOR, GLASS)], (0., -6.5, 0.)), 160, 96, 5),
    "floor_alone_from_below": (_custom([("polygon", FLOOR, GLASS)], (0., -20., -20.)), 160, 96, 5),
    "stacked_quads": (_custom([("polygon", FLOOR, GLASS), ("polygon", LOWER, GLASS), ("sphere", (0., -1., -12.), 2., None)]), 160, 96, 6),
    "glass_triangle": (_custom([("polygon", TRIANGLE, GLASS), ("sphere", (0., 1., -20.), 3., None)]), 160, 96, 5),
    "camera_beyond_the_limit": (_demo(FAR_CAMERA), 128, 64, 5),
}


def build(pkg, O, what):
    """-> (product scene, oracle scene) of a case."""
    if what["scene"] == "demo":
        s, o = workloads.product_scene(pkg, "demo"), workloads.oracle_scene(O, "demo")
    else:
        s, o = pkg.Scene.new(), O.OracleScene()
        for sh in what["scene"]:
            if sh[0] == "sphere":
                s.shapes.append(pkg.sphere.create(pkg.Vec3f(*sh[1]), sh[2], pkg.Reflectance()))
                o.add_sphere(sh[1], sh[2], O.reflectance())
            else:
                s.shapes.append(pkg.polygon.ConvexPolygon.create([pkg.Vec3f(*v) for v in sh[1]], pkg.Reflectance(**sh[2])))
                o.add_polygon(sh[1], O.reflectance(**sh[2]))
        for pos, col, inten in workloads.DEMO_LIGHTS:
            s.lights.append(pkg.create_light(pkg.Vec3f(*pos), pkg.Vec3f(*col), inten))
            o.add_light(pos, col, inten)
    s.camera = pkg.Vec3f(*what["camera"])
    o.set_camera(what["camera"])
    return s, o


@pytest.fixture(scope="module")
def ctxs(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    old = os.environ.get("RM_DEAD_CHILDREN")
    try:
        os.environ["RM_DEAD_CHILDREN"] = "0"
        off = pkg.backend.Context(0)
        os.environ.pop("RM_DEAD_CHILDREN")
        on = pkg.backend.Context(0)
    finally:
        if old is None:
            os.environ.pop("RM_DEAD_CHILDREN", None)
        else:
            os.environ["RM_DEAD_CHILDREN"] = old
    yield on, off
    on.close()
    off.close()


_oracle_frames = {}


def oracle_frame(O, name, oscene, w, h, depth):
    if name not in _oracle_frames:
        frame = O.render(oscene, w, h, fov=workloads.FOV, max_depth=depth)
        frame.setflags(write=False)
        _oracle_frames[name] = frame
    return _oracle_frames[name]


def both(pkg, ctxs, scene, w, h, depth, flags=0):
    frames = []
    for c in ctxs:
        c.upload(scene.flatten())
        p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)
        p.flags = flags
        out = np.zeros((h, w, 3), dtype=np.float64)
        c.render(p, out)
        frames.append(out)
    return frames


def assert_same(a, b, label):
    same = a.view(np.uint64) == b.view(np.uint64)
    assert same.all(), "%s: %d values differ" % (label, int((~same).sum()))


@pytest.mark.parametrize("name", list(CASES))
def test_strict_frames_bit_equal_and_match_the_oracle(pkg, O, ctxs, name):
    what, w, h, depth = CASES[name]
    scene, oscene = build(pkg, O, what)
    on, off = both(pkg, ctxs, scene, w, h, depth)
    assert_same(on, off, name)
    ref = oracle_frame(O, name, oscene, w, h, depth)
    err = float(np.abs(on - ref).max())
    print("%s: max |delta| vs oracle %.3e, lit %d" % (name, err, int((on.sum(axis=2) > 0).sum())))
    assert err <= 1e-9, "%s: %g off the oracle" % (name, err)
    if name != "camera_beyond_the_limit":
        assert on.any()


@pytest.mark.parametrize("name", list(CASES))
def test_fast_frames_bit_equal(pkg, ctxs, O, name):
    what, w, h, depth = CASES[name]
    scene, _ = build(pkg, O, what)
    on, off = both(pkg, ctxs, scene, w, h, depth, flags=pkg._lib.RM_FLAG_FAST_FP)
    assert_same(on, off, name + " (fast)")


def test_cases_reach_what_they_are_meant_to(pkg, O):
    """The scenes above do carry the flags they are about, and the far camera's launch has the bit off (CPU side of the
    same facts: the flags from the upload, the bit from the launch plan)."""
    def flags_of(name):
        sides, glass, shape_of, limit = empty_sides(pkg, build(pkg, O, CASES[name][0])[0])
        return [sides[shape_of.index(i)] for i in range(len(sides))], limit

    assert flags_of("demo_256x128_d5")[0][5] == 2
    assert flags_of("floor_alone_grazing_from_above")[0] == [3]
    assert flags_of("stacked_quads")[0][:2] == [0, 2]                # the upper quad has the sphere above and the lower one below
    assert flags_of("glass_triangle")[0][0] == 1                     # the sphere is behind it
    limit = flags_of("camera_beyond_the_limit")[1]
    assert 0. < limit < sum(abs(c) for c in FAR_CAMERA)
    assert plan_bit(pkg, FAR_CAMERA, limit) == (0, 1)
    assert plan_bit(pkg, (0., -20., -20.), limit) == (1, 1)
