"""GPU: the shadow rays' occluder masks change which primitives a shadow walk tests, never a picture.
Frames rendered with the masks (the default) and without them (RM_SHADOW_MASKS=0, read at rm_init) are
bit-equal: C1, C2, C4, views of workloads.camera_walk, the fast flavour, and seeded random scenes of up to
11 primitives with lights inside, on and around their bounds."""
import os

import numpy as np
import pytest

import workloads
from test_shadow_masks import build_pair, masks, random_shapes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    old = os.environ.get("RM_SHADOW_MASKS")
    try:
        os.environ["RM_SHADOW_MASKS"] = "0"
        off = pkg.backend.Context(0)
        os.environ.pop("RM_SHADOW_MASKS")
        on = pkg.backend.Context(0)
    finally:
        if old is None:
            os.environ.pop("RM_SHADOW_MASKS", None)
        else:
            os.environ["RM_SHADOW_MASKS"] = old
    yield on, off
    on.close()
    off.close()


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


@pytest.mark.parametrize("config", ["C1", "C2", "C4"])
def test_configs_bit_equal(pkg, ctxs, config):
    cfg = workloads.CONFIGS[config]
    on, off = both(pkg, ctxs, workloads.product_scene(pkg, cfg["scene"]), cfg["width"], cfg["height"], cfg["max_depth"])
    assert on.any()
    assert_same(on, off, config)


def test_fast_flavour_bit_equal(pkg, ctxs):
    on, off = both(pkg, ctxs, workloads.product_scene(pkg, "demo"), 640, 480, 5, flags=pkg._lib.RM_FLAG_FAST_FP)
    assert_same(on, off, "fast")


def test_camera_walk_bit_equal(pkg, ctxs):
    scene = workloads.product_scene(pkg, "demo")
    for cam in workloads.camera_walk(n=48)[::8]:
        scene.camera = pkg.Vec3f(*cam)
        on, off = both(pkg, ctxs, scene, 640, 480, 5)
        assert_same(on, off, "camera %s" % (cam,))


@pytest.mark.parametrize("seed", range(24))
def test_random_scenes_bit_equal(pkg, O, ctxs, seed):
    shapes, lights = random_shapes(seed)
    scene, _ = build_pair(pkg, O, shapes, lights)
    assert masks(pkg, scene)[0] is not None
    on, off = both(pkg, ctxs, scene, 256, 192, 5)
    assert_same(on, off, "seed %d" % seed)


def test_identical_upload_still_skipped(pkg, ctxs):
    c = ctxs[0]
    scene = workloads.product_scene(pkg, "demo")
    c.upload(scene.flatten())
    calls, copies = c.uploads()
    c.upload(scene.flatten())
    c.set_camera((0., 1., 2.))
    assert c.uploads() == (calls + 1, copies)
