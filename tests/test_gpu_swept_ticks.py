"""The ticks that move a shape, through the swept hierarchy and beside the flat walk, on the GPU (-m gpu): the moving camera's
ticks given velocities (rm_render_progressive_camera, rm_render_converging_camera) and the moving spheres' ticks
(rm_render_progressive_motion, rm_render_converging_motion) in a default context and in one with RM_SWEPT_BVH=0 -- counts,
reports, means and bytes equal tick for tick -- and rm_swept_tick_info, which tells a tick that walked a swept hierarchy from one
that quietly walked flat: two flat runs compare equal too.

Frames are 32 x 32, a tick casts 5 samples, depth 5."""
import numpy as np
import pytest

import hierarchy_reference as HR
import moving_reference as MV
import motion_reference as MR
import radiance_reference as RR
import test_gpu_lens as GL
import test_gpu_progressive as GP
import test_gpu_swept as GSW
import variant_matrix as VM
import workloads

pytestmark = pytest.mark.gpu

NAN, BYTE = GP.NAN, GP.BYTE
CAMERA_VELOCITY, CAMERA_TURN = (0.5, 0.2, -0.25), (0.15, 0.05, -0.1)
# (restart, the velocities' factor): restart, continue, changed velocity, continue
TICKS = ((True, 1.), (False, 1.), (False, 1.5), (False, 1.5))
CONVERGE = (0.01, 10, 20)                                              # tolerance, min_samples, max_samples


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_swept_ticks"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return MV.Yardstick(pkg, O, orc)


def params(pkg):
    return pkg.backend.make_params(workloads.FOV, 32., 32., 5)


def info(c):
    t = c.swept_tick_info()
    return t["walked_swept"], t["builds"]


def tick(pkg, c, family, v, restart=False):
    """One tick of 5 samples of `family` -> (count or report, the mean's bytes, the display bytes)."""
    p = params(pkg)
    rgb, rgb8 = np.full((32, 32, 3), NAN), np.full((32, 32, 3), BYTE, np.uint8)
    out = dict(restart=restart, host_rgb=rgb, host_rgb8=rgb8)
    if family == "progressive_camera":
        _, total = c.render_progressive_camera(p, CAMERA_VELOCITY, MV.SHUTTER, VM.APERTURE, VM.FOCUS, 5, CAMERA_TURN, v, **out)
    elif family == "converging_camera":
        _, rep = c.render_converging_camera(p, CAMERA_VELOCITY, MV.SHUTTER, VM.APERTURE, VM.FOCUS, 5, *CONVERGE, CAMERA_TURN, v, **out)
    elif family == "progressive_motion":
        _, total = c.render_progressive_motion(p, v, MV.SHUTTER, VM.APERTURE, VM.FOCUS, 5, **out)
    elif family == "converging_motion":
        _, rep = c.render_converging_motion(p, v, MV.SHUTTER, VM.APERTURE, VM.FOCUS, 5, *CONVERGE, **out)
    elif family == "progressive_moving":
        _, total = c.render_progressive_moving(p, v, MV.SHUTTER, VM.APERTURE, VM.FOCUS, 5, **out)
    else:
        raise AssertionError(family)
    assert not np.isnan(rgb).any()
    what = total if family.startswith("progressive") else (rep.listed, rep.passes, rep.max_count, rep.samples_cast)
    return what, rgb.tobytes(), rgb8.tobytes()


def velocities_of(Y, key, family):
    """The test velocities: on every shape for the camera's ticks, on the spheres alone for the moving spheres'."""
    kinds = Y.kinds(key)
    v = np.asarray(MR.velocities(kinds) if family.endswith("_motion") else MV.velocities(kinds, MV.CELL_SPEED), dtype=np.float64)
    assert (v != 0.).any()
    return v


def four_ticks(pkg, c, scene, family, v):
    """-> (the four ticks' results, rm_swept_tick_info after each)."""
    GL.upload(c, scene)
    out, seen = [], []
    for restart, factor in TICKS:
        out.append(tick(pkg, c, family, factor * v, restart))
        seen.append(info(c))
    return out, seen


CASES = [(family, name) for family in ("progressive_camera", "converging_camera") for name in ("matrix-mesh", "matrix-spheres")] + \
        [(family, name) for family in ("progressive_motion", "converging_motion") for name in ("matrix-spheres", "seventeen")]


@pytest.mark.parametrize("family,name", CASES, ids=["%s-%s" % c for c in CASES])
def test_the_ticks_walk_the_hierarchy_to_the_flat_ticks_bytes(pkg, Y, family, name, monkeypatch):
    """Two contexts, the default and RM_SWEPT_BVH=0 (flat, as these ticks always were): restart, continue, a changed velocity,
    continue.  Equal counts or reports, means and bytes tick for tick; the changed velocity began the frame again and is another
    picture.  The default context walked a swept hierarchy in every tick and built two; the other none."""
    key, scene = GSW.scene_of(Y, name)
    v = velocities_of(Y, key, family)
    c = pkg.backend.Context(0)
    try:
        assert info(c) == (0, 0)
        swept, seen = four_ticks(pkg, c, scene, family, v)
    finally:
        c.close()
    assert seen == [(1, 1), (1, 1), (1, 2), (1, 2)], seen
    monkeypatch.setenv("RM_SWEPT_BVH", "0")
    c = pkg.backend.Context(0)
    try:
        flat, seen = four_ticks(pkg, c, scene, family, v)
    finally:
        c.close()
    assert seen == [(0, 0)] * 4, seen
    if family.startswith("progressive"):
        assert [t[0] for t in swept] == [5, 10, 5, 10]                  # the changed velocity began the frame again
    else:
        assert [t[0][1] for t in swept] == [1, 2, 1, 2]
    for k, (a, b) in enumerate(zip(swept, flat)):
        assert a == b, "%s, %s: tick %d differs between the swept and the flat walk" % (family, name, k)
    assert swept[1][1] != swept[3][1]                                   # ... and the faster shapes are another picture


def test_the_ticks_share_one_hierarchy(pkg, Y):
    """A camera tick behind a moving shapes' tick with the same velocities and shutter adds no build; a moving spheres' tick with
    other velocities does, and the way back too."""
    key, scene = GSW.scene_of(Y, "matrix-mesh")
    v = velocities_of(Y, key, "progressive_moving")
    c = pkg.backend.Context(0)
    try:
        GL.upload(c, scene)
        tick(pkg, c, "progressive_moving", v, True)
        assert info(c) == (1, 1)
        tick(pkg, c, "progressive_camera", v, True)
        assert info(c) == (1, 1)
        tick(pkg, c, "converging_camera", v, True)
        assert info(c) == (1, 1)
        tick(pkg, c, "converging_motion", velocities_of(Y, key, "converging_motion"), True)
        assert info(c) == (1, 2)
        tick(pkg, c, "progressive_camera", v)
        assert info(c) == (1, 3)
    finally:
        c.close()


def test_ticks_that_walk_flat_say_so(pkg, Y, monkeypatch):
    """walked_swept is 0 after a camera tick without velocities (the static scene's kernels keep the image's own hierarchy),
    after a plain progressive tick, and on an image without a hierarchy; a refused tick builds nothing."""
    key, scene = GSW.scene_of(Y, "matrix-spheres")
    v = velocities_of(Y, key, "progressive_camera")
    c = pkg.backend.Context(0)
    try:
        GL.upload(c, scene)
        tick(pkg, c, "progressive_camera", v, True)
        assert info(c) == (1, 1)
        tick(pkg, c, "progressive_camera", None, True)                  # velocities=None
        assert info(c) == (0, 1)
        tick(pkg, c, "converging_camera", v, True)
        assert info(c) == (1, 1)
        tick(pkg, c, "converging_camera", None, True)
        assert info(c) == (0, 1)
        tick(pkg, c, "progressive_motion", velocities_of(Y, key, "progressive_motion"), True)
        assert info(c) == (1, 2)
        c.render_progressive(params(pkg), VM.APERTURE, VM.FOCUS, 5, restart=True)   # a plain tick
        assert info(c) == (0, 2)
        # a velocity on a polygon: the moving spheres' ticks refuse it, and build nothing for it
        kinds = Y.kinds(key)
        bad = np.zeros((len(kinds), 3))
        polygon = list(kinds).index(MV.ORC_POLYGON)
        bad[polygon] = (1., 0., 0.)
        for family in ("progressive_motion", "converging_motion"):
            with pytest.raises(pkg._lib.BackendError, match=r"velocities\[%d\] is not zero and shape %d is not a sphere" % (polygon, polygon)):
                tick(pkg, c, family, bad, True)
            assert info(c) == (0, 2)
        tick(pkg, c, "progressive_camera", bad, True)                   # ... which the camera's ticks obey
        assert info(c) == (1, 3)
    finally:
        c.close()
    # an image without a hierarchy: the demo's if it holds none, else any under RM_DISABLE_BVH=1
    dkey, demo = GSW.scene_of(Y, "demo")
    H = HR.image_of(pkg, demo)[1]["H"]
    if H["off_bvh_spheres"] or H["off_bvh_triangles"]:
        monkeypatch.setenv("RM_DISABLE_BVH", "1")
    c = pkg.backend.Context(0)
    try:
        GL.upload(c, demo)
        for family in ("progressive_camera", "converging_camera", "progressive_motion", "converging_motion"):
            tick(pkg, c, family, velocities_of(Y, dkey, family), True)
            assert info(c) == (0, 0), family
    finally:
        c.close()
