"""The fast flavour on the frames where ties exist, and on their tie-free neighbours (-m gpu).

tests/test_tie_reference.py freezes, on the oracle alone, where the reference cannot decide a pixel: the demo scene seen from
(0, 5, 0) has a line of rays in the plane of a triangle edge, and nothing else the suite's sweep renders has any.  Here
RM_FLAG_FAST_FP renders those frames four ways -- a plain context, a context with the tile classification and the dispatch
order forced (test_gpu_parity's ctx_order_forced), a context made under RM_DISABLE_BVH=1, and the oriented kernels
(namespace rmdev_fast_o) -- and every frame is held to the certificate of tests/tie_reference.py: it differs from orc_render
only at unstable pixels, and shows a colour of the pixel's family there.  The four frames must be equal bit for bit.  The same
shapes from the two tie-free cameras may differ nowhere.

The oriented kernels cannot be given the identity itself: rm_camera_orient takes a basis equal to it for the fixed view.  The
basis here has right = (1, 0, 2^-1000): it passes rm_camera_basis_check, is not the identity, and (bx * right + by * up) +
forward gives backproject's own (bx, by, -1) value for value -- 2^-1000 bx vanishes against -1; the centre row's y is +0
where backproject leaves -0, which the oracle's outcomes do not see -- so orc_render stays the reference.

Seeded random scenes with a tie below the first hit were searched for and not found (tests/test_tie_reference.py), so none
is rendered here.

Measured on an MI355X, differing pixels of the fast flavour / unstable pixels, the same pixels in all four ways: 2 / 5 at
64x32, 1 / 16 at 224x96, 5 / 28 at 352x224, every one certified; 0 from the tie-free cameras."""
import numpy as np
import pytest

import test_gpu_camera as GC
import test_tie_reference as TT
import tie_reference as TR
import workloads
from test_gpu_render_matrix import contexts                          # noqa: F401 (the fixture: one context per environment)

pytestmark = pytest.mark.gpu

RM_FLAG_FAST_FP = 2
DEPTH = TT.DEPTH
SHAPES = [(64, 32), (224, 96), (352, 224)]
ORDER_FORCED = {"RM_TILE_CLASSIFY": "1", "RM_PATCH_ORDER": "1", "RM_FIRST_ROUND": "0"}
NEARLY_FIXED = ((1., 0., 2. ** -1000), (0., 1., 0.), (0., 0., -1.))
# way -> (the environment its context is made under, the basis)
WAYS = {"plain": ({}, None), "order forced": (ORDER_FORCED, None), "no hierarchy": ({"RM_DISABLE_BVH": "1"}, None),
        "oriented": (ORDER_FORCED, NEARLY_FIXED)}
REPORT = []


def four_ways(pkg, O, contexts, camera, w, h, ties):
    """The fast flavour's frame of the demo scene from `camera`, rendered the four ways and held to orc_render -- at certified
    ties where `ties`, nowhere else.  -> the differing pixels (x, y)."""
    scene, oscene = workloads.product_scene(pkg, "demo"), workloads.oracle_scene(O, "demo")
    oscene.set_camera(camera)
    ref = O.render(oscene, w, h, max_depth=DEPTH)
    frames, differing = {}, {}
    for way, (env, basis) in WAYS.items():
        ctx = contexts(env)
        ctx.upload(scene.flatten())
        GC.set_view(ctx, camera, basis)
        try:
            p = pkg.backend.make_params(workloads.FOV, float(h), float(w), DEPTH)
            p.flags = RM_FLAG_FAST_FP
            name = ctx.kernel_name(p)
            assert name.startswith("rmdev_fast_o::" if basis else "rmdev_fast::"), (way, name)
            got = GC.device_frame(ctx, p)
        finally:
            ctx.orient(None)
        label = "demo from %s %dx%d, %s" % (camera, w, h, way)
        assert not (got == -1.).any(), "%s: a pixel was left out" % label
        tie = TR.Tie(oscene, w, h, DEPTH, eye=camera, basis=basis) if ties else None
        _, n_bad = TR.compare_fast(got, ref, tie=tie, label=label)
        frames[way] = got
        bad = np.flatnonzero((np.abs(got - ref).reshape(-1, 3) >= TR.TIGHT).any(axis=1))
        differing[way] = [(int(i) % w, int(i) // w) for i in bad]
        assert len(bad) == n_bad
        print("%s: %s, %d differing pixels" % (label, name, n_bad))
    for way, got in frames.items():
        assert got.tobytes() == frames["plain"].tobytes(), "demo from %s %dx%d: the %s frame differs from the plain one in %d values" % (
            camera, w, h, way, int((got != frames["plain"]).sum()))
    return differing["plain"]


@pytest.mark.parametrize("w,h", SHAPES)
def test_tie_rich_frames_differ_only_at_certified_ties(pkg, O, contexts, w, h):
    unstable = TT.UNSTABLE[(w, h)]
    assert unstable and (w, h) in TT.CERTIFIED_ON and len(unstable) <= TR.MAX_UNSTABLE_SHARE * w * h
    differing = four_ways(pkg, O, contexts, TT.TIE_CAMERA, w, h, ties=True)
    REPORT.append("demo from %s %dx%d: %d unstable pixels, %d differing: %s" % (TT.TIE_CAMERA, w, h, len(unstable), len(differing), differing))
    print(REPORT[-1])
    assert set(differing) <= set(unstable)


@pytest.mark.parametrize("camera", [TT.SWEEP_CAMERAS[0], TT.SWEEP_CAMERAS[2]])
@pytest.mark.parametrize("w,h", SHAPES)
def test_tie_free_frames_differ_nowhere(pkg, O, contexts, w, h, camera):
    differing = four_ways(pkg, O, contexts, camera, w, h, ties=False)
    REPORT.append("demo from %s %dx%d: no unstable pixel, %d differing" % (camera, w, h, len(differing)))
    print(REPORT[-1])
    assert not differing


def test_report():
    """Last: the counts per frame, in one place."""
    for line in REPORT:
        print(line)
