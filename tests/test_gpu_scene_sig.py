"""GPU: the plain-walk kernels' tile body compiled for the default scene's shape counts (render_tile<.., SIG>, DESIGN.md
section 4 "scene signatures") never changes a picture.  Frames of a few patches rendered by a context with the default knobs
and by one with RM_SCENE_SIG=0 (the knob is read at rm_init: a fresh context per setting) are bit-equal in the f64 frame and
in the display bytes -- the default scene and a seeded scene of the same counts, strict and fast flavours, the fixed view and
an oriented camera, depth caps 1, 2, 3, 5, 8, 10 and 18 (ray stacks 4, 8, 16 and 32), the integer and the generic power, with a classified first step and without
(RM_TILE_CLASSIFY=1 / =0) -- and every frame lies within 1e-9 a channel of the oracle: the strict frames everywhere, the fast
ones by the fast flavour's one rule (tests/tie_reference.py compare_fast: the same bound, but at pixels the oracle itself cannot
decide, each of which must carry the tie certificate of this very view).  Every near miss -- the default scene with one pinned
field changed -- renders within that bound as well, in both flavours, bit-equal between the two contexts, and its launches go
out generic: a kernel of either flavour that took the body for the signature all the same would walk the wrong number of
shapes, and fail here by its pixels.  What a launch went out with is read off the context itself (rmi_last_scene_sig: the
signature bits of the argument block the kernel was given), not only off a plan made beside it."""
import ctypes as C
import os

import numpy as np
import pytest

import workloads
import scene_sig_scenes as S
import tie_reference as TR
from test_gpu_camera import cam, basis_rows, view             # (cam: the oracle's frames through an oriented camera; a fixture)

pytestmark = pytest.mark.gpu

# depth cap -> frame, a few patches each: ray stacks 4 (caps to 5), 8 (to 9), 16 (to 17) and 32
SIZES = {1: (64, 32), 2: (96, 64), 3: (64, 32), 5: (96, 64), 8: (64, 32), 10: (64, 32), 18: (64, 32)}
DEPTHS = list(SIZES)
# (generic_power: an exponent that is no integer sends the launch to the kernels with the device's pow, which carry the body too)
SCENES = {"default": S.demo(), "default_moved": S.demo(camera=(2., 1., 4.)), "same_counts": S.random_same_signature(),
          "generic_power": S.demo(S.SPHERES[:1] + [("sphere",) + S.SPHERES[1][1:3] + (dict(S.GREEN, specular_exponent=12.5),)] + S.SPHERES[2:] + S.POLYGONS)}
EYE, TARGET = (9., 5., 6.), (0., -1., -12.)                                       # the oriented camera: from the right, above
KNOBS = ("RM_SCENE_SIG", "RM_TILE_CLASSIFY")


@pytest.fixture(scope="module")
def ctxs(pkg):
    """-> {classify: (context with the default knobs, context with RM_SCENE_SIG=0)}, classify in "1", "0"."""
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    old = {k: os.environ.get(k) for k in KNOBS}
    made = {}
    try:
        for classify in ("1", "0"):
            os.environ["RM_TILE_CLASSIFY"] = classify
            os.environ.pop("RM_SCENE_SIG", None)
            on = pkg.backend.Context(0)
            os.environ["RM_SCENE_SIG"] = "0"
            made[classify] = (on, pkg.backend.Context(0))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield made
    for pair in made.values():
        for c in pair:
            c.close()


_built = {}


def built(pkg, O, name, what):
    if name not in _built:
        _built[name] = S.build(pkg, O, what)
    return _built[name]


_oracle_frames = {}


def oracle_frame(O, key, oscene, w, h, depth):
    if key not in _oracle_frames:
        frame = O.render(oscene, w, h, fov=workloads.FOV, max_depth=depth)
        frame.setflags(write=False)
        _oracle_frames[key] = frame
    return _oracle_frames[key]


def launched_sig(pkg, c):
    """-> (the signature in the argument block of the context's last render launch, the resident image's)."""
    f = pkg.lib().rmi_last_scene_sig
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    launched, resident = C.c_uint32(99), C.c_uint32(99)
    assert f(c.ptr, C.byref(launched), C.byref(resident)) == 0
    return launched.value, resident.value


def render_pair(pkg, pair, scene, w, h, depth, fast, oriented=None, sig=1):
    """-> [(f64 frame, display bytes)] of the two contexts (the default knobs, RM_SCENE_SIG=0).  Both launches of each -- the
    f64 frame's and the display bytes' -- must have gone out with the signature `sig` in the first context and with none in the
    second, over a resident image whose signature is `sig`."""
    out = []
    for c, want in zip(pair, (sig, 0)):
        c.upload(scene.flatten())
        if oriented is not None:
            c.set_camera(oriented[0])
        c.orient(None if oriented is None else oriented[1])
        p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)
        p.flags = pkg._lib.RM_FLAG_FAST_FP if fast else 0
        frame = np.zeros((h, w, 3), dtype=np.float64)
        c.render(p, frame)
        assert launched_sig(pkg, c) == (want, sig), "the f64 frame's launch carried %s" % (launched_sig(pkg, c),)
        disp = np.zeros(h * w * 3, dtype=np.uint8)
        c.render_display(p, disp)
        assert launched_sig(pkg, c) == (want, sig), "the display frame's launch carried %s" % (launched_sig(pkg, c),)
        out.append((frame, disp))
    return out


def assert_bit_equal(rs, label):
    same = rs[0][0].view(np.uint64) == rs[1][0].view(np.uint64)
    assert same.all(), "%s: %d values differ between the default and RM_SCENE_SIG=0" % (label, int((~same).sum()))
    assert np.array_equal(rs[0][1], rs[1][1]), "%s: display bytes differ between the default and RM_SCENE_SIG=0" % label


@pytest.mark.parametrize("classify", ["1", "0"])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name", list(SCENES))
def test_fixed_view_bit_equal_and_on_the_oracle(pkg, O, ctxs, name, depth, classify):
    scene, oscene = built(pkg, O, name, SCENES[name])
    w, h = SIZES[depth]
    assert S.plan_verdict(pkg, scene, depth)[1] == 1, "%s: the launch carries no signature" % name
    rs = render_pair(pkg, ctxs[classify], scene, w, h, depth, fast=False)
    assert_bit_equal(rs, "%s d%d" % (name, depth))
    ref = oracle_frame(O, (name, w, h, depth), oscene, w, h, depth)
    err = float(np.abs(rs[0][0] - ref).max())
    print("%s d%d classify=%s: max |delta| vs oracle %.3e, lit %d" % (name, depth, classify, err, int((rs[0][0].sum(axis=2) > 0).sum())))
    assert err <= 1e-9, "%s d%d: %g off the oracle" % (name, depth, err)
    assert rs[0][0].any()
    fs = render_pair(pkg, ctxs[classify], scene, w, h, depth, fast=True)
    assert_bit_equal(fs, "%s d%d (fast)" % (name, depth))
    TR.compare_fast(fs[0][0], ref, 1e-9, TR.Tie(oscene, w, h, depth), "%s d%d (fast)" % (name, depth))


@pytest.mark.parametrize("classify", ["1", "0"])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name", ["default", "same_counts", "generic_power"])
def test_oriented_view_bit_equal_and_on_the_oracle(pkg, O, ctxs, cam, name, depth, classify):
    scene, oscene = built(pkg, O, name, SCENES[name])
    w, h = SIZES[depth]
    eye, basis = view(pkg, EYE, TARGET)
    rs = render_pair(pkg, ctxs[classify], scene, w, h, depth, fast=False, oriented=(eye, basis))
    assert_bit_equal(rs, "%s d%d oriented" % (name, depth))
    ref = cam.frame("scene_sig_" + name, oscene, eye, basis_rows(basis), w, h, depth)
    err = float(np.abs(rs[0][0] - ref).max())
    print("%s d%d oriented classify=%s: max |delta| vs oracle %.3e, lit %d" % (name, depth, classify, err, int((rs[0][0].sum(axis=2) > 0).sum())))
    assert err <= 1e-9, "%s d%d oriented: %g off the oracle" % (name, depth, err)
    assert rs[0][0].any()
    fs = render_pair(pkg, ctxs[classify], scene, w, h, depth, fast=True, oriented=(eye, basis))
    assert_bit_equal(fs, "%s d%d oriented (fast)" % (name, depth))
    TR.compare_fast(fs[0][0], ref, 1e-9, TR.Tie(oscene, w, h, depth, eye=eye, basis=basis_rows(basis)), "%s d%d oriented (fast)" % (name, depth))


@pytest.mark.parametrize("name", list(S.NEAR_MISSES))
def test_near_misses_render_generic_and_right(pkg, O, ctxs, name):
    scene, oscene = built(pkg, O, "miss_" + name, S.NEAR_MISSES[name])
    w, h, depth = 96, 64, 5
    assert S.plan_verdict(pkg, scene, depth)[:2] == (0, 0), "%s: its plan carries a signature" % name
    for classify in ("1", "0"):
        rs = render_pair(pkg, ctxs[classify], scene, w, h, depth, fast=False, sig=0)
        assert_bit_equal(rs, name)
        ref = oracle_frame(O, ("miss", name), oscene, w, h, depth)
        err = float(np.abs(rs[0][0] - ref).max())
        print("%s classify=%s: max |delta| vs oracle %.3e, lit %d" % (name, classify, err, int((rs[0][0].sum(axis=2) > 0).sum())))
        assert err <= 1e-9, "%s: %g off the oracle" % (name, err)
        assert rs[0][0].any()
        fs = render_pair(pkg, ctxs[classify], scene, w, h, depth, fast=True, sig=0)
        assert_bit_equal(fs, name + " (fast)")
        TR.compare_fast(fs[0][0], ref, 1e-9, TR.Tie(oscene, w, h, depth), name + " (fast)")


def test_the_scenes_show_what_the_body_walks(pkg, O):
    """The frames above are not sky: by the oracle's own closest-hit search the default view's 96x64 frame meets spheres, the
    triangle and the quad, so every unrolled walk of the body decides pixels of it."""
    _, oscene = built(pkg, O, "default", SCENES["default"])
    L, c = O.lib(), oscene.c
    r = L.orc_create_renderer(workloads.FOV, 64., 96.)
    seen = set()
    for y in range(64):
        for x in range(96):
            d = L.orc_normalized(L.orc_backproject(C.byref(r), x, y))
            its, which = O.Intersection(), C.c_uint8(0)
            if L.orc_find_closest_intersect(c.camera, d, c.shapes, c.n_shapes, C.byref(its), C.byref(which)):
                seen.add(int(which.value))
    print("shapes met by primary rays:", sorted(seen))
    assert {0, 4, 5} <= seen and len(seen & {1, 2, 3}) >= 2
