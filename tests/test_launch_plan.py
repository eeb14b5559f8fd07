"""CPU checks of the render launch's plan (rm_plan.cpp plan_launch): the state machine of a stream's launches -- which
launch dispatches by whose order, which launches are frozen, when a view or an order key starts afresh, what the patches are
ordered by, when the tags wrap and what is cleared then, how the sky tail follows the hint, and the launch shapes of the
benchmark's configurations.  The planner touches no device: rmi_plan_launches (an internal export, not part of the ABI) plans
a sequence of launches on one imaginary stream and commits each plan's "state after" itself.  Expected values are the rules
the planner's comments state, worked out here by hand; the shapes of C2 / C3 / C5 were read off the launches of the commit
before the planner existed, on a device of 256 compute units.

Behind them the two decisions of a shading launch (rmi_shading_launch): which instantiation of the shading kernels a scene and a
depth cap take, and how many workgroups a frame gets."""
import ctypes as C

import pytest

import workloads

PLACE, COST, CONTENT = 0, 1, 2                     # RM_KEY_*
CLEAR_NONE, CLEAR_FLAT, CLEAR_ALL = 0, 1, 2
FIXED = ((1., 0., 0.), (0., 1., 0.), (0., 0., -1.))
DEMO = dict(n_spheres=4, n_polygons=2, n_triangles=0, total_words=264, bvh=0)          # 6 primitives: classified at the launch's head
CORNELL = dict(n_spheres=0, n_polygons=0, n_triangles=36, total_words=1884, bvh=1)
SYNTH = dict(n_spheres=256, n_polygons=1, n_triangles=0, total_words=6254, bvh=1)
# the GPU tests' way to an order in frames of a few thousand tiles
ENV = {"RM_PATCH_ORDER": "1", "RM_TILE_CLASSIFY": "1", "RM_FIRST_ROUND": "256"}
# 640x352: 220 patches, 3,520 tiles; the first round is two rounds of 256 waves = 32 patches, 188 patches have a place in the order
N_STATIC, N_DYN, CLS = 512, 188, 55


class StreamState(C.Structure):
    _fields_ = [("order_frames", C.c_uint32), ("order_key", C.c_uint64 * 3), ("list_tag", C.c_uint32 * 2), ("static_read", C.c_int),
                ("static_written", C.c_int), ("last_tag", C.c_uint32), ("seq", C.c_uint32), ("view_seq0", C.c_uint32),
                ("key_seq0", C.c_uint32), ("ord_tag", C.c_uint32), ("view", C.c_double * 16), ("tag", C.c_uint32),
                ("tagged_tiles", C.c_uint32), ("tagged_scene", C.c_uint64), ("tagged", C.c_bool), ("frozen_run", C.c_uint32)]


ROW_FIELDS = ("grid block lds_bytes fast stack pow_mode waves per_wave staged bvh cull edges order feedback classify classify_in_front "
              "ordered frozen clear_masks order_patches order_clear n_tiles cls_blocks cls_iters n_static tail_patches ov_cap key_mode "
              "mask_tag mask_tag_prev ord_tag ord_read_tag launch_seq reads_own_order late_places").split()


class Row(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ROW_FIELDS] + [("after", StreamState)]


def state(row):
    s = row.after
    return {n: (list(getattr(s, n)) if hasattr(getattr(s, n), "__len__") else getattr(s, n)) for n, _ in StreamState._fields_}


def launch(scene=DEMO, cam=(0., 0., 0.), w=640, h=352, depth=5, band=None, basis=None, epoch=1, hint=0):
    return dict(scene=scene, cam=cam, w=w, h=h, depth=depth, band=band, basis=basis, epoch=epoch, hint=hint)


def plan(pkg, launches, n_cus=256, integer_exponents=1):
    """-> one Row per launch of the sequence, planned on one stream with the knobs of the environment as it is now.
    integer_exponents: the scene image's verdict (0: the launches take POW_GENERIC); a launch may carry rm_params' "flags"."""
    L = pkg.lib()

    class Case(C.Structure):
        _fields_ = [(n, C.c_uint32) for n in "n_spheres n_polygons n_triangles total_words bvh integer_exponents oriented n_cus".split()] + \
                   [("scene_epoch", C.c_uint64), ("params", pkg._lib.rm_params), ("camera", pkg._lib.rm_vec3),
                    ("basis", pkg._lib.rm_camera_basis), ("hint", C.c_uint64)]

    cases = (Case * len(launches))()
    for c, l in zip(cases, launches):
        for k, v in l["scene"].items():
            setattr(c, k, v)
        c.integer_exponents, c.n_cus, c.scene_epoch, c.hint = integer_exponents, n_cus, l["epoch"], l["hint"]
        c.oriented = 0 if l["basis"] is None else 1
        c.params = pkg.backend.make_params(workloads.FOV, float(l["h"]), float(l["w"]), l["depth"], l["band"])
        c.params.flags = l.get("flags", c.params.flags)
        c.camera = pkg._lib.vec3(l["cam"])
        c.basis = pkg._lib.camera_basis(FIXED if l["basis"] is None else l["basis"])
    rows = (Row * len(launches))()
    f = L.rmi_plan_launches
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    assert f(C.addressof(cases), len(launches), C.addressof(rows)) == 0
    return list(rows)


def plan_with_counts(pkg, launches, n_lit):
    """As plan(), with the hint a device would have left: before launch i the host reads (launch_seq << 32) | n_lit[j] of the
    last launch j < i that classified (a frozen launch writes none).  Which launches classify does not depend on the hint."""
    rows = plan(pkg, launches)
    hinted, last = [], 0
    for i, l in enumerate(launches):
        hinted.append(dict(l, hint=last))
        if rows[i].cls_blocks:
            last = (rows[i].launch_seq << 32) | n_lit[i]
    return plan(pkg, hinted)


def expected_grid(r, n_static=N_STATIC, n_dyn=N_DYN):
    return r.cls_blocks + n_static + 16 * (n_dyn - r.tail_patches) + r.tail_patches + 16 * r.ov_cap + (r.cls_blocks if r.late_places else 0)


@pytest.fixture
def env(monkeypatch):
    """env(**knobs): the environment holds ENV and these knobs, and none of an earlier call's."""
    extra = []

    def set_env(**knobs):
        for k in extra:
            monkeypatch.delenv(k)
        extra[:] = [k for k in knobs if k not in ENV]
        for k, v in dict(ENV, **knobs).items():
            monkeypatch.setenv(k, v)
    return set_env


def test_standing_view_reuses_then_freezes(pkg, env):
    env()
    before = [state(r) for r in plan(pkg, [launch()] * 29)]
    rows = plan_with_counts(pkg, [launch()] * 30, [100] * 30)
    for i, r in enumerate(rows):
        assert (r.classify, r.classify_in_front, r.ordered, r.n_static, r.n_tiles) == (1, 0, 1, N_STATIC, 3520), i
        assert r.grid == expected_grid(r), i
        # launches 1-3 of the view dispatch by their own order; from the fourth on by the predecessor's, whose words they take
        assert r.reads_own_order == (1 if i < 3 else 0), i
        assert (r.mask_tag_prev != 0) == (i >= 3), i
        assert r.late_places == (1 if i >= 3 and not r.frozen else 0), i
        assert r.key_mode == (PLACE if i == 0 else COST), i
    # order_freeze = 7: from the view's fifth launch on, seven frozen launches, one that classifies, seven more, ...
    assert [r.frozen for r in rows] == [0] * 4 + ([1] * 7 + [0]) * 3 + [1] * 2
    seq = 0
    for i, r in enumerate(rows):
        if r.frozen:
            assert (r.cls_blocks, r.cls_iters) == (0, 0) and r.grid == N_STATIC + 16 * (N_DYN - r.tail_patches) + r.tail_patches + 16 * r.ov_cap
            assert r.mask_tag == r.mask_tag_prev == rows[i - 1].after.tag
            assert (r.clear_masks, r.order_clear) == (0, CLEAR_NONE)
            # the state after is the state before, but for the count of frozen launches
            was, now = before[i - 1], state(r)
            assert now.pop("frozen_run") == was.pop("frozen_run") + 1 and now == was, i
        else:
            seq += 1
            assert (r.cls_blocks, r.cls_iters, r.launch_seq, r.after.frozen_run) == (CLS, 1, seq, 0), i
            assert r.mask_tag_prev == (r.mask_tag - 1 if i >= 3 else 0)
    # the launch that classifies after a frozen run is set up as if the run had not been
    assert (rows[11].launch_seq, rows[11].ord_tag, rows[11].mask_tag, rows[11].ord_read_tag) == (5, 5, 5, 4)


def test_freeze_knob_and_its_conditions(pkg, env):
    env(RM_ORDER_FREEZE="0")
    assert not any(r.frozen for r in plan(pkg, [launch()] * 20))
    env(RM_ORDER_FREEZE="2")
    assert [r.frozen for r in plan(pkg, [launch()] * 11)] == [0] * 4 + [1, 1, 0, 1, 1, 0, 1]
    # a frozen launch takes its predecessor's words, order and places, and nothing may look at what it does not lay out
    for knob in ({"RM_MASK_REUSE": "0"}, {"RM_ORDER_LATE_PLACES": "0"}, {"RM_ORDER_REUSE": "0"}, {"RM_SKY_TAIL_FORCE": "37"},
                 {"RM_TEST_STALL_ORDER": "2"}, {"RM_DEBUG_TAIL": "1"}):
        env(**knob)
        assert not any(r.frozen for r in plan(pkg, [launch()] * 12)), knob


TURNED = ((0., 0., -1.), (0., 1., 0.), (-1., 0., 0.))   # the fixed view yawed by a quarter turn


@pytest.mark.parametrize("change, fresh_key", [
    (dict(cam=(0., 5., 0.)), False), (dict(basis=TURNED), False), (dict(depth=4), False),
    (dict(w=800, h=608), True), (dict(band=(2, 9, 1)), True), (dict(epoch=2), True)])
def test_a_change_ends_reuse_and_freeze_at_once(pkg, env, change, fresh_key):
    """A moved camera, a turned basis: a new view (view_seq0).  Another frame size, band or scene: a new order key -- the
    order block is cleared whole and its launches are counted from zero.  (The depth cap is in neither: nothing changes.)"""
    env()
    rows = plan(pkg, [launch()] * 7 + [launch(**change)] * 12)
    assert [r.frozen for r in rows[:7]] == [0, 0, 0, 0, 1, 1, 1]
    r = rows[7]
    if "depth" in change:
        assert r.frozen == 1 and r.reads_own_order == 0
        return
    assert (r.frozen, r.reads_own_order, r.mask_tag_prev, r.late_places) == (0, 1, 0, 0)
    assert r.after.view_seq0 == r.launch_seq == 5 and r.after.frozen_run == 0
    if fresh_key:
        assert (r.order_clear, r.after.order_frames, r.after.key_seq0, r.key_mode, r.ord_tag) == (CLEAR_ALL, 1, 5, PLACE, 1)
        # (another number of tiles or another scene: the tagged classification words start afresh too)
        assert (r.clear_masks, r.mask_tag) == (1, 1)
    else:
        assert (r.order_clear, r.after.order_frames, r.after.key_seq0, r.key_mode, r.clear_masks) == (CLEAR_NONE, 5, 1, CONTENT, 0)
    # ... and the new view goes through the same steps: its fourth launch is the first to reuse -- and, being at least the
    # fifth of its key (f >= 4), the first frozen; under a new key that is the view's fifth
    assert [x.reads_own_order for x in rows[7:13]] == [1, 1, 1, 0, 0, 0]
    assert [x.frozen for x in rows[7:]] == ([0] * 4 + [1] * 7 + [0] if fresh_key else [0] * 3 + [1] * 7 + [0, 1])
    assert all(x.after.view_seq0 == 5 for x in rows[7:])


def test_key_mode(pkg, env):
    seq = [launch()] * 3 + [launch(cam=(1., 0., 0.))] * 2 + [launch(cam=(2., 0., 0.))]
    env()
    assert [r.key_mode for r in plan(pkg, seq)] == [PLACE, COST, COST, CONTENT, COST, CONTENT]
    env(RM_ORDER_KEYS="0")
    assert [r.key_mode for r in plan(pkg, seq)] == [PLACE] * 6
    env(RM_ORDER_KEYS="1")
    assert [r.key_mode for r in plan(pkg, seq)] == [PLACE, COST, COST, PLACE, COST, PLACE]
    env(RM_ORDER_KEYS="2")
    assert [r.key_mode for r in plan(pkg, seq)] == [PLACE] + [CONTENT] * 5
    # words that are not exact (more than 56 primitives at the launch's head) cannot be ordered by content
    env(RM_CLASSIFY_IN_LAUNCH_PRIMS="100")
    many = dict(DEMO, n_spheres=60)
    assert [r.key_mode for r in plan(pkg, [dict(l, scene=many) for l in seq])] == [PLACE, COST, COST, PLACE, COST, PLACE]


def test_tags_wrap_and_clears(pkg, env):
    env(RM_ORDER_FREEZE="0")
    rows = plan(pkg, [launch()] * 2100)
    # the classification words' tag: 1..255, then the words are cleared and it starts again
    assert [r.mask_tag for r in rows[:600]] == (list(range(1, 256)) * 3)[:600]
    assert [i for i, r in enumerate(rows) if r.clear_masks] == list(range(0, 2100, 255))
    assert all(r.mask_tag_prev == (r.mask_tag - 1 if i >= 3 and r.reads_own_order == 0 else 0) for i, r in enumerate(rows))
    # the order's tag: 1..2^11 - 1; the whole block is cleared for a new key only, the two orders when the tags are used up
    assert [r.ord_tag for r in rows] == (list(range(1, 2048)) * 2)[:2100]
    assert [(i, r.order_clear) for i, r in enumerate(rows) if r.order_clear] == [(0, CLEAR_ALL), (2047, CLEAR_FLAT)]
    assert [r.order_patches for r in rows] == [220] * 2100
    # (no order of the old tags to dispatch by: the launch after a wrap reads its own)
    assert [r.reads_own_order for r in rows[2045:2050]] == [0, 0, 1, 0, 0] and rows[2047].ord_read_tag == 1
    env(RM_ORDER_FREEZE="0", RM_ORD_TAG_WRAP="3")
    rows = plan(pkg, [launch()] * 10)
    assert [r.ord_tag for r in rows] == [1, 2, 3, 1, 2, 3, 1, 2, 3, 1]
    assert [r.order_clear for r in rows] == [CLEAR_ALL, 0, 0, CLEAR_FLAT, 0, 0, CLEAR_FLAT, 0, 0, CLEAR_FLAT]
    assert [r.reads_own_order for r in rows] == [1, 1, 1, 1, 0, 0, 1, 0, 0, 1]


def test_sky_tail_follows_the_hint(pkg, env):
    def tails(n_lit, n=4, **knobs):
        env(**knobs)
        rows = plan_with_counts(pkg, [launch()] * n, [n_lit] * n)
        assert all(r.grid == expected_grid(r) for r in rows)
        return [(r.tail_patches, r.ov_cap) for r in rows]
    # no hint yet; then the view's first launch's count, a guess (room max(768, patches / 16), at most the tail); then exact (room 32)
    assert tails(100) == [(0, 0), (88, 88), (88, 32), (88, 32)]
    assert tails(100, RM_SKY_TAIL_MOTION="0") == [(0, 0), (0, 0), (88, 32), (88, 32)]
    assert tails(180) == [(0, 0), (8, 8), (8, 8), (8, 8)]
    assert tails(181) == [(0, 0)] * 4                                   # tails under 8 are dropped
    assert tails(189) == [(0, 0)] * 4                                   # more than there are places: not a valid hint
    assert tails(100, RM_SKY_TAIL_CAP="5") == [(0, 0), (88, 5), (88, 5), (88, 5)]
    assert tails(100, RM_SKY_TAIL_CAP="0") == [(0, 0), (88, 0), (88, 0), (88, 0)]
    assert tails(100, RM_SKY_TAIL="0") == [(0, 0)] * 4
    assert tails(100, RM_SKY_TAIL_FORCE="37") == [(37, 37)] * 4     # (test hook: taken for a guess)
    assert tails(100, RM_SKY_TAIL_FORCE="1000") == [(188, 188)] * 4
    assert tails(100, RM_SKY_TAIL_FORCE="37", RM_SKY_TAIL_CAP="10") == [(37, 10)] * 4
    # a hint from before the order's key (another frame size), from this launch or a later one, or none: no tail
    env()
    stale = plan(pkg, [launch(w=800, h=608)] * 2 + [launch(hint=(2 << 32) | 100)] + [launch(hint=(4 << 32) | 100), launch(hint=(5 << 32) | 100),
                                                                                      launch(hint=(4 << 32) | 100), launch(hint=100)])
    assert [r.launch_seq for r in stale] == [1, 2, 3, 4, 5, 6, 7] and stale[2].after.key_seq0 == 3
    assert [r.tail_patches for r in stale] == [0, 0, 0, 0, 0, 88, 0]
    # a moved view takes the last view's count for a guess
    moved = plan_with_counts(pkg, [launch()] * 3 + [launch(cam=(1., 0., 0.))] * 2, [100, 100, 100, 120, 120])
    assert [(r.tail_patches, r.ov_cap) for r in moved] == [(0, 0), (88, 88), (88, 32), (88, 88), (68, 68)]
    # a guess's room in a launch of many patches: patches / 16 (4096x4096: 16,384 patches, ordered by place for the tail alone)
    env(RM_FIRST_ROUND="4096")
    big = plan(pkg, [launch(w=4096, h=4096), launch(w=4096, h=4096, hint=(1 << 32) | 5000)])
    assert (big[1].n_static, big[1].key_mode, big[1].tail_patches, big[1].ov_cap) == (8192, PLACE, 16384 - 512 - 5000, 1024)
    assert big[1].grid == expected_grid(big[1], 8192, 16384 - 512) and (big[1].cls_blocks, big[1].cls_iters) == (1024, 4)


@pytest.mark.parametrize("config, scene, kernel, grid, lds", [
    ("C2", DEMO, (0, 4, 1, 1, 1, 1, 0, 0, 0, 1, 0), 32175, 8016),
    ("C3", CORNELL, (0, 4, 1, 1, 1, 0, 1, 1, 1, 1, 0), 32175, 7536),
    ("C5", SYNTH, (0, 16, 1, 1, 1, 0, 1, 1, 0, 1, 0), 263168, 8592)])
def test_benchmark_launch_shapes(pkg, config, scene, kernel, grid, lds):
    """rmdev_strict::rm_render_static<stack, pow, waves, tiles per wave, STAGED, BVH, CULL, EDGES, ORDER, FEEDBACK>, the grid and
    the LDS bytes of the configuration's first launch on 256 compute units, with no knob set."""
    cfg = workloads.CONFIGS[config]
    r = plan(pkg, [launch(scene=scene, w=cfg["width"], h=cfg["height"], depth=cfg["max_depth"])])[0]
    assert (r.fast, r.stack, r.pow_mode, r.waves, r.per_wave, r.staged, r.bvh, r.cull, r.edges, r.order, r.feedback) == kernel
    assert (r.grid, r.block, r.lds_bytes) == (grid, 64, lds)


# ---------------------------------------------------------------- the shading launches (rm_plan.cpp rm_shading_variant_of, rm_shading_grid)
POW_GENERIC, POW_INTEGER = 0, 1
RM_MAX_DEPTH = 32
HEADER_WORDS = 19                                  # rm_dev_header's integer fields (tests/test_scene_image.py HEADER_FIELDS)
OFF_BVH_SPHERES, OFF_BVH_TRIANGLES = 13, 14


def shading_hook(pkg):
    return pkg.lib().rmi_shading_launch            # (an internal export like rmi_plan_launches; its prototype is _lib.py's)


def shading_variant(pkg, header, integer_exponents, max_depth):
    """-> (bvh, pow_mode, stack) of a shading launch: header = rm_dev_header's 19 integer fields in their order."""
    assert len(header) == HEADER_WORDS
    out = (C.c_uint32 * 3)()
    assert shading_hook(pkg)((C.c_uint32 * HEADER_WORDS)(*header), int(integer_exponents), max_depth, out, 0, 0, 0, 0, 0, None) == 0
    return bool(out[0]), int(out[1]), int(out[2])


def shading_grid(pkg, total, rays_per_pixel, n_cus, per_cu, max_blocks):
    out = C.c_uint32(0xFFFFFFFF)
    assert shading_hook(pkg)(None, 0, 0, None, total, rays_per_pixel, n_cus, per_cu, max_blocks, C.byref(out)) == 0
    return out.value


def header_with(spheres=0, triangles=0):
    h = [0] * HEADER_WORDS
    h[OFF_BVH_SPHERES], h[OFF_BVH_TRIANGLES] = spheres, triangles
    return h


def test_shading_variant_outcomes(pkg, monkeypatch):
    for k in ("RM_FORCE_GENERIC_POW", "RM_FORCE_STACK"):
        monkeypatch.delenv(k, raising=False)
    # the eight (bvh, pow, stack) outcomes, both sides of the depth rule at 5 and 6
    for spheres in (0, 1024):
        for integer in (False, True):
            for depth in (5, 6):
                assert shading_variant(pkg, header_with(spheres), integer, depth) == \
                    (spheres != 0, POW_INTEGER if integer else POW_GENERIC, 4 if depth <= 5 else 32)
    # ... and its ends
    assert shading_variant(pkg, header_with(), True, 0) == (False, POW_INTEGER, 4)
    assert shading_variant(pkg, header_with(), True, RM_MAX_DEPTH) == (False, POW_INTEGER, 32)
    # each hierarchy alone and both together
    assert [shading_variant(pkg, header_with(s, t), True, 5)[0] for s, t in ((0, 0), (512, 0), (0, 768), (512, 768))] == [False, True, True, True]
    # no other field of the header is looked at
    others = [7 if i not in (OFF_BVH_SPHERES, OFF_BVH_TRIANGLES) else 0 for i in range(HEADER_WORDS)]
    assert shading_variant(pkg, others, True, 5) == (False, POW_INTEGER, 4)


def test_shading_variant_knobs(pkg, monkeypatch):
    monkeypatch.delenv("RM_FORCE_STACK", raising=False)
    for forced, expect in (("1", POW_GENERIC), ("0", POW_INTEGER)):
        monkeypatch.setenv("RM_FORCE_GENERIC_POW", forced)
        assert shading_variant(pkg, header_with(), True, 5)[1] == expect
        assert shading_variant(pkg, header_with(), False, 5)[1] == POW_GENERIC
    monkeypatch.delenv("RM_FORCE_GENERIC_POW")
    # RM_FORCE_STACK is the render kernels' alone: the shading kernels come with 4 and 32 parked rays only
    before = [shading_variant(pkg, header_with(s), i, d) for s in (0, 64) for i in (False, True) for d in (0, 5, 6, RM_MAX_DEPTH)]
    monkeypatch.setenv("RM_FORCE_STACK", "32")
    assert [shading_variant(pkg, header_with(s), i, d) for s in (0, 64) for i in (False, True) for d in (0, 5, 6, RM_MAX_DEPTH)] == before
    assert shading_variant(pkg, header_with(), True, 5)[2] == 4


def test_shading_grid(pkg):
    """min(ceil(total / (64 / rays_per_pixel)), max(1, n_cus) * per_cu), then the cap where it is not 0, then at least 1 -- worked
    out here, in Python's integers."""
    for rays in (1, 4, 9, 49, 64):
        for total in (1, 63, 64, 65, 2 ** 31 - 1):
            for cap in (0, 1, 3):
                for n_cus, per_cu in ((256, 8), (256, 1), (0, 5), (1, 1), (304, 3)):
                    pixels_a_group = 64 // rays
                    g = min(-(-total // pixels_a_group), max(1, n_cus) * per_cu)
                    if cap:
                        g = min(g, cap)
                    g = max(g, 1)
                    assert shading_grid(pkg, total, rays, n_cus, per_cu, cap) == g, (total, rays, n_cus, per_cu, cap)
    # a frame smaller than the device, a device smaller than the frame, and the largest frame one ray a pixel
    assert shading_grid(pkg, 32 * 32, 4, 256, 8, 0) == 64
    assert shading_grid(pkg, 1920 * 1056, 8, 256, 8, 0) == 2048
    assert shading_grid(pkg, 2 ** 31 - 1, 64, 2 ** 20, 2 ** 11, 0) == 2 ** 31 - 1
    # what the hook refuses: a group of no pixels
    assert shading_hook(pkg)(None, 0, 0, None, 64, 0, 256, 8, 0, C.byref(C.c_uint32())) == 1
    assert shading_hook(pkg)(None, 0, 0, None, 64, 65, 256, 8, 0, C.byref(C.c_uint32())) == 1
