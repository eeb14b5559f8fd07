"""Temporal reprojection on the GPU (-m gpu): rm_reproject_device through the Python binding and the C ABI against
tests/reproject_reference.py, the rule in numpy (pinned on the CPU by tests/test_reproject_reference.py).

The rule is + - * /, floor and comparisons of doubles, each rounded once, so everything here is demanded BYTE FOR BYTE: sum,
stats, count, the carried mask and the carried total, which must also be the mask's sum.  The previous frame is a real
converging frame -- three passes of 8 with area lights of radius 1.5, made by rm_accumulate_converging_device -- and both hit
buffers are rm_primary_hits_device's.  Every output stands between guards, the rows from `rows` on hold sentinels in every
buffer -- poison in the inputs, so that a tap that read one would show -- and neither may change."""
import ctypes as C

import numpy as np
import pytest

import reproject_reference as R
import workloads
from denoise_reference import HIT_DTYPE

pytestmark = pytest.mark.gpu

NAN, BYTE, WORD = float("nan"), 0xA5, 0x5a5a5a5a
GUARD = 256                                                            # elements in front of and behind every output
SIZES = [(32, 32), (72, 64), (64, 96)]                                 # (h, w): one tile row of four; 8 rows left alone; 3 x 8 tiles
SCENES = ["demo", "cornell"]
# where the previous view stands: the demo's own camera; inside the Cornell box (x 0..556, y 0..549, z -500..59 as the scene is
# built), near its closed end and looking along it -- the scene's own camera sits in a corner of the box's floor
BASES = {"demo": None, "cornell": (278., 273., 40.)}
NS, TOL, LO, HI, RADIUS = 8, 0.02, 8, 64, 1.5
DEPTH = 3
# what the current view is, from the previous one (the scene's own camera, the fixed view): a step of the position and a yaw
VIEWS = {"same": ((0., 0., 0.), 0.), "sideways": ((.25, 0., 0.), 0.), "yaw": ((0., 0., 0.), .05), "back": ((0., 0., 1.), 0.),
         "behind": ((0., 0., 0.), 0.)}                                 # behind: the scene's own view again, but the previous frame is another:
#                                                                        one from a camera that went forward by the median distance of what
#                                                                        the view sees, so about half of that lies behind the previous camera


def params(pkg, h, w):
    return pkg.backend.make_params(workloads.FOV, float(h), float(w), DEPTH)


def frame_of(p):
    return R.Frame(p.width, p.height, p.ratio, p.half_fov)


def view_of(cam):
    """tests/reproject_reference.View of what Context.camera() returned"""
    pos, b = cam[0], cam[1]
    return R.View((pos.x, pos.y, pos.z), tuple((v.x, v.y, v.z) for v in (b.right, b.up, b.forward)))


def hits_array(device_hits, h, w):
    raw = device_hits.raw if hasattr(device_hits, "raw") else device_hits
    return raw.cpu().numpy().reshape(h, w, 9).copy().view(HIT_DTYPE).reshape(h, w)


def move(pkg, c, base, step, yaw):
    """The context's camera: `base` (a position) moved by `step`, the fixed view yawed by `yaw`"""
    c.set_camera(pkg.Vec3f(base[0] + step[0], base[1] + step[1], base[2] + step[2]))
    c.orient(pkg.backend.basis_turn(pkg.backend.FIXED_VIEW, yaw=yaw) if yaw != 0. else None)


def converging_frame(c, p, n_lights, passes=3, ns=NS, lo=LO, hi=HI, tol=TOL):
    """`passes` passes of `ns` of a converging frame with area lights, from the context's camera as it stands, in buffers of the
    test's own -> (sum, stats, count, mean) tensors"""
    import torch
    h, w = p.frame_height, p.frame_width
    dev = "cuda:0"
    total, stats = torch.zeros((h, w, 3), dtype=torch.float64, device=dev), torch.zeros((h, w, 2), dtype=torch.float64, device=dev)
    count, mean = torch.zeros((h, w), dtype=torch.int32, device=dev), torch.zeros((h, w, 3), dtype=torch.float64, device=dev)
    table = torch.from_numpy(c.lens_sequence(0, hi)).to(dev)
    offsets = torch.from_numpy(c.light_sequence(0, hi, (RADIUS,) * n_lights)).to(dev)
    for k in range(passes):
        c.accumulate_converging_device(p, total, stats, count, 0., 1., ns, table, tol, lo, hi, k == 0, offsets=offsets, mean=mean)
    torch.cuda.synchronize()
    return total, stats, count, mean


class Scene:
    """A context with a scene resident, and what the tests share of it: the previous frames and hit buffers, made once a size"""

    def __init__(self, pkg, name):
        self.pkg, self.name = pkg, name
        self.c = pkg.backend.Context(0)
        scene = workloads.product_scene(pkg, name)
        self.n_lights = len(scene.lights)
        self.c.upload(scene.flatten())
        self.c.orient(None)
        pos = self.c.camera()[0]
        self.base = BASES[name] or (pos.x, pos.y, pos.z)
        self.previous, self.current = {}, {}

    def prev(self, h, w, forward=False):
        """(params, the previous view, its frame's tensors (sum, stats, count), its hits tensor) -- never written to.  The view is
        the scene's own, or with `forward` one that went forward by the median distance of what that view hits."""
        if (h, w, forward) not in self.previous:
            p = params(self.pkg, h, w)
            step = 0.
            if forward:
                seen = hits_array(self.prev(h, w)[3], h, w)[:h - h % 32]
                step = float(np.median(seen["t"][seen["hit"] != 0]))
            move(self.pkg, self.c, self.base, (0., 0., -step), 0.)
            view = self.c.camera()
            total, stats, count, _ = converging_frame(self.c, p, self.n_lights)
            hits = self.c.primary_hits_device(p).raw
            move(self.pkg, self.c, self.base, (0., 0., 0.), 0.)
            self.previous[(h, w, forward)] = (p, view, (total, stats, count), hits)
        return self.previous[(h, w, forward)]

    def cur_hits(self, h, w, name):
        if (h, w, name) not in self.current:
            step, yaw = VIEWS[name]
            move(self.pkg, self.c, self.base, step, yaw)
            self.current[(h, w, name)] = self.c.primary_hits_device(params(self.pkg, h, w)).raw
            move(self.pkg, self.c, self.base, (0., 0., 0.), 0.)
        return self.current[(h, w, name)]


@pytest.fixture(scope="module")
def scenes(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    made = {}

    def get(name):
        if name not in made:
            made[name] = Scene(pkg, name)
        return made[name]

    yield get
    for s in made.values():
        s.c.close()


_REFERENCE = {}


def reference(key, inputs, prev_hits, cur_hits, view, frame, ctl):
    """The yardstick's answer, computed once a case and shared"""
    k = (key, ctl.sigma_z, ctl.min_normal_dot, ctl.max_history)
    if k not in _REFERENCE:
        total, stats, count = (t.cpu().numpy() for t in inputs)
        h, w = count.shape
        _REFERENCE[k] = R.reproject(total, stats, count, hits_array(prev_hits, h, w), hits_array(cur_hits, h, w), view, frame, ctl)
        for a in _REFERENCE[k]:
            a.setflags(write=False)
    return _REFERENCE[k]


class Outputs:
    """The outputs of a call, each between guards and filled with sentinels"""

    def __init__(self, h, w):
        import torch
        self.h, self.w, self.rows = h, w, h - h % 32
        dev = "cuda:0"

        def guarded(count, dtype, fill):
            raw = torch.full((GUARD + count + GUARD,), fill, dtype=dtype, device=dev)
            return raw, raw[GUARD:GUARD + count]

        self.raw, self.fill = {}, {"sum": NAN, "stats": NAN, "count": WORD, "carried": BYTE, "total": WORD}
        self.raw["sum"], s = guarded(h * w * 3, torch.float64, NAN)
        self.raw["stats"], t = guarded(h * w * 2, torch.float64, NAN)
        self.raw["count"], n = guarded(h * w, torch.int32, WORD)
        self.raw["carried"], m = guarded(h * w, torch.uint8, BYTE)
        self.raw["total"], self.total = guarded(1, torch.int32, WORD)
        self.sum, self.stats, self.count, self.carried = s.view(h, w, 3), t.view(h, w, 2), n.view(h, w), m.view(h, w)

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        for name, raw in self.raw.items():
            a = raw.cpu().numpy()
            if not (np.isnan(a).all() if a.dtype == np.float64 else (a == self.fill[name]).all()):
                return False
        return True

    def results(self):
        """-> (sum, stats, count, carried, total) of the rows the call writes, after the guards and the rows beyond were found intact"""
        import torch
        torch.cuda.synchronize()
        for name, raw in self.raw.items():
            a = raw.cpu().numpy()
            for edge in (a[:GUARD], a[-GUARD:]):
                assert np.isnan(edge).all() if a.dtype == np.float64 else (edge == self.fill[name]).all(), "the guard of %s was written" % name
        s, t, n, m = (x.cpu().numpy() for x in (self.sum, self.stats, self.count, self.carried))
        r = self.rows
        assert np.isnan(s[r:]).all() and np.isnan(t[r:]).all() and (n[r:] == WORD).all() and (m[r:] == BYTE).all(), "rows beyond `rows` were written"
        return s[:r], t[:r], n[:r].view(np.uint32), m[:r], int(self.total.cpu().numpy()[0])


def poisoned(inputs, hits, rows):
    """Copies of the inputs with poison in the rows from `rows` on"""
    total, stats, count = (t.clone() for t in inputs)
    hits = hits.clone()
    total[rows:], stats[rows:], count[rows:], hits[rows:] = NAN, NAN, 7, NAN
    return (total, stats, count), hits


def same_bytes(got, want, what):
    for name, g, w in zip(("sum", "stats", "count", "carried"), got, want):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), "%s: %s differs at %d places" % (what, name, int((g != w).sum()))
    assert got[4] == int(want[3].sum()) == int(got[3].sum()), "%s: the carried total" % what


# ---------------------------------------------------------------- 1. the views, byte for byte
@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("h,w", SIZES)
def test_every_view_gives_the_yardsticks_bytes(pkg, scenes, scene, h, w):
    import torch
    s = scenes(scene)
    rows = h - h % 32
    seen = {}
    for name in VIEWS:
        p, cam, inputs, prev_hits = s.prev(h, w, forward=(name == "behind"))
        view, frame = view_of(cam), frame_of(p)
        counts = inputs[2].cpu().numpy()[:rows]
        assert counts.min() >= 8 and counts.max() <= 24                 # three passes of 8, the first over every pixel
        inputs_p, prev_p = poisoned(inputs, prev_hits, rows)
        cur = s.cur_hits(h, w, name)
        cur_p = cur.clone()
        cur_p[rows:] = NAN
        before = [t.clone() for t in inputs_p + (prev_p, cur_p)]
        for most in (1, 8, 65536):
            ctl = R.Control(max_history=most)
            out = Outputs(h, w)
            s.c.reproject_device(p, *inputs_p, prev_p, cur_p, cam, out.sum, out.stats, out.count, max_history=most, carried=out.carried,
                                 carried_total=out.total)
            got = out.results()
            want = reference((scene, h, w, name), inputs, prev_hits, cur, view, frame, ctl)
            same_bytes(got, want, "%s %dx%d %s, max_history %d" % (scene, w, h, name, most))
            assert got[2].max() <= most
            seen[(name, most)] = got
        for a, b in zip(before, inputs_p + (prev_p, cur_p)):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "an input was written"
    p, cam, inputs, prev_hits = s.prev(h, w)
    view, frame = view_of(cam), frame_of(p)
    counts = inputs[2].cpu().numpy()[:rows]
    n_hit = int((hits_array(prev_hits, h, w)[:rows]["hit"] != 0).sum())
    # the same view: every pixel that hit something carries -- its own tap is among the admitted, so no more than its own count
    same = seen[("same", 65536)]
    assert same[4] == n_hit and (same[2][same[3] == 1] <= counts[same[3] == 1]).all()
    # a step or a turn: the picture is carried
    for name in ("sideways", "yaw", "back"):
        assert 0 < seen[(name, 8)][4] <= rows * w, name
    cur = hits_array(s.cur_hits(h, w, "yaw"), h, w)[:rows]
    sx, sy, ok = R.sample_positions(cur, view, frame, w, rows)
    if scene == "demo":                                                 # (the turn brings in the left edge, which is sky in the Cornell view)
        assert ((cur["hit"] != 0) & ~ok).any()                          # pixels that left the frustum
    sx, sy, ok = R.sample_positions(hits_array(s.cur_hits(h, w, "back"), h, w)[:rows], view, frame, w, rows)
    assert (sx[ok] != np.floor(sx[ok])).mean() > .9                     # nearly every sample position is fractional
    # the previous camera had gone forward: what lies behind it carries nothing, what lies in front of it may
    ahead = view_of(s.prev(h, w, forward=True)[1])
    here = hits_array(s.cur_hits(h, w, "behind"), h, w)[:rows]
    zf = R.dot3(here["point"] - ahead.position, ahead.forward)
    behind = (here["hit"] != 0) & (zf <= 0.)
    assert behind.sum() > n_hit // 4 and not seen[("behind", 8)][3][behind].any()


# ---------------------------------------------------------------- 2. optional outputs; a stream of the caller's
def test_the_optional_outputs_may_be_left_out(pkg, scenes):
    import torch
    s = scenes("demo")
    p, cam, inputs, prev_hits = s.prev(32, 32)
    cur = s.cur_hits(32, 32, "sideways")
    full = Outputs(32, 32)
    s.c.reproject_device(p, *inputs, prev_hits, cur, cam, full.sum, full.stats, full.count, carried=full.carried, carried_total=full.total)
    want = full.results()
    bare = Outputs(32, 32)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        s.c.reproject_device(p, *inputs, prev_hits, cur, cam, bare.sum, bare.stats, bare.count)
    stream.synchronize()
    assert (bare.raw["carried"].cpu().numpy() == BYTE).all() and (bare.raw["total"].cpu().numpy() == WORD).all()
    for a, b in zip((bare.sum, bare.stats, bare.count), (full.sum, full.stats, full.count)):
        assert torch.equal(a, b)
    # the total is zeroed by the call: a second call into the same word does not add up
    s.c.reproject_device(p, *inputs, prev_hits, cur, cam, full.sum, full.stats, full.count, carried=full.carried, carried_total=full.total)
    assert full.results()[4] == want[4]
    # an rm_view is taken as well as what Context.camera() returned
    again = Outputs(32, 32)
    s.c.reproject_device(p, *inputs, prev_hits, cur, pkg._lib.rm_view(cam[0], cam[1]), again.sum, again.stats, again.count)
    assert torch.equal(again.sum, full.sum)


# ---------------------------------------------------------------- 3. garbage ends without a fault
def test_nan_points_and_garbage_counts_end_without_a_fault(pkg, scenes):
    """Unspecified pixels, which the yardstick need not match: the rule's range check is made in doubles before any address is
    formed, so no value of a hit or a count can leave the buffers.  What must hold: the call ends, the guards and the rows beyond
    stand, and pixels whose own hit and taps are clean are the yardstick's."""
    import torch
    s = scenes("demo")
    h, w = 72, 64
    p, cam, inputs, prev_hits = s.prev(h, w)
    cur = s.cur_hits(h, w, "sideways")
    r = np.random.default_rng(7)
    bad_cur, bad_prev = cur.clone(), prev_hits.clone()
    poison = torch.tensor([NAN, float("inf"), -float("inf"), 1e300, -1e300, 1e18], dtype=torch.float64, device="cuda:0")
    bad_cur[8:40, :, 1:4] = poison[torch.from_numpy(r.integers(0, 6, size=(32, w, 3))).to("cuda:0")]
    bad_prev[40:64, :, 1:7] = NAN
    bad_count = inputs[2].clone()
    bad_count[32:64] = torch.from_numpy(r.integers(-2 ** 31, 2 ** 31, size=(32, w)).astype(np.int32)).to("cuda:0")
    out = Outputs(h, w)
    s.c.reproject_device(p, inputs[0], inputs[1], bad_count, bad_prev, bad_cur, cam, out.sum, out.stats, out.count, carried=out.carried,
                         carried_total=out.total)
    got = out.results()
    assert got[4] == int(got[3].sum())
    assert not got[3][8:40].any() and (got[2][8:40] == 0).all()          # a hit that is NaN, infinite or far away carries nothing
    want = reference(("demo", h, w, "sideways"), inputs, prev_hits, cur, view_of(cam), frame_of(p), R.Control())
    assert got[0][:6].tobytes() == want[0][:6].tobytes() and got[2][:6].tobytes() == want[2][:6].tobytes()


# ---------------------------------------------------------------- 4. the refusals, each by name, nothing touched
def test_every_refusal_names_its_offender_and_touches_nothing(pkg, scenes):
    import torch
    L, B = pkg.lib(), pkg._lib
    s = scenes("demo")
    c = s.c
    p0, cam, inputs, prev_hits = s.prev(32, 32)
    cur = s.cur_hits(32, 32, "sideways")
    out = Outputs(32, 32)
    good = dict(sigma_z=.1, min_normal_dot=.9, max_history=32)
    good_view = B.rm_view(cam[0], cam[1])
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(p=p0, ctl=good, view=good_view, **ptrs):
        a = dict(prev_sum=inputs[0], prev_stats=inputs[1], prev_count=inputs[2], prev_hits=prev_hits, cur_hits=cur, out_sum=out.sum,
                 out_stats=out.stats, out_count=out.count, carried=out.carried, total=out.total)
        a.update(ptrs)
        d = B.rm_reproject(ctl["sigma_z"], ctl["min_normal_dot"], ctl["max_history"], 0) if ctl else None
        st = L.rm_reproject_device(c.ptr, C.byref(p) if p is not None else None, C.byref(d) if d is not None else None,
                                   C.byref(view) if view is not None else None, vp(a["prev_sum"]), vp(a["prev_stats"]), vp(a["prev_count"]),
                                   vp(a["prev_hits"]), vp(a["cur_hits"]), vp(a["out_sum"]), vp(a["out_stats"]), vp(a["out_count"]),
                                   vp(a["carried"]), vp(a["total"]), None)
        torch.cuda.synchronize()
        return st, L.rm_last_error(c.ptr).decode()

    def with_params(**kw):
        p = params(pkg, 32, 32)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def with_view(**kw):
        v = B.rm_view(B.rm_vec3(0., 0., 5.), B.rm_camera_basis(B.rm_vec3(1., 0., 0.), B.rm_vec3(0., 1., 0.), B.rm_vec3(0., 0., -1.)))
        for k, x in kw.items():
            setattr(getattr(v, k.split("_")[0]) if "_" in k else v, k.split("_")[-1], x)
        return v

    E, D = B.RM_ERR_INVALID_ARG, B.RM_ERR_DIMENSIONS
    cases = [
        (dict(p=None), E, "rm_reproject_device: NULL params"),
        (dict(p=with_params(flags=4)), E, "params.flags may carry RM_FLAG_FAST_FP only"),
        (dict(p=with_params(patch_row_begin=1)), E, "default patch-row band only"),
        (dict(p=with_params(patch_size=16)), E, "patch_size must be 32"),
        (dict(p=with_params(frame_height=0)), E, "empty frame"),
        (dict(p=with_params(frame_width=48)), D, "frame width is not a multiple of 32"),
        (dict(p=with_params(frame_width=65536, frame_height=65536)), D, "more than 2^31 - 1 pixels"),
        (dict(ctl=None), E, "rm_reproject_device: NULL reproject"),
        (dict(ctl=dict(good, sigma_z=0.)), E, "reproject.sigma_z = 0 is not a finite number > 0"),
        (dict(ctl=dict(good, sigma_z=NAN)), E, "reproject.sigma_z = nan is not a finite number > 0"),
        (dict(ctl=dict(good, sigma_z=float("inf"))), E, "reproject.sigma_z = inf is not a finite number > 0"),
        (dict(ctl=dict(good, min_normal_dot=1.)), E, "reproject.min_normal_dot = 1 is outside [-1, 1)"),
        (dict(ctl=dict(good, min_normal_dot=-1.25)), E, "reproject.min_normal_dot = -1.25 is outside [-1, 1)"),
        (dict(ctl=dict(good, min_normal_dot=NAN)), E, "reproject.min_normal_dot = nan is outside [-1, 1)"),
        (dict(ctl=dict(good, max_history=0)), E, "reproject.max_history = 0 is outside 1..65536"),
        (dict(ctl=dict(good, max_history=65537)), E, "reproject.max_history = 65537 is outside 1..65536"),
        (dict(view=None), E, "rm_reproject_device: NULL previous_view"),
        (dict(view=with_view(position_x=NAN)), E, "previous_view.position (nan, 0, 5) is not finite"),
        (dict(view=with_view(basis_right=B.rm_vec3(2., 0., 0.))), E, "previous_view.basis: "),
        (dict(view=with_view(basis_up=B.rm_vec3(0., NAN, 0.))), E, "previous_view.basis: "),
        (dict(view=with_view(basis_forward=B.rm_vec3(0., 1., 0.))), E, "previous_view.basis: "),
        (dict(prev_sum=None), E, "rm_reproject_device: NULL prev_sum"),
        (dict(prev_stats=None), E, "rm_reproject_device: NULL prev_stats"),
        (dict(prev_count=None), E, "rm_reproject_device: NULL prev_count"),
        (dict(prev_hits=None), E, "rm_reproject_device: NULL prev_hits"),
        (dict(cur_hits=None), E, "rm_reproject_device: NULL cur_hits"),
        (dict(out_sum=None), E, "rm_reproject_device: NULL out_sum"),
        (dict(out_stats=None), E, "rm_reproject_device: NULL out_stats"),
        (dict(out_count=None), E, "rm_reproject_device: NULL out_count"),
        (dict(out_sum=inputs[0]), E, "out_sum == prev_sum"),
        (dict(out_stats=inputs[1]), E, "out_stats == prev_stats"),
        (dict(out_count=inputs[2]), E, "out_count == prev_count"),
        (dict(out_sum=prev_hits), E, "out_sum == prev_hits"),
        (dict(out_stats=cur), E, "out_stats == cur_hits"),
        (dict(carried=inputs[2]), E, "out_carried == prev_count"),
        (dict(total=cur), E, "out_carried_total == cur_hits"),
    ]
    before = [t.clone() for t in inputs + (prev_hits, cur)]
    for kw, status, text in cases:
        st, msg = call(**kw)
        assert st == status and text in msg and msg.startswith("rm_reproject_device: "), (kw, st, msg)
        assert out.untouched(), text
    for a, b in zip(before, inputs + (prev_hits, cur)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # a frame without a whole patch row: RM_OK, nothing done; then everything in order does run
    assert call(p=with_params(frame_height=31))[0] == B.RM_OK and out.untouched()
    assert call()[0] == B.RM_OK and not out.untouched()
    # ... and the Python wrapper refuses an output that is an input before the library
    with pytest.raises(ValueError, match="out_total must not be prev_total's own tensor"):
        c.reproject_device(p0, *inputs, prev_hits, cur, cam, inputs[0], out.stats, out.count)
    # rm_converge_history's own: the settings' ranges, by name, and the state stays what it was
    hist = lambda d: L.rm_converge_history(c.ptr, C.byref(B.rm_reproject(d["sigma_z"], d["min_normal_dot"], d["max_history"], 0)))
    for bad, text in ((dict(good, sigma_z=-1.), "rm_converge_history: reproject.sigma_z = -1 is not a finite number > 0"),
                      (dict(good, min_normal_dot=NAN), "rm_converge_history: reproject.min_normal_dot = nan is outside [-1, 1)"),
                      (dict(good, max_history=0), "rm_converge_history: reproject.max_history = 0 is outside 1..65536")):
        assert hist(bad) == E and text in L.rm_last_error(c.ptr).decode()
    assert L.rm_converge_history_info(c.ptr, None) == E and b"rm_converge_history_info: NULL report" in L.rm_last_error(c.ptr)
    assert c.history_info() == {"reprojections": 0, "last_reprojected": 0, "carried": 0, "without": 0}
