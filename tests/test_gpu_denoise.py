"""The variance-guided filter on the GPU (-m gpu): rm_denoise_device through the Python binding and the C ABI against
tests/denoise_reference.py, the rule in numpy (pinned on the CPU by tests/test_denoise_reference.py).

The rule is + - * / and comparisons of doubles, each rounded once, so everything here is demanded BYTE FOR BYTE: the mean, the
variance and the display bytes, for both paths an iteration can take (RM_DENOISE_TILED=0: every tap gathered from global memory;
=3: steps 1 and 2 from a tile staged in LDS) and for the choice the library makes when the knob is unset.  Every output and the
workspace stand between guards, the rows from `rows` on hold sentinels in every buffer -- poison in the inputs, so that a tap
that read one would show -- and neither may change."""
import ctypes as C

import numpy as np
import pytest

import denoise_reference as DR
import workloads

pytestmark = pytest.mark.gpu

NAN, BYTE, WORD = float("nan"), 0xA5, 0x5a5a5a5a
GUARD = 256                                                            # elements in front of and behind every output
SIZES = [(96, 96), (32, 32), (40, 64)]                                 # (h, w): the smallest frame with a pixel whose 25 taps at step 16
#                                                                        are all inside; one whose outer taps all leave from step 16 on;
#                                                                        one with rows beyond `rows` (40 % 32 = 8 of them)
PATHS = {"gather": "0", "tiled": "3", "chosen": None}                  # (RM_DENOISE_TILED: the sum of the steps that take the LDS path)


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def synthetic():
    """(h, w) -> the seeded inputs, made once and shared (never written to)"""
    out = {}
    for seed, (h, w) in enumerate(SIZES):
        out[(h, w)] = DR.synthetic(100 + seed, h, w)
        for a in out[(h, w)]:
            a.setflags(write=False)
    return out


_REFERENCE = {}


def reference(key, S, stats, n, hits, ctl):
    """The yardstick's answer, computed once a case (`key` names the inputs) and shared among the paths."""
    k = (key, hits is not None, ctl.sigma_l, ctl.sigma_z, ctl.epsilon, ctl.fallback_variance, ctl.iterations, ctl.normal_squarings)
    if k not in _REFERENCE:
        _REFERENCE[k] = DR.denoise(S, stats, n, hits, ctl)
        for a in _REFERENCE[k]:
            a.setflags(write=False)
    return _REFERENCE[k]


def set_path(monkeypatch, path):
    if PATHS[path] is None:
        monkeypatch.delenv("RM_DENOISE_TILED", raising=False)
    else:
        monkeypatch.setenv("RM_DENOISE_TILED", PATHS[path])


class Buffers:
    """Device buffers of a call: the inputs with poison in the rows from `rows` on, every output and the workspace between
    guards and filled with sentinels."""

    def __init__(self, pkg, c, S, stats, n, hits):
        import torch
        h, w = n.shape
        self.h, self.w, self.rows = h, w, DR.rows_of(h)
        self.p = pkg.backend.make_params(workloads.FOV, float(h), float(w), 3)
        dev = "cuda:0"
        S, stats, n = np.array(S), np.array(stats), np.array(n)
        S[self.rows:], stats[self.rows:], n[self.rows:] = NAN, NAN, 7
        self.sum, self.stats = torch.from_numpy(S).to(dev), torch.from_numpy(stats).to(dev)
        self.count = torch.from_numpy(n.view(np.int32)).to(dev)
        self.hits = None
        if hits is not None:
            raw = np.array(hits).view(np.float64).reshape(h, w, 9)
            raw[self.rows:] = NAN
            self.hits = torch.from_numpy(raw).to(dev)
        self.ws_bytes = c.denoise_workspace(self.p)

        def guarded(count, dtype, fill):
            raw = torch.full((GUARD + count + GUARD,), fill, dtype=dtype, device=dev)
            return raw, raw[GUARD:GUARD + count]

        self.raw, self.fill = {}, {"out": NAN, "variance": NAN, "rgb8": BYTE, "ws": BYTE}
        self.raw["out"], out = guarded(h * w * 3, torch.float64, NAN)
        self.raw["variance"], var = guarded(h * w, torch.float64, NAN)
        self.raw["rgb8"], rgb8 = guarded(h * w * 3, torch.uint8, BYTE)
        self.raw["ws"], self.ws = guarded(self.ws_bytes, torch.uint8, BYTE)
        self.out, self.variance, self.rgb8 = out.view(h, w, 3), var.view(h, w), rgb8.view(h, w, 3)
        self.inputs_before = [t.clone() for t in (self.sum, self.stats, self.count) + ((self.hits,) if hits is not None else ())]

    def untouched(self, names=("out", "variance", "rgb8", "ws")):
        """Nothing was written: every named buffer holds its sentinel from end to end."""
        import torch
        torch.cuda.synchronize()
        for name in names:
            a = self.raw[name].cpu().numpy()
            if not (np.isnan(a).all() if a.dtype == np.float64 else (a == self.fill[name]).all()):
                return False
        return True

    def results(self):
        """-> (C, V, bytes) of the rows the filter writes, after the guards, the rows beyond and the inputs were found intact."""
        import torch
        torch.cuda.synchronize()
        for name, raw in self.raw.items():
            a = raw.cpu().numpy()
            for edge in (a[:GUARD], a[-GUARD:]):
                assert np.isnan(edge).all() if a.dtype == np.float64 else (edge == self.fill[name]).all(), "the guard of %s was written" % name
        out, var, rgb8 = self.out.cpu().numpy(), self.variance.cpu().numpy(), self.rgb8.cpu().numpy()
        assert np.isnan(out[self.rows:]).all() and np.isnan(var[self.rows:]).all() and (rgb8[self.rows:] == BYTE).all(), "rows beyond `rows` were written"
        now = (self.sum, self.stats, self.count) + ((self.hits,) if self.hits is not None else ())
        for a, b in zip(now, self.inputs_before):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), "an input was written"
        return out[:self.rows], var[:self.rows], rgb8[:self.rows]

    def run(self, c, ctl, outputs=True):
        c.denoise_device(self.p, self.sum, self.stats, self.count, self.out, ctl.sigma_l, ctl.sigma_z, ctl.epsilon, ctl.fallback_variance,
                         ctl.iterations, ctl.normal_squarings, hits=self.hits, variance=self.variance if outputs else None,
                         rgb8=self.rgb8 if outputs else None, workspace=self.ws)
        return self.results()


def same_bytes(got, want, what):
    C_, V_, B_ = got
    rC, rV, rB = want
    for name, a, b in (("mean", C_, rC), ("variance", V_, rV), ("bytes", B_, rB)):
        if a.tobytes() != b.tobytes():
            differ = np.argwhere(a.view(np.uint64 if a.dtype == np.float64 else a.dtype) != b.view(np.uint64 if b.dtype == np.float64 else b.dtype))
            worst = float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64))))
            raise AssertionError("%s: %s differs from the yardstick in %d places, first at %s, by at most %.3g" % (what, name, len(differ), differ[0], worst))


# ---------------------------------------------------------------- 1. seeded inputs, every size, iteration count, guide and path
def test_the_seeded_inputs_hold_every_branch(synthetic):
    for (h, w), (S, stats, n, hits) in synthetic.items():
        rows = DR.rows_of(h)
        n, hits = n[:rows], hits[:rows]
        assert (n == 0).any() and (n == 1).any() and (n >= 2).any(), (h, w)
        assert (hits["hit"] == 1).any() and (hits["hit"] == 0).any(), (h, w)
        assert len(np.unique(hits["shape"][hits["hit"] == 1])) >= 3, (h, w)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "guided"])
@pytest.mark.parametrize("iterations", [0, 1, 3, 5])
@pytest.mark.parametrize("h,w", SIZES)
def test_the_filter_is_the_yardstick_byte_for_byte(pkg, ctx, synthetic, monkeypatch, h, w, iterations, guided, path):
    S, stats, n, hits = synthetic[(h, w)]
    ctl = DR.Control(sigma_l=4., sigma_z=.1, epsilon=1e-10, fallback_variance=.75, iterations=iterations, normal_squarings=5)
    want = reference(("synthetic", h, w), S, stats, n, hits if guided else None, ctl)
    set_path(monkeypatch, path)
    b = Buffers(pkg, ctx, S, stats, n, hits if guided else None)
    same_bytes(b.run(ctx, ctl), want, "%dx%d, %d iterations, %s, %s" % (h, w, iterations, "guided" if guided else "unguided", path))
    if iterations == 0:
        some = n[:b.rows] > 0
        assert np.array_equal(want[0][some], S[:b.rows][some] / n[:b.rows][some].astype(np.float64)[:, None])   # (the converging frames' mean)


@pytest.mark.parametrize("squarings,sigma_z", [(0, 10.), (8, .01), (1, 1.)])
def test_other_controls_and_absent_optional_outputs(pkg, ctx, synthetic, monkeypatch, squarings, sigma_z):
    S, stats, n, hits = synthetic[(96, 96)]
    ctl = DR.Control(sigma_l=.5, sigma_z=sigma_z, epsilon=1e-4, fallback_variance=0., iterations=4, normal_squarings=squarings)
    want = reference(("synthetic", 96, 96), S, stats, n, hits, ctl)
    for path in ("gather", "tiled"):
        set_path(monkeypatch, path)
        b = Buffers(pkg, ctx, S, stats, n, hits)
        same_bytes(b.run(ctx, ctl), want, "squarings %d, sigma_z %g, %s" % (squarings, sigma_z, path))
        # without variance and rgb8 the mean is the same and the two are left alone
        b = Buffers(pkg, ctx, S, stats, n, hits)
        got = b.run(ctx, ctl, outputs=False)
        assert got[0].tobytes() == want[0].tobytes() and b.untouched(("variance", "rgb8"))


# ---------------------------------------------------------------- 2. real inputs: converging passes and the hits under the pixels
@pytest.mark.parametrize("name", ["demo", "cornell"])
def test_real_converging_frames_with_primary_hits(pkg, ctx, monkeypatch, name):
    import torch
    h = w = 96
    ctx.orient(None)
    ctx.upload(workloads.product_scene(pkg, name).flatten())
    p = pkg.backend.make_params(workloads.FOV, float(h), float(w), 3)
    total, stats = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0"), torch.zeros((h, w, 2), dtype=torch.float64, device="cuda:0")
    count = torch.zeros((h, w), dtype=torch.int32, device="cuda:0")
    table = torch.from_numpy(ctx.lens_sequence(0, 64)).to("cuda:0")
    for k in range(3):
        ctx.accumulate_converging_device(p, total, stats, count, 0., 5., 8, table, 0.02, 8, 64, k == 0)
    hits = ctx.primary_hits_device(p)
    torch.cuda.synchronize()
    S, Q, n = total.cpu().numpy(), stats.cpu().numpy(), count.cpu().numpy().view(np.uint32)
    H = np.ascontiguousarray(hits.raw.cpu().numpy()).view(DR.HIT_DTYPE).reshape(h, w)
    assert n.min() >= 8 and len(np.unique(n)) >= 2                       # some pixels settled after the first passes, some went on
    hit = H["hit"] == 1
    assert hit.any() and (~hit).any()
    if name == "demo":
        assert len(np.unique(H["shape"][hit])) >= 2                      # several shapes: silhouettes between them
    else:
        assert len(np.unique(H["shape"][hit])) == 1 and len(np.unique(H["element"][hit])) >= 2   # one mesh, many triangles: one surface to the guide
    for guided in (True, False):
        ctl = DR.Control(iterations=5)
        want = reference(("real", name), S, Q, n, H if guided else None, ctl)
        for path in ("gather", "tiled"):
            set_path(monkeypatch, path)
            b = Buffers(pkg, ctx, S, Q, n, H if guided else None)
            same_bytes(b.run(ctx, ctl), want, "%s, %s, %s" % (name, "guided" if guided else "unguided", path))
    # the filter does something here: it moves noisy pixels, and with the guide it moves fewer of them across the shapes' edges
    guided_C, unguided_C = reference(("real", name), S, Q, n, H, ctl)[0], reference(("real", name), S, Q, n, None, ctl)[0]
    mean = S / n.astype(np.float64)[..., None]
    assert not np.array_equal(guided_C, mean) and not np.array_equal(guided_C, unguided_C)


# ---------------------------------------------------------------- 3. two shapes never mix; sigma_l = 0
@pytest.mark.parametrize("path", ["gather", "tiled"])
def test_two_shapes_come_back_exactly(pkg, ctx, monkeypatch, path):
    h = w = 64
    yy, xx = np.mgrid[0:h, 0:w]
    left = xx + yy // 3 < 40
    n = np.full((h, w), 8, np.uint32)
    S = np.where(left[..., None], 8., 0.) * np.ones(3)
    stats = np.zeros((h, w, 2))
    stats[..., 0] = np.where(left, 24., 0.)
    stats[..., 1] = stats[..., 0] * stats[..., 0] / 8. + 7. * .09        # a large variance: the luminance stop is wide open
    hits = np.zeros((h, w), DR.HIT_DTYPE)
    hits["hit"], hits["shape"], hits["t"], hits["normal"] = 1, np.where(left, 2, 5), 3., (0., 0., 1.)
    hits["point"] = np.stack([xx * .01, yy * .01, np.full((h, w), -3.)], axis=-1)
    hits["element"] = xx % 7
    set_path(monkeypatch, path)
    ctl = DR.Control()
    got = Buffers(pkg, ctx, S, stats, n, hits).run(ctx, ctl)
    assert np.all(got[0][left] == 1.) and np.all(got[0][~left] == 0.)
    assert np.all(got[2][left] == 255) and np.all(got[2][~left] == 0)
    same_bytes(got, reference(("two shapes",), S, stats, n, hits, ctl), "two shapes, %s" % path)
    unguided = Buffers(pkg, ctx, S, stats, n, None).run(ctx, ctl)
    assert ((unguided[0] > 0.) & (unguided[0] < 1.)).any()               # without the guide the edge does blur


@pytest.mark.parametrize("path", ["gather", "tiled"])
def test_no_luminance_stop_and_a_tiny_epsilon(pkg, ctx, synthetic, monkeypatch, path):
    """sigma_l = 0 leaves den = epsilon: a tap whose y differs at all weighs about epsilon / a^2, a subnormal or zero for a tiny
    epsilon, so the filter is nearly the identity -- and the quotients, products and sums of such numbers are still the yardstick's."""
    S, stats, n, hits = synthetic[(96, 96)]
    set_path(monkeypatch, path)
    for eps in (1e-300, 1e-30):
        ctl = DR.Control(sigma_l=0., epsilon=eps, iterations=5)
        for guide in (None, hits):
            want = reference(("synthetic", 96, 96), S, stats, n, guide, ctl)
            same_bytes(Buffers(pkg, ctx, S, stats, n, guide).run(ctx, ctl), want, "sigma_l = 0, epsilon %g, %s" % (eps, path))
        C0 = DR.denoise(S, stats, n, None, DR.Control(iterations=0))[0]
        kept = n > 0
        assert np.abs(want[0][kept] - C0[kept]).max() < 1e-6             # (nearly the identity where there is a sample)


# ---------------------------------------------------------------- 4. the refusals, each by name, nothing touched
def test_every_refusal_names_its_offender_and_touches_nothing(pkg, ctx, synthetic):
    import torch
    L, B = pkg.lib(), pkg._lib
    S, stats, n, hits = synthetic[(32, 32)]
    b = Buffers(pkg, ctx, S, stats, n, hits)
    good = dict(sigma_l=4., sigma_z=.1, epsilon=1e-10, fallback_variance=1., iterations=5, normal_squarings=5)
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(p=b.p, ctl=good, **ptrs):
        a = dict(sum=b.sum, stats=b.stats, count=b.count, hits=b.hits, ws=b.ws, out=b.out, variance=b.variance, rgb8=b.rgb8)
        a.update(ptrs)
        d = B.rm_denoise(*[ctl[k] for k in ("sigma_l", "sigma_z", "epsilon", "fallback_variance", "iterations", "normal_squarings")]) if ctl else None
        st = L.rm_denoise_device(ctx.ptr, C.byref(p) if p is not None else None, C.byref(d) if d is not None else None, vp(a["sum"]),
                                 vp(a["stats"]), vp(a["count"]), vp(a["hits"]), vp(a["ws"]), vp(a["out"]), vp(a["variance"]), vp(a["rgb8"]), None)
        torch.cuda.synchronize()
        return st, L.rm_last_error(ctx.ptr).decode()

    def params(**kw):
        p = pkg.backend.make_params(workloads.FOV, 32., 32., 3)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    E, D = B.RM_ERR_INVALID_ARG, B.RM_ERR_DIMENSIONS
    cases = [
        (dict(p=None), E, "rm_denoise_device: NULL params"),
        (dict(p=params(flags=4)), E, "params.flags may carry RM_FLAG_FAST_FP only"),
        (dict(p=params(patch_row_begin=1)), E, "default patch-row band only"),
        (dict(p=params(patch_size=16)), E, "patch_size must be 32"),
        (dict(p=params(frame_height=0)), E, "empty frame"),
        (dict(p=params(frame_width=48)), D, "frame width is not a multiple of 32"),
        (dict(p=params(frame_width=65536, frame_height=65536)), D, "more than 2^31 - 1 pixels"),
        (dict(ctl=None), E, "rm_denoise_device: NULL denoise"),
        (dict(ctl=dict(good, sigma_l=-1.)), E, "denoise.sigma_l = -1 is not a finite number >= 0"),
        (dict(ctl=dict(good, sigma_l=NAN)), E, "denoise.sigma_l = nan is not a finite number >= 0"),
        (dict(ctl=dict(good, sigma_z=0.)), E, "denoise.sigma_z = 0 is not a finite number > 0"),
        (dict(ctl=dict(good, sigma_z=NAN)), E, "denoise.sigma_z = nan is not a finite number > 0"),
        (dict(ctl=dict(good, epsilon=0.)), E, "denoise.epsilon = 0 is not a finite number > 0"),
        (dict(ctl=dict(good, epsilon=float("inf"))), E, "denoise.epsilon = inf is not a finite number > 0"),
        (dict(ctl=dict(good, epsilon=NAN)), E, "denoise.epsilon = nan"),
        (dict(ctl=dict(good, fallback_variance=-.5)), E, "denoise.fallback_variance = -0.5 is not a finite number >= 0"),
        (dict(ctl=dict(good, fallback_variance=NAN)), E, "denoise.fallback_variance = nan"),
        (dict(ctl=dict(good, iterations=6)), E, "denoise.iterations = 6 is outside 0..5"),
        (dict(ctl=dict(good, normal_squarings=9)), E, "denoise.normal_squarings = 9 is outside 0..8"),
        (dict(sum=None), E, "rm_denoise_device: NULL sum"),
        (dict(stats=None), E, "rm_denoise_device: NULL stats"),
        (dict(count=None), E, "rm_denoise_device: NULL count"),
        (dict(ws=None), E, "rm_denoise_device: NULL workspace"),
        (dict(out=None), E, "rm_denoise_device: NULL out"),
        (dict(out=b.sum), E, "device_out == device_sum"),
        (dict(out=b.stats), E, "device_out == device_stats"),
        (dict(out=b.count), E, "device_out == device_count"),
        (dict(out=b.hits), E, "device_out == device_hits"),
    ]
    for kw, status, text in cases:
        st, msg = call(**kw)
        assert st == status and text in msg and msg.startswith("rm_denoise_device: "), (kw, st, msg)
        assert b.untouched(), text
    # a frame without a whole patch row: RM_OK, nothing done; then everything in order does run
    assert call(p=params(frame_height=31))[0] == B.RM_OK and b.untouched()
    assert call()[0] == B.RM_OK and not b.untouched(("out",))
    # ... and the Python wrapper refuses an output that is an input, and a workspace that is too small, before the library
    with pytest.raises(ValueError, match="out must not be sum's own tensor"):
        ctx.denoise_device(b.p, b.sum, b.stats, b.count, b.sum)
    with pytest.raises(ValueError, match="workspace must be"):
        ctx.denoise_device(b.p, b.sum, b.stats, b.count, b.out, workspace=b.ws[:b.ws_bytes - 256])
