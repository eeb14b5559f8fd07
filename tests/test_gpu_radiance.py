"""Radiance queries on the GPU (-m gpu): rm_radiance_rays / rm_radiance_samples and their device variants through the C ABI,
and Renderer.render_supersampled over them, against the CPU oracle's own orc_cast_ray(o, d, scene, bg, 1, max_depth)
(tests/radiance_reference.py, pinned on the CPU by tests/test_radiance_abi.py).

Every channel of every answer within TIGHT = 1e-9 of the oracle, no ray left out: the kernels are the strict flavour and
take the reference's decisions bit for bit.  Largest deviations observed on an MI355X are recorded in DESIGN.md section 6e."""
import ctypes as C

import numpy as np
import pytest

import radiance_reference as RR
import test_gpu_query as GQ
import workloads

pytestmark = pytest.mark.gpu

TIGHT = RR.TIGHT
W, H = 96, 64


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_radiance"))


class Sets:
    """Scenes, ray sets and the oracle's answers, each made once and shared (never written to)."""

    def __init__(self, pkg, O, orc):
        self.pkg, self.O, self.orc = pkg, O, orc
        self._scene, self._rays, self._ref = {}, {}, {}

    def scene(self, name):
        if name not in self._scene:
            if name == "panes":
                self._scene[name] = RR.pane_stack(self.pkg, self.O)
            else:
                self._scene[name] = (workloads.product_scene(self.pkg, name), workloads.oracle_scene(self.O, name))
        return self._scene[name]

    def rays(self, name):
        if name not in self._rays:
            rng = np.random.default_rng(RR.SEEDS[name])
            if name == "panes":
                self._rays[name] = RR.pane_rays(rng)
            else:
                self._rays[name] = RR.rays_for(name, self.scene(name)[0].flatten().desc(), rng)
            for a in self._rays[name]:
                a.setflags(write=False)
        return self._rays[name]

    def ref(self, name, depth, bg=RR.BACKGROUND, scale=1.):
        key = (name, depth, tuple(bg), scale)
        if key not in self._ref:
            o, d = self.rays(name)
            self._ref[key] = self.orc.cast(self.scene(name)[1], o, d * scale, depth, bg)
            self._ref[key].setflags(write=False)
        return self._ref[key]


@pytest.fixture(scope="module")
def sets(pkg, O, orc):
    return Sets(pkg, O, orc)


def upload(ctx, scene):
    ctx.orient(None)
    ctx.upload(scene.flatten())


def worst(got, ref):
    return float(np.abs(got - ref).max(initial=0.))


# ---------------------------------------------------------------- 1. ray lists against the oracle
@pytest.mark.parametrize("name", ["demo", "cornell", "synthetic256"])
def test_ray_lists_match_the_oracle(ctx, sets, name):
    upload(ctx, sets.scene(name)[0])
    o, d = sets.rays(name)
    for depth, bg in ((3, RR.BACKGROUND), (6, RR.BACKGROUND), (3, (0.3, 0.0, 0.7))):
        got = ctx.radiance(o, d, max_depth=depth, background=bg)
        ref = sets.ref(name, depth, bg)
        delta = worst(got, ref)
        print("%s depth %d background %s: max |delta| %.3e over %d rays, %d lit" % (name, depth, bg, delta, len(o), int((ref != 0.).any(axis=1).sum())))
        assert got.shape == ref.shape and delta < TIGHT
        # a ray that leaves the scene returns exactly +0 in every channel
        gone = ~(ref != 0.).any(axis=1)
        assert gone.any() and not got[gone].view(np.uint64).any()


def test_generic_pow_in_a_context_of_its_own(pkg, sets, monkeypatch):
    """RM_FORCE_GENERIC_POW=1 is read when a context is made (rm_init): a context of its own runs the POW_GENERIC kernels."""
    monkeypatch.setenv("RM_FORCE_GENERIC_POW", "1")
    c = pkg.backend.Context(0)
    try:
        c.upload(sets.scene("demo")[0].flatten())
        o, d = sets.rays("demo")
        got = c.radiance(o, d, max_depth=6)
    finally:
        c.close()
    delta = worst(got, sets.ref("demo", 6))
    print("generic pow, demo depth 6: max |delta| %.3e" % delta)
    assert delta < TIGHT


# ---------------------------------------------------------------- 2. sizes
def test_sizes_agree_with_the_long_call(ctx, sets):
    upload(ctx, sets.scene("synthetic256")[0])
    o, d = sets.rays("synthetic256")
    full = ctx.radiance(o, d, max_depth=6)
    for n in (1, 63, 64, 65):
        part = ctx.radiance(o[:n], d[:n], max_depth=6)
        assert part.tobytes() == full[:n].tobytes(), "n = %d" % n
    assert ctx.radiance(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0, 3)


# ---------------------------------------------------------------- 3. depth caps
def test_depth_caps_through_the_pane_stack(ctx, sets):
    upload(ctx, sets.scene("panes")[0])
    o, d = sets.rays("panes")
    for depth in (0, 1, 2, 6, 17, 32):
        got = ctx.radiance(o, d, max_depth=depth)
        delta = worst(got, sets.ref("panes", depth))
        print("panes depth %d: max |delta| %.3e" % (depth, delta))
        assert delta < TIGHT
        if depth == 0:
            assert np.all(got == 0.1)                                # the background, exactly
    assert np.all(ctx.radiance(o[:70], d[:70], max_depth=0, background=(0.25, 0.5, 0.75)) == np.array([0.25, 0.5, 0.75]))


# ---------------------------------------------------------------- 4. the sky
def test_a_ray_into_the_sky_returns_exact_zero(ctx, sets):
    scene = sets.scene("demo")[0]
    upload(ctx, scene)
    pos, _, _ = ctx.camera()
    o = np.array([[pos.x, pos.y, pos.z]] * 3)
    d = GQ.unit(np.array([[0., 1., 0.], [0., 1., 0.2], [0.1, 1., 0.]]))
    for bg in (RR.BACKGROUND, (-0.5, 2., 0.)):
        got = ctx.radiance(o, d, max_depth=5, background=bg)
        assert not got.view(np.uint64).any(), got                    # +0.0 in every channel, whatever the background


# ---------------------------------------------------------------- 5. directions within the assert, not of unit length
@pytest.mark.parametrize("scale", [1. + 4e-5, 1. - 4e-5])
def test_non_unit_directions(ctx, sets, scale):
    upload(ctx, sets.scene("demo")[0])
    o, d = sets.rays("demo")
    assert np.abs(((d * scale) ** 2).sum(axis=1) - 1.).max() < 1e-4
    got = ctx.radiance(o, d * scale, max_depth=6)
    ref = sets.ref("demo", 6, scale=scale)
    delta = worst(got, ref)
    print("directions x %.6f: max |delta| %.3e (against the unit set's answers: %.3e)" % (scale, delta, worst(got, sets.ref("demo", 6))))
    assert delta < TIGHT


# ---------------------------------------------------------------- 6. samples
def side_view(ctx, desc):
    """One look_at from the side: the eye off to the right of and above the fixed camera, looking at the scene's middle."""
    lo, hi = GQ.bounds_of(desc)
    pos, _, _ = ctx.camera()
    eye = np.array([pos.x, pos.y, pos.z]) + np.array([0.12, 0.06, 0.]) * np.linalg.norm(hi - lo)
    ctx.look_at(tuple(eye), tuple((lo + hi) / 2.))
    pos, basis, on = ctx.camera()
    assert on
    return (pos.x, pos.y, pos.z), RR.basis_tuple(basis)


@pytest.mark.parametrize("name", ["demo", "cornell"])
@pytest.mark.parametrize("view", ["fixed", "side"])
def test_samples_match_the_oracle_and_the_render(pkg, ctx, sets, orc, name, view):
    scene, oscene = sets.scene(name)
    handle = scene.flatten()
    upload(ctx, scene)
    try:
        pos, _, _ = ctx.camera()
        eye, basis = (pos.x, pos.y, pos.z), None
        if view == "side":
            eye, basis = side_view(ctx, handle.desc())
        p = pkg.backend.make_params(workloads.FOV, float(H), float(W), 5)
        rng = np.random.default_rng(RR.SEEDS["samples"])
        xy = np.concatenate([RR.pixel_positions(W, H), rng.uniform((0., 0.), (W, H), size=(RR.N_RAYS, 2))])
        assert xy[:, 0].max() < W and xy[:, 1].max() < H
        got = ctx.radiance_samples(p, xy)
        ref = orc.cast(oscene, eye, RR.sample_directions(xy, orc.renderer(W, H), basis), 5, normalize=True)
        delta = worst(got, ref)
        lit = (ref != 0.).any(axis=1).mean()
        print("%s %s view: samples max |delta| %.3e, %.0f %% lit" % (name, view, delta, 100. * lit))
        assert delta < TIGHT and lit > 0.05
        assert len(np.unique(ref.round(6), axis=0)) > 500            # a picture, not a flat shade
        frame = np.zeros((H, W, 3))
        ctx.render(p, frame)
        d_render = worst(got[:W * H].reshape(H, W, 3), frame)
        print("%s %s view: integer positions against rm_render: %.3e" % (name, view, d_render))
        assert d_render < TIGHT
    finally:
        ctx.orient(None)


def test_samples_answer_the_rows_the_render_leaves_alone(pkg, ctx, sets, orc):
    scene, oscene = sets.scene("demo")
    upload(ctx, scene)
    p = pkg.backend.make_params(workloads.FOV, 70., float(W), 3)
    xy = RR.pixel_positions(W, 70)
    got = ctx.radiance_samples(p, xy)
    pos, _, _ = ctx.camera()
    ref = orc.cast(oscene, (pos.x, pos.y, pos.z), RR.sample_directions(xy, orc.renderer(W, 70)), 3, normalize=True)
    assert worst(got, ref) < TIGHT
    assert (ref[64 * W:] != 0.).any()                                # the six last rows show the floor
    # ... and a frame width that is no multiple of 32
    odd = pkg.backend.make_params(workloads.FOV, 70., 50., 3)
    xy = RR.pixel_positions(50, 70)
    ref = orc.cast(oscene, (pos.x, pos.y, pos.z), RR.sample_directions(xy, orc.renderer(50, 70)), 3, normalize=True)
    assert worst(ctx.radiance_samples(odd, xy), ref) < TIGHT


# ---------------------------------------------------------------- 7. device variants
def test_device_variants_equal_the_host_variants(pkg, ctx, sets):
    import torch
    upload(ctx, sets.scene("cornell")[0])
    o, d = sets.rays("cornell")
    p = pkg.backend.make_params(workloads.FOV, float(H), float(W), 4)
    xy = np.random.default_rng(7).uniform((0., 0.), (W, H), size=(1000, 2))
    host = ctx.radiance(o, d, max_depth=4, background=(0.2, 0.1, 0.))
    host_s = ctx.radiance_samples(p, xy)
    to, td, txy = (torch.from_numpy(np.array(a)).to("cuda:0") for a in (o, d, xy))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev = ctx.radiance_device(to, td, max_depth=4, background=(0.2, 0.1, 0.))
        dev_s = ctx.radiance_samples_device(p, txy)
    s.synchronize()
    assert dev.shape == (len(o), 3) and dev.dtype == torch.float64
    assert dev.cpu().numpy().tobytes() == host.tobytes()
    assert dev_s.cpu().numpy().tobytes() == host_s.tobytes()
    # torch's current stream by default
    assert ctx.radiance_device(to, td, max_depth=4, background=(0.2, 0.1, 0.)).cpu().numpy().tobytes() == host.tobytes()


# ---------------------------------------------------------------- 8. refusals
def test_refusals_leave_the_output_alone(pkg, ctx, sets):
    L, B = pkg.lib(), pkg._lib
    V = C.POINTER(B.rm_vec3)
    upload(ctx, sets.scene("demo")[0])
    SENTINEL = 7.25
    o = np.zeros((4, 3))
    d = np.tile([0., 0., -1.], (4, 1))
    sh = B.rm_shading(B.rm_vec3(.1, .1, .1), 3, 0)

    def rays(c, oo, dd, shading, n=4):
        out = np.full((4, 3), SENTINEL)
        st = L.rm_radiance_rays(c.ptr, oo.ctypes.data_as(V), dd.ctypes.data_as(V), n, C.byref(shading) if shading is not None else None,
                                out.ctypes.data_as(V))
        assert np.all(out == SENTINEL) or st == 0
        return st, L.rm_last_error(c.ptr).decode()

    def samples(c, p, xy):
        xy = np.ascontiguousarray(xy, dtype=np.float64)
        out = np.full((len(xy), 3), SENTINEL)
        st = L.rm_radiance_samples(c.ptr, C.byref(p), xy.ctypes.data_as(C.POINTER(C.c_double)), len(xy), out.ctypes.data_as(V))
        assert np.all(out == SENTINEL) or st == 0
        return st, L.rm_last_error(c.ptr).decode()

    assert rays(ctx, o, d, sh)[0] == 0
    bad = o.copy(); bad[2, 1] = np.nan
    st, msg = rays(ctx, bad, d, sh)
    assert st == B.RM_ERR_INVALID_ARG and "ray 2" in msg
    bad = d.copy(); bad[1] = [0., 0., -1.01]
    st, msg = rays(ctx, o, bad, sh)
    assert st == B.RM_ERR_INVALID_ARG and "ray 1" in msg
    assert rays(ctx, o, d, B.rm_shading(B.rm_vec3(.1, .1, .1), 33, 0))[0] == B.RM_ERR_DEPTH
    assert rays(ctx, o, d, B.rm_shading(B.rm_vec3(.1, .1, .1), 32, 0))[0] == 0
    st, msg = rays(ctx, o, d, None)
    assert st == B.RM_ERR_INVALID_ARG and "shading" in msg
    assert rays(ctx, o, d, B.rm_shading(B.rm_vec3(.1, np.inf, .1), 3, 0))[0] == B.RM_ERR_INVALID_ARG
    assert rays(ctx, o, d, None, n=0)[0] == 0                        # n == 0 is RM_OK and does nothing

    p = pkg.backend.make_params(workloads.FOV, float(H), float(W), 3)
    good = [[0., 0.], [95.5, 63.5], [10.25, 3.]]
    assert samples(ctx, p, good)[0] == 0
    for xy, who in (([[0., 0.], [float(W), 1.]], "sample 1"), ([[1., float(H)]], "sample 0"), ([[-0.5, 1.]], "sample 0"),
                    ([[1., 1.], [2., 2.], [np.nan, 1.]], "sample 2"), ([[1., np.inf]], "sample 0")):
        st, msg = samples(ctx, p, xy)
        assert st == B.RM_ERR_INVALID_ARG and who in msg, (xy, msg)
    p.patch_row_begin, p.patch_row_end = 0, 1                        # a non-default band
    assert samples(ctx, p, good)[0] == B.RM_ERR_INVALID_ARG
    p.patch_row_begin, p.patch_row_end = 0, 0
    p.flags = B.RM_FLAG_FAST_FP                                      # tolerated and ignored
    fast = ctx.radiance_samples(p, good)
    p.flags = 0
    assert fast.tobytes() == ctx.radiance_samples(p, good).tobytes()
    for flag in (B.RM_FLAG_U8_COMPACT, B.RM_FLAG_F64_COMPACT, B.RM_FLAG_FAST_FP | B.RM_FLAG_U8_COMPACT, 1):
        p.flags = flag
        assert samples(ctx, p, good)[0] == B.RM_ERR_INVALID_ARG
    p.flags = 0
    p.max_depth = 33
    assert samples(ctx, p, good)[0] == B.RM_ERR_DEPTH
    p.max_depth = 3
    # the device variants refuse what they can see without touching an element
    assert L.rm_radiance_rays_device(ctx.ptr, None, None, 4, C.byref(sh), None, None) == B.RM_ERR_INVALID_ARG
    assert L.rm_radiance_rays_device(ctx.ptr, None, None, 0, C.byref(sh), None, None) == 0
    assert L.rm_radiance_samples_device(ctx.ptr, C.byref(p), None, 4, None, None) == B.RM_ERR_INVALID_ARG

    fresh = pkg.backend.Context(0)
    try:
        assert rays(fresh, o, d, sh)[0] == B.RM_ERR_NO_SCENE
        assert samples(fresh, p, good)[0] == B.RM_ERR_NO_SCENE
        assert L.rm_radiance_rays_device(fresh.ptr, None, None, 4, C.byref(sh), None, None) == B.RM_ERR_NO_SCENE
    finally:
        fresh.close()


# ---------------------------------------------------------------- 9. queries leave the frames alone
def test_radiance_queries_do_not_disturb_the_frames(pkg):
    import torch
    demo, cornell = workloads.product_scene(pkg, "demo"), workloads.product_scene(pkg, "cornell")
    rng = np.random.default_rng(9)
    o, d = GQ.random_rays(rng, 5000, (-20., -10., -50.), (20., 10., 5.))
    xy = rng.uniform((0., 0.), (640., 480.), size=(5000, 2))

    def queries(c):
        before = (c.uploads(), c.launch_stats())
        c.radiance(o, d, max_depth=4)
        c.radiance_samples(pkg.backend.make_params(1.2, 480., 640., 3), xy)           # another frame geometry
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            c.radiance_device(torch.from_numpy(o).to("cuda:0"), torch.from_numpy(d).to("cuda:0"), max_depth=6)
            c.radiance_samples_device(pkg.backend.make_params(workloads.FOV, 256., 320., 3), torch.from_numpy(xy / 2.).to("cuda:0"))
        s.synchronize()
        assert (c.uploads(), c.launch_stats()) == before

    def frames(with_queries):
        c = pkg.backend.Context(0)
        out = []
        p = pkg.backend.make_params(workloads.FOV, 1080., 1920., 5)
        for step in range(6):
            if step == 4:
                c.upload(cornell.flatten())
            elif step == 0:
                c.upload(demo.flatten())
            if step == 3:
                c.set_camera((0., 1., -2.))
            if with_queries and step in (1, 2, 4):
                queries(c)
            f = np.zeros((1080, 1920, 3))
            c.render(p, f)
            out.append(f)
        c.close()
        return out

    plain, queried = frames(False), frames(True)
    for k, (a, b) in enumerate(zip(plain, queried)):
        assert a.tobytes() == b.tobytes(), "frame %d differs once radiance queries ran in between" % k


# ---------------------------------------------------------------- 10. supersampling
def test_supersampled_frames(pkg, sets, orc):
    scene, oscene = sets.scene("demo")
    r = pkg.create_renderer(workloads.FOV, 64., 64.)
    plain = pkg.create_frame_buffer(64, 64)
    r.render(plain, scene)
    frames = {}
    for n in (1, 2, 3):
        fb = pkg.create_frame_buffer(64, 64)
        r.render_supersampled(fb, scene, n)
        frames[n] = fb.buffer.copy()
    assert worst(frames[1], plain.buffer) < TIGHT
    cam = oscene.c.camera.tup()
    desc = scene.flatten().desc()
    for n in (2, 3):
        xy = RR.supersample_positions(64, 64, n)
        d = RR.sample_directions(xy, orc.renderer(64, 64))
        rgb, _, shape = orc.cast(oscene, cam, d, 3, normalize=True, want_first=True)
        mean = rgb.reshape(64, 64, n * n, 3).sum(axis=2) / float(n * n)
        delta = worst(frames[n], mean)
        print("supersampling n = %d: max |delta| %.3e" % (n, delta))
        assert delta < TIGHT
    # a sphere's silhouette: a pixel some of whose nine samples first hit a sphere while others hit something else, or nothing
    spheres = np.array([desc.shapes[k].kind == pkg._lib.RM_SHAPE_SPHERE for k in range(desc.n_shapes)])
    on_sphere = (shape >= 0) & spheres[np.maximum(shape, 0)]
    per_pixel = on_sphere.reshape(64, 64, 9)
    silhouette = per_pixel.any(axis=2) & ~per_pixel.all(axis=2)
    assert silhouette.sum() > 10
    diff = np.abs(frames[3] - frames[1]).max(axis=2)
    print("supersampling: %d silhouette pixels, largest change n = 1 -> 3 among them %.3e" % (int(silhouette.sum()), float(diff[silhouette].max())))
    assert (diff[silhouette] > 1e-3).any(), "no silhouette pixel changes under supersampling"
    # 64 x 70: the last six rows keep what they held
    r70 = pkg.create_renderer(workloads.FOV, 70., 64.)
    fb = pkg.create_frame_buffer(64, 70)
    fb.buffer[:] = -3.5
    r70.render_supersampled(fb, scene, 2)
    assert np.all(fb.buffer[64:] == -3.5) and not (fb.buffer[:64] == -3.5).any()
    xy = RR.supersample_positions(64, 64, 2)
    ref = orc.cast(oscene, cam, RR.sample_directions(xy, orc.renderer(64, 70)), 3, normalize=True)
    assert worst(fb.buffer[:64], ref.reshape(64, 64, 4, 3).sum(axis=2) / 4.) < TIGHT
