"""Adaptive anti-aliasing on the GPU (-m gpu): rm_refine_device and rm_render_antialiased through the C ABI, the Python
bindings and the C++ mirror, against tests/antialias_reference.py -- contrast, mask and sample means in numpy over the
CPU oracle's frames and its cast_ray (pinned on the CPU by tests/test_antialias_abi.py).

The masks are demanded exactly and every channel of every refined pixel within TIGHT = 1e-9 of the yardstick, no pixel left
out: the frames agree with the oracle's to 1e-9 and no contrast of a tested frame lies within 1e-6 of the threshold (asserted
in tests/test_antialias_abi.py; a test that uses another frame or threshold asserts it first).  Largest deviations observed
on an MI355X are recorded in DESIGN.md section 6f."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import antialias_reference as AR
import radiance_reference as RR
import test_gpu_query as GQ
import workloads

pytestmark = pytest.mark.gpu

TIGHT = AR.TIGHT
THR = AR.THRESHOLD


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_antialias"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return AR.Yardstick(pkg, O, orc)


def upload(ctx, scene):
    ctx.orient(None)
    ctx.upload(scene.flatten())


def worst(got, ref):
    return float(np.abs(got - ref).max(initial=0.))


class Run:
    """One rm_render_device + rm_refine_device on torch's current stream: the frame as rendered, as refined, the mask, the
    workspace's count and its list (sorted)."""

    def __init__(self, pkg, c, w, h, depth, n, threshold, frame_fill=0., mask_fill=0xAB, refine_flags=0):
        import torch
        self.p = p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)
        dev = torch.full((h, w, 3), frame_fill, dtype=torch.float64, device="cuda:0")
        m = torch.full((h, w), mask_fill, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        c.render_device(p, dev.data_ptr())
        torch.cuda.synchronize()
        self.rendered = dev.cpu().numpy()
        p.flags = refine_flags
        ws = c.refine_device(p, dev, n, threshold, mask=m)
        torch.cuda.synchronize()
        ws = ws.cpu().numpy()
        self.count = int(ws[0])
        self.listed = np.sort(ws[1:1 + self.count])
        self.frame = dev.cpu().numpy()
        self.mask = m.cpu().numpy()


def check_against(run, m_ref, f_ref, rows, what):
    """Mask, list and frame of a Run against the yardstick's mask and refined frame."""
    w = m_ref.shape[1]
    assert np.array_equal(run.mask[:rows], m_ref.astype(np.uint8)), "%s: %d mask bytes differ" % (what, int((run.mask[:rows] != m_ref).sum()))
    assert run.count == int(m_ref.sum())
    assert np.array_equal(run.listed, np.flatnonzero(m_ref.ravel()))                # indices y * frame_width + x
    delta = worst(run.frame[:rows][m_ref], f_ref[:rows][m_ref])
    print("%s: %d of %d pixels refined, max |delta| %.3e among them" % (what, run.count, rows * w, delta))
    assert delta < TIGHT
    assert run.frame[:rows][~m_ref].tobytes() == run.rendered[:rows][~m_ref].tobytes()   # unrefined pixels keep their bytes


# ---------------------------------------------------------------- 1. mask, list and frame against the yardstick
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("name,depth", [("demo", 3), ("cornell", 3), ("synthetic256", 6)])
def test_mask_list_and_frame_match_the_yardstick(pkg, ctx, Y, name, depth, n):
    assert (name, 64, 64, depth) in AR.FRAMES                        # decided with room: tests/test_antialias_abi.py
    upload(ctx, Y.scene(name)[0])
    run = Run(pkg, ctx, 64, 64, depth, n, THR)
    assert worst(run.rendered, Y.frame(name, 64, 64, depth)) < TIGHT
    m_ref, f_ref = Y.refined(name, 64, 64, depth, n, THR)
    assert int(m_ref.sum()) == AR.FRAMES[(name, 64, 64, depth)]
    check_against(run, m_ref, f_ref, 64, "%s depth %d n = %d" % (name, depth, n))


# ---------------------------------------------------------------- 2. groups and tails
def test_groups_tails_and_the_capped_grid(pkg, ctx, Y, monkeypatch):
    """Demo 32x32: 436 listed pixels, no multiple of 64 (n = 1), 4 (n = 4: P = 4), 2 or 7; n = 5 leaves 14 lanes of a wave
    without a sample, n = 8 fills a wave with one pixel.  RM_REFINE_MAX_BLOCKS = 1 and 3 (read at rm_init: contexts of their
    own) drive the loop over the groups and its tail; nothing changes, byte for byte."""
    assert AR.FRAMES[("demo", 32, 32, 3)] == 436
    scene = Y.scene("demo")[0]
    upload(ctx, scene)
    free = {}
    for n in (1, 4, 5, 8):
        free[n] = run = Run(pkg, ctx, 32, 32, 3, n, THR)
        m_ref, f_ref = Y.refined("demo", 32, 32, 3, n, THR)
        check_against(run, m_ref, f_ref, 32, "demo 32x32 n = %d (P = %d)" % (n, 64 // (n * n)))
    for cap in (1, 3):
        monkeypatch.setenv("RM_REFINE_MAX_BLOCKS", str(cap))
        c = pkg.backend.Context(0)
        try:
            c.upload(scene.flatten())
            for n in (1, 4, 5, 8):
                run = Run(pkg, c, 32, 32, 3, n, THR)
                what = "%d workgroup(s), n = %d" % (cap, n)
                assert run.count == free[n].count == 436 and np.array_equal(run.listed, free[n].listed), what
                assert run.mask.tobytes() == free[n].mask.tobytes(), what
                assert run.frame.tobytes() == free[n].frame.tobytes(), what
        finally:
            c.close()


# ---------------------------------------------------------------- 3. the ends of the threshold
def test_ends_of_the_threshold(pkg, ctx, Y, orc):
    scene, oscene = Y.scene("demo")
    upload(ctx, scene)
    none = Run(pkg, ctx, 64, 64, 3, 3, float("inf"))
    assert none.count == 0 and none.frame.tobytes() == none.rendered.tobytes() and not none.mask.any()
    r = pkg.create_renderer(workloads.FOV, 64., 64.)
    for n in (2, 3):
        every = Run(pkg, ctx, 64, 64, 3, n, -1.)
        assert every.count == 64 * 64 and every.mask.all() and np.array_equal(every.listed, np.arange(64 * 64))
        fb = pkg.create_frame_buffer(64, 64)
        r.render_supersampled(fb, scene, n)
        xy = RR.supersample_positions(64, 64, n)
        rgb = orc.cast(oscene, Y.eye("demo"), RR.sample_directions(xy, orc.renderer(64, 64)), 3, normalize=True)
        means = AR.refined(every.rendered, np.ones((64, 64), bool), rgb.reshape(64 * 64, n * n, 3))
        d_super, d_oracle = worst(every.frame, fb.buffer), worst(every.frame, means)
        print("threshold -1, n = %d: against render_supersampled %.3e, against the oracle's sample means %.3e" % (n, d_super, d_oracle))
        assert d_super < TIGHT and d_oracle < TIGHT
    upload(ctx, scene)                                               # (the Renderer's context is another one; this one kept its scene)
    one = Run(pkg, ctx, 64, 64, 3, 1, -1.)
    assert one.count == 64 * 64 and worst(one.frame, one.rendered) < TIGHT


# ---------------------------------------------------------------- 4. the rows a render leaves alone
@pytest.mark.parametrize("sentinel", [float("nan"), 1e6])
def test_rows_below_the_last_patch_row_are_neither_read_nor_written(pkg, ctx, Y, sentinel):
    """96x80: rows = 64.  The frame holds a sentinel beforehand -- NaN, and 1e6, which a look from row 63 down at row 64 would
    turn into a contrast far above the threshold -- and the mask 0xAB."""
    upload(ctx, Y.scene("demo")[0])
    f = Y.frame("demo", 96, 80, 3)
    assert AR.nearest_to(f, 64, THR) > AR.MARGIN and 0 < AR.mask(f, 64, THR)[63].sum() < 96
    run = Run(pkg, ctx, 96, 80, 3, 2, THR, frame_fill=sentinel)
    m_ref, f_ref = Y.refined("demo", 96, 80, 3, 2, THR)
    check_against(run, m_ref, f_ref, 64, "demo 96x80, sentinel %r" % sentinel)
    assert np.array_equal(run.mask[63], m_ref[63].astype(np.uint8))  # the reference never looked at row 64
    below = np.full((16, 96, 3), sentinel)
    assert run.frame[64:].tobytes() == below.tobytes() and run.rendered[64:].tobytes() == below.tobytes()
    assert np.all(run.mask[64:] == 0xAB)
    assert run.listed.max() < 64 * 96


# ---------------------------------------------------------------- 5. the oriented context
@pytest.mark.parametrize("n", [2, 3])
def test_oriented_context(pkg, ctx, Y, n):
    scene = Y.scene("demo")[0]
    upload(ctx, scene)
    try:
        lo, hi = GQ.bounds_of(scene.flatten().desc())
        pos, _, _ = ctx.camera()
        eye = np.array([pos.x, pos.y, pos.z]) + np.array([0.12, 0.06, 0.]) * np.linalg.norm(hi - lo)
        ctx.look_at(tuple(eye), tuple((lo + hi) / 2.))
        pos, basis, on = ctx.camera()
        assert on
        view = ((pos.x, pos.y, pos.z), RR.basis_tuple(basis))
        f = Y.frame("demo", 64, 64, 3, view)
        near = AR.nearest_to(f, 64, THR)
        print("side view: the nearest contrast lies %.3e from the threshold" % near)
        assert near > AR.MARGIN                                       # another frame: its mask may be demanded exactly only then
        run = Run(pkg, ctx, 64, 64, 3, n, THR)
        assert worst(run.rendered, f) < TIGHT
        m_ref, f_ref = Y.refined("demo", 64, 64, 3, n, THR, view)
        assert 0 < m_ref.sum() < m_ref.size
        check_against(run, m_ref, f_ref, 64, "demo from the side, n = %d" % n)
    finally:
        ctx.orient(None)


# ---------------------------------------------------------------- 6. state
def test_a_refine_leaves_the_render_state_alone(pkg):
    import torch
    demo = workloads.product_scene(pkg, "demo")
    p = pkg.backend.make_params(workloads.FOV, 1080., 1920., 5)

    def frames(with_refine):
        c = pkg.backend.Context(0)
        try:
            c.upload(demo.flatten())
            first = np.zeros((1080, 1920, 3))
            c.render(p, first)
            if with_refine:
                before = (c.uploads(), c.launch_stats())
                dev = torch.from_numpy(first).to("cuda:0")
                ws = c.refine_device(p, dev, 2, THR)
                torch.cuda.synchronize()
                assert 0 < int(ws[0]) < 1056 * 1920
                assert (c.uploads(), c.launch_stats()) == before
            again = np.zeros((1080, 1920, 3))
            c.render(p, again)
            return first, again
        finally:
            c.close()

    plain, refined = frames(False), frames(True)
    for k, (a, b) in enumerate(zip(plain, refined)):
        assert a.tobytes() == b.tobytes(), "frame %d differs once a refine ran in between" % (2 * k + 1)


# ---------------------------------------------------------------- 7. the host path
CPP_MAIN = r"""
#include <cstdio>
#include "rusty_marcher.hpp"
using namespace rusty_marcher;
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    scene::Scene sc = scene::Scene::create_default();
    framebuffer::FrameBuffer fb = framebuffer::create_frame_buffer(64, 64);
    renderer::Renderer r = renderer::create_renderer(1.5, 64., 64.);
    r.render_antialiased(fb, sc, 3u, 0.125);
    std::FILE *f = std::fopen(argv[1], "wb");
    if (!f) return 3;
    for (const auto &row : fb.buffer) std::fwrite(row.data(), sizeof(Vec3f), row.size(), f);
    std::fclose(f);
    std::printf("refined %u\n", r.last_refined);
    return 0;
}
"""


def test_host_path_python_and_the_cpp_mirror(pkg, entry, ctx, Y, capsys, tmp_path):
    assert workloads.FOV == 1.5
    scene = Y.scene("demo")[0]
    m_ref, f_ref = Y.refined("demo", 64, 64, 3, 3, THR)
    # rm_render_antialiased
    upload(ctx, scene)
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 3)
    host = np.full((64, 64, 3), -3.5)
    timing, count = ctx.render_antialiased(p, host, 3, THR)
    assert count == int(m_ref.sum()) and worst(host, f_ref) < TIGHT and timing.kernel_ms > 0.
    plain = np.zeros((64, 64, 3))
    ctx.render(p, plain)
    assert host[~m_ref].tobytes() == plain[~m_ref].tobytes()
    # ... 64 x 70: the six last rows keep what they held
    p70 = pkg.backend.make_params(workloads.FOV, 70., 64., 3)
    host70 = np.full((70, 64, 3), -3.5)
    _, count70 = ctx.render_antialiased(p70, host70, 2, -1.)
    assert count70 == 64 * 64 and np.all(host70[64:] == -3.5) and not (host70[:64] == -3.5).any()
    # Renderer.render_antialiased: the prints and the return value of render()
    r = pkg.create_renderer(workloads.FOV, 64., 64.)
    fb = pkg.create_frame_buffer(64, 64)
    capsys.readouterr()
    message = r.render_antialiased(fb, scene, 3, THR)
    out = capsys.readouterr().out
    assert message.startswith("Scene rendered in ") and message in out
    assert "Rendering using patches of size 32, using 4 patches overall" in out and "compute units used" in out
    assert r.last_refined == count and fb.buffer.tobytes() == host.tobytes()
    # the C++ mirror, from compiled code
    src, exe, dump = tmp_path / "aa.cpp", tmp_path / "aa", tmp_path / "aa.f64"
    src.write_text(CPP_MAIN)
    lib_dir = os.path.join(entry.PKG_DIR, "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(entry.ROOT, "include"), "-I", os.path.join(entry.PKG_DIR, "host"),
                           str(src), "-o", str(exe), "-L", lib_dir, "-lrusty_marcher_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath," + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")])
    log = subprocess.check_output([str(exe), str(dump)]).decode()
    assert "refined %d" % count in log
    assert np.fromfile(str(dump)).tobytes() == host.tobytes()


# ---------------------------------------------------------------- 8. errors
def test_refusals_leave_frame_workspace_and_mask_alone(pkg, ctx, Y):
    import torch
    L, B = pkg.lib(), pkg._lib
    upload(ctx, Y.scene("demo")[0])
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 3)
    frame = torch.full((64, 64, 3), 7.25, dtype=torch.float64, device="cuda:0")
    ws = torch.full((ctx.refine_workspace(p) // 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    mask = torch.full((64, 64), 0xAB, dtype=torch.uint8, device="cuda:0")

    def call(c, params, refine, f=frame, w=ws):
        st = L.rm_refine_device(c.ptr, C.byref(params), C.byref(refine) if refine is not None else None,
                                C.c_void_p(f.data_ptr()) if f is not None else None, C.c_void_p(w.data_ptr()) if w is not None else None,
                                C.c_void_p(mask.data_ptr()), None)
        torch.cuda.synchronize()
        assert st != 0
        assert bool((frame == 7.25).all()) and bool((ws == 0x5A5A5A5A).all()) and bool((mask == 0xAB).all())
        return st, L.rm_last_error(c.ptr).decode()

    E = B.RM_ERR_INVALID_ARG
    for n in (0, 9):
        st, msg = call(ctx, p, B.rm_refine(n, 0, THR))
        assert st == E and "refine.n" in msg
    st, msg = call(ctx, p, B.rm_refine(2, 0, float("nan")))
    assert st == E and "threshold" in msg
    st, msg = call(ctx, p, None)
    assert st == E and "refine" in msg
    assert call(ctx, p, B.rm_refine(2, 0, THR), f=None)[0] == E and "frame" in L.rm_last_error(ctx.ptr).decode()
    assert call(ctx, p, B.rm_refine(2, 0, THR), w=None)[0] == E and "workspace" in L.rm_last_error(ctx.ptr).decode()
    good = B.rm_refine(2, 0, THR)
    for flag in (B.RM_FLAG_U8_COMPACT, B.RM_FLAG_F64_COMPACT, B.RM_FLAG_FAST_FP | B.RM_FLAG_F64_COMPACT):
        p.flags = flag
        assert call(ctx, p, good)[0] == E
    p.flags = 0
    p.patch_row_begin, p.patch_row_end = 0, 1                        # a non-default band
    assert call(ctx, p, good)[0] == E
    p.patch_row_begin, p.patch_row_end = 0, 0
    p.max_depth = 33
    assert call(ctx, p, good)[0] == B.RM_ERR_DEPTH
    p.max_depth = 3
    p.background.y = float("inf")
    st, msg = call(ctx, p, good)
    assert st == E and "background" in msg
    p.background.y = 0.1
    odd = pkg.backend.make_params(workloads.FOV, 64., 100., 3)
    assert call(ctx, odd, good)[0] == B.RM_ERR_DIMENSIONS
    fresh = pkg.backend.Context(0)
    try:
        assert call(fresh, p, good)[0] == B.RM_ERR_NO_SCENE
        host = np.full((64, 64, 3), 7.25)
        n = C.c_uint32(99)
        assert L.rm_render_antialiased(fresh.ptr, C.byref(p), C.byref(good), host.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n), None) == B.RM_ERR_NO_SCENE
        assert np.all(host == 7.25) and n.value == 99
    finally:
        fresh.close()
    # rm_render_antialiased refuses the compact layouts and a band before it renders
    host = np.full((64, 64, 3), 7.25)
    hp = host.ctypes.data_as(C.POINTER(C.c_double))
    before = ctx.launch_stats()
    p.flags = B.RM_FLAG_F64_COMPACT
    assert L.rm_render_antialiased(ctx.ptr, C.byref(p), C.byref(good), hp, None, None) == E
    p.flags = 0
    p.patch_row_begin, p.patch_row_end = 1, 2
    assert L.rm_render_antialiased(ctx.ptr, C.byref(p), C.byref(good), hp, None, None) == E
    p.patch_row_begin, p.patch_row_end = 0, 0
    assert L.rm_render_antialiased(ctx.ptr, C.byref(p), C.byref(B.rm_refine(9, 0, THR)), hp, None, None) == E
    assert np.all(host == 7.25) and ctx.launch_stats() == before
    # what is tolerated: RM_FLAG_FAST_FP (ignored: the refine is the strict flavour), and a frame without a whole patch row
    strict, fast = Run(pkg, ctx, 64, 64, 3, 2, THR), Run(pkg, ctx, 64, 64, 3, 2, THR, refine_flags=B.RM_FLAG_FAST_FP)
    assert fast.count == strict.count == AR.FRAMES[("demo", 64, 64, 3)] and fast.frame.tobytes() == strict.frame.tobytes()
    short = pkg.backend.make_params(workloads.FOV, 31., 64., 3)
    f31 = torch.full((31, 64, 3), 7.25, dtype=torch.float64, device="cuda:0")
    w31 = ctx.refine_device(short, f31, 2, -1.)
    torch.cuda.synchronize()
    assert bool((f31 == 7.25).all()) and w31.numel() * 4 == 256      # rows == 0: RM_OK, nothing done
