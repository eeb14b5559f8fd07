"""The thin-lens camera on the GPU (-m gpu): rm_render_lens_device and rm_render_lens through the C ABI, the Python bindings
and the C++ mirror, against tests/lens_reference.py -- the lens rays in numpy, cast by the CPU oracle's cast_ray and resolved
in table order (pinned on the CPU by tests/test_lens_abi.py).

Every channel of every pixel of the rows a lens frame writes is demanded within TIGHT = 1e-9 of the yardstick, no pixel left
out; what the header calls byte for byte is demanded byte for byte.  Largest deviations observed on an MI355X are recorded in
DESIGN.md section 6g."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lens_reference as LR
import radiance_reference as RR
import test_gpu_query as GQ
import workloads

pytestmark = pytest.mark.gpu

TIGHT = LR.TIGHT
# aperture and focus per scene: the demo's are the non-vacuity pin's (tests/test_lens_abi.py); the Cornell box stands 500 away
LENS = {"demo": (LR.APERTURE, LR.FOCUS), "cornell": (12., 500.), "synthetic256": (LR.APERTURE, LR.FOCUS)}


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_lens"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return LR.Yardstick(pkg, O, orc)


def upload(ctx, scene):
    ctx.orient(None)
    ctx.upload(scene.flatten())


def worst(got, ref):
    return float(np.abs(got - ref).max(initial=0.))


def lens_frame(pkg, c, w, h, depth, aperture, focus, table, fill=0., flags=0):
    """One rm_render_lens_device on torch's current stream into a frame that held `fill` -> the frame."""
    import torch
    p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)
    p.flags = flags
    dev = torch.full((h, w, 3), fill, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    c.render_lens_device(p, dev, aperture, focus, table)
    torch.cuda.synchronize()
    return dev.cpu().numpy()


# ---------------------------------------------------------------- 1. parity with the yardstick
@pytest.mark.parametrize("n", [1, 4, 5, 7, 16, 64])
@pytest.mark.parametrize("name,depth", [("demo", 3), ("cornell", 3), ("synthetic256", 6)])
def test_lens_frames_match_the_yardstick(pkg, ctx, Y, name, depth, n):
    """32 x 32 = 1024 pixels: no multiple of P = 12 (n = 5, four idle lanes a wave) or P = 9 (n = 7); n = 64 is one pixel a
    wave, n = 1 sixty-four.  max_depth 6 takes the kernels with STACK = 32, the 256 spheres those with the hierarchy.  The
    library's table and a random valid one (a lens point on the rim included)."""
    assert 1024 % (64 // 5) and 1024 % (64 // 7)
    aperture, focus = LENS[name]
    upload(ctx, Y.scene(name)[0])
    rng = np.random.default_rng(20261200 + n)
    for what, table in (("library", ctx.lens_table(n)), ("random", LR.random_table(rng, n))):
        got = lens_frame(pkg, ctx, 32, 32, depth, aperture, focus, table, fill=float("nan"))
        ref = Y.frame(name, 32, 32, depth, aperture, focus, table)
        delta = worst(got, ref)
        print("%s depth %d, %d samples, %s table: max |delta| %.3e" % (name, depth, n, what, delta))
        assert not np.isnan(got).any() and delta < TIGHT


def test_the_pinned_frame_and_the_ends_of_the_depth(pkg, ctx, Y):
    """The demo's 64 x 64 frame of the non-vacuity pin (16 samples: 1,024 groups), and a cap of 0: the background everywhere."""
    upload(ctx, Y.scene("demo")[0])
    table = ctx.lens_table(16)
    got = lens_frame(pkg, ctx, 64, 64, 3, LR.APERTURE, LR.FOCUS, table)
    delta = worst(got, Y.frame("demo", 64, 64, 3, LR.APERTURE, LR.FOCUS, table))
    sharp = Y.frame("demo", 64, 64, 3, 0., LR.FOCUS, table)
    print("demo 64x64, 16 samples: max |delta| %.3e" % delta)
    assert delta < TIGHT and int((np.abs(got - sharp) > 0.05).any(axis=2).sum()) >= 100
    capped = lens_frame(pkg, ctx, 32, 32, 0, LR.APERTURE, LR.FOCUS, ctx.lens_table(5), fill=float("nan"))
    assert worst(capped, Y.frame("demo", 32, 32, 0, LR.APERTURE, LR.FOCUS, ctx.lens_table(5))) < TIGHT
    assert worst(capped, np.full((32, 32, 3), 0.1)) < 1e-15


# ---------------------------------------------------------------- 2. aperture 0 is the supersampled frame
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("name,depth", [("demo", 3), ("synthetic256", 6)])
def test_aperture_0_is_the_refine_kernels_frame_byte_for_byte(pkg, ctx, Y, name, depth, n):
    import torch
    upload(ctx, Y.scene(name)[0])
    p = pkg.backend.make_params(workloads.FOV, 64., 64., depth)
    dev = torch.zeros((64, 64, 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.render_device(p, dev.data_ptr())
    torch.cuda.synchronize()
    ws = ctx.refine_device(p, dev, n, -1.)
    torch.cuda.synchronize()
    assert int(ws[0]) == 64 * 64
    refined = dev.cpu().numpy()
    got = lens_frame(pkg, ctx, 64, 64, depth, 0., LR.FOCUS, LR.supersample_table(n), fill=float("nan"))
    assert got.tobytes() == refined.tobytes(), "%d pixels differ" % int((got != refined).any(axis=2).sum())
    # ... whatever the focus says
    assert lens_frame(pkg, ctx, 64, 64, depth, 0., 123.5, LR.supersample_table(n)).tobytes() == refined.tobytes()


# ---------------------------------------------------------------- 3. the grid
def test_a_capped_grid_changes_nothing(pkg, ctx, Y, monkeypatch):
    """RM_LENS_MAX_BLOCKS = 1 and 3 (read at rm_init: contexts of their own) drive the loop over the groups and its tail."""
    scene = Y.scene("demo")[0]
    upload(ctx, scene)
    tables = {n: ctx.lens_table(n) for n in (1, 5, 16, 64)}
    free = {n: lens_frame(pkg, ctx, 32, 32, 3, LR.APERTURE, LR.FOCUS, t) for n, t in tables.items()}
    for cap in (1, 3):
        monkeypatch.setenv("RM_LENS_MAX_BLOCKS", str(cap))
        c = pkg.backend.Context(0)
        try:
            c.upload(scene.flatten())
            for n, t in tables.items():
                got = lens_frame(pkg, c, 32, 32, 3, LR.APERTURE, LR.FOCUS, t, fill=float("nan"))
                assert got.tobytes() == free[n].tobytes(), "%d workgroup(s), %d samples" % (cap, n)
        finally:
            c.close()


# ---------------------------------------------------------------- 4. the oriented context
@pytest.mark.parametrize("n", [4, 7])
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
        focus = float(np.linalg.norm((lo + hi) / 2. - eye))
        table = ctx.lens_table(n)
        got = lens_frame(pkg, ctx, 64, 64, 3, LR.APERTURE, focus, table, fill=float("nan"))
        ref = Y.frame("demo", 64, 64, 3, LR.APERTURE, focus, table, view)
        plain = Y.frame("demo", 64, 64, 3, LR.APERTURE, focus, table)
        delta = worst(got, ref)
        print("demo from the side, %d samples: max |delta| %.3e" % (n, delta))
        assert delta < TIGHT and worst(ref, plain) > 0.05             # ... and it is another picture than the fixed view's
    finally:
        ctx.orient(None)


# ---------------------------------------------------------------- 5. the rows a lens frame leaves alone
def test_rows_below_the_last_patch_row_and_the_memory_behind_the_frame_keep_their_bytes(pkg, ctx, Y):
    """32 x 40: rows = 32.  The frame, its eight last rows and a guard region behind it hold NaN beforehand."""
    import torch
    upload(ctx, Y.scene("demo")[0])
    p = pkg.backend.make_params(workloads.FOV, 40., 32., 3)
    guard = 4096
    buf = torch.full((40 * 32 * 3 + guard,), float("nan"), dtype=torch.float64, device="cuda:0")
    before = buf.cpu().numpy().copy()
    frame = buf[:40 * 32 * 3].view(40, 32, 3)
    table = ctx.lens_table(7)
    ctx.render_lens_device(p, frame, LR.APERTURE, LR.FOCUS, table)
    torch.cuda.synchronize()
    after = buf.cpu().numpy()
    got = after[:40 * 32 * 3].reshape(40, 32, 3)
    assert worst(got[:32], Y.frame("demo", 32, 40, 3, LR.APERTURE, LR.FOCUS, table)[:32]) < TIGHT
    assert got[32:].tobytes() == before[:8 * 32 * 3].tobytes()       # NaN, bit for bit
    assert after[40 * 32 * 3:].tobytes() == before[40 * 32 * 3:].tobytes()
    # the host path copies the rows [0, 32) only
    host = np.full((40, 32, 3), -3.5)
    ctx.render_lens(p, host, LR.APERTURE, LR.FOCUS, table)
    assert host[:32].tobytes() == got[:32].tobytes() and np.all(host[32:] == -3.5)


# ---------------------------------------------------------------- 6. state
def test_lens_calls_leave_the_render_state_alone(pkg):
    import torch
    demo = workloads.product_scene(pkg, "demo")
    p = pkg.backend.make_params(workloads.FOV, 1080., 1920., 5)
    small = pkg.backend.make_params(workloads.FOV, 64., 64., 5)

    def frames(with_lens):
        c = pkg.backend.Context(0)
        try:
            c.upload(demo.flatten())
            out = []
            dev = torch.zeros((1080, 1920, 3), dtype=torch.float64, device="cuda:0") if with_lens else None
            for k in range(3):
                f = np.zeros((1080, 1920, 3))
                c.render(p, f)
                out.append(f)
                if with_lens and k < 2:                              # before, between and after: lens calls behind frames 1 and 2
                    before = (c.uploads(), c.launch_stats())
                    c.render_lens_device(p, dev, LR.APERTURE, LR.FOCUS, c.lens_table(2))
                    torch.cuda.synchronize()
                    host = np.zeros((64, 64, 3))
                    c.render_lens(small, host, LR.APERTURE, LR.FOCUS, c.lens_table(4))
                    assert bool((dev[:1056] != 0.).any()) and host.any()
                    assert (c.uploads(), c.launch_stats()) == before
            return out
        finally:
            c.close()

    plain, lensed = frames(False), frames(True)
    for k, (a, b) in enumerate(zip(plain, lensed)):
        assert a.tobytes() == b.tobytes(), "frame %d differs once lens calls ran" % (k + 1)


# ---------------------------------------------------------------- 7. the host paths
CPP_MAIN = r"""
#include <cstdio>
#include "rusty_marcher.hpp"
using namespace rusty_marcher;
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    scene::Scene sc = scene::Scene::create_default();
    framebuffer::FrameBuffer fb = framebuffer::create_frame_buffer(64, 64);
    renderer::Renderer r = renderer::create_renderer(1.5, 64., 64.);
    r.render_lens(fb, sc, 0.4, 5., 16u);
    std::FILE *f = std::fopen(argv[1], "wb");
    if (!f) return 3;
    for (const auto &row : fb.buffer) std::fwrite(row.data(), sizeof(Vec3f), row.size(), f);
    std::fclose(f);
    std::printf("kernel %.6f ms\n", r.last_timing.kernel_ms);
    return 0;
}
"""


def test_host_path_python_and_the_cpp_mirror(pkg, entry, ctx, Y, capsys, tmp_path):
    assert workloads.FOV == 1.5 and (LR.APERTURE, LR.FOCUS) == (0.4, 5.)
    scene = Y.scene("demo")[0]
    upload(ctx, scene)
    table = ctx.lens_table(16)
    device = lens_frame(pkg, ctx, 64, 64, 3, LR.APERTURE, LR.FOCUS, table)
    # rm_render_lens
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 3)
    host = np.full((64, 64, 3), -3.5)
    timing = ctx.render_lens(p, host, LR.APERTURE, LR.FOCUS, table)
    assert host.tobytes() == device.tobytes() and timing.kernel_ms > 0. and timing.total_ms >= timing.kernel_ms
    # ... twice, with a smaller and a larger frame in between: the context's buffers are grown and reused
    for w, h, n in ((32, 32, 5), (96, 64, 4)):
        q = pkg.backend.make_params(workloads.FOV, float(h), float(w), 3)
        f = np.full((h, w, 3), -3.5)
        ctx.render_lens(q, f, LR.APERTURE, LR.FOCUS, ctx.lens_table(n))
        assert f.tobytes() == lens_frame(pkg, ctx, w, h, 3, LR.APERTURE, LR.FOCUS, ctx.lens_table(n)).tobytes()
    again = np.full((64, 64, 3), -3.5)
    ctx.render_lens(p, again, LR.APERTURE, LR.FOCUS, table)
    assert again.tobytes() == device.tobytes()
    # Renderer.render_depth_of_field: the prints and the return value of render()
    r = pkg.create_renderer(workloads.FOV, 64., 64.)
    fb = pkg.create_frame_buffer(64, 64)
    capsys.readouterr()
    message = r.render_depth_of_field(fb, scene, LR.APERTURE, LR.FOCUS, 16)
    out = capsys.readouterr().out
    assert message.startswith("Scene rendered in ") and message in out
    assert "Rendering using patches of size 32, using 4 patches overall" in out and "compute units used" in out
    assert fb.buffer.tobytes() == device.tobytes() and r.last_timing.kernel_ms > 0.
    # the C++ mirror, from compiled code
    src, exe, dump = tmp_path / "dof.cpp", tmp_path / "dof", tmp_path / "dof.f64"
    src.write_text(CPP_MAIN)
    lib_dir = os.path.join(entry.PKG_DIR, "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(entry.ROOT, "include"), "-I", os.path.join(entry.PKG_DIR, "host"),
                           str(src), "-o", str(exe), "-L", lib_dir, "-lrusty_marcher_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath," + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")])
    log = subprocess.check_output([str(exe), str(dump)]).decode()
    assert "kernel " in log
    assert np.fromfile(str(dump)).tobytes() == device.tobytes()


# ---------------------------------------------------------------- 8. errors
def test_refusals_leave_the_frame_alone(pkg, ctx, Y):
    import torch
    L, B = pkg.lib(), pkg._lib
    upload(ctx, Y.scene("demo")[0])
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 3)
    frame = torch.full((64, 64, 3), 7.25, dtype=torch.float64, device="cuda:0")
    table = torch.from_numpy(LR.lens_table(4)).to("cuda:0")
    host = np.full((64, 64, 3), 7.25)
    host_table = LR.lens_table(4)
    D = C.POINTER(C.c_double)
    nan, inf = float("nan"), float("inf")

    def call(c, params, lens, t=table, f=frame):
        """Both entry points: the same status, the same message, nothing written."""
        lp = C.byref(lens) if lens is not None else None
        st = L.rm_render_lens_device(c.ptr, C.byref(params), lp, C.c_void_p(t.data_ptr()) if t is not None else None,
                                     C.c_void_p(f.data_ptr()) if f is not None else None, None)
        msg = L.rm_last_error(c.ptr).decode()
        torch.cuda.synchronize()
        st_h = L.rm_render_lens(c.ptr, C.byref(params), lp, host_table.ctypes.data_as(D) if t is not None else None,
                                host.ctypes.data_as(D) if f is not None else None, None)
        msg_h = L.rm_last_error(c.ptr).decode()
        assert st != 0 and st_h == st and msg_h.replace("rm_render_lens", "rm_render_lens_device") == msg
        assert bool((frame == 7.25).all()) and np.all(host == 7.25)
        return st, msg

    E = B.RM_ERR_INVALID_ARG
    for aperture in (-1e-9, nan, inf, -inf):
        st, msg = call(ctx, p, B.rm_lens(aperture, LR.FOCUS, 4, 0))
        assert st == E and "aperture" in msg
    for focus in (0., -5., nan, inf):
        st, msg = call(ctx, p, B.rm_lens(LR.APERTURE, focus, 4, 0))
        assert st == E and "focus" in msg
    for n in (0, 65, 2 ** 32 - 1):
        st, msg = call(ctx, p, B.rm_lens(LR.APERTURE, LR.FOCUS, n, 0))
        assert st == E and "n_samples" in msg
    good = B.rm_lens(LR.APERTURE, LR.FOCUS, 4, 0)
    st, msg = call(ctx, p, None)
    assert st == E and "NULL lens" in msg
    st, msg = call(ctx, p, good, t=None)
    assert st == E and "table" in msg
    st, msg = call(ctx, p, good, f=None)
    assert st == E and "frame" in msg
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
    p.background.y = inf
    st, msg = call(ctx, p, good)
    assert st == E and "background" in msg
    p.background.y = 0.1
    odd = pkg.backend.make_params(workloads.FOV, 64., 100., 3)
    assert call(ctx, odd, good)[0] == B.RM_ERR_DIMENSIONS
    huge = pkg.backend.make_params(workloads.FOV, 65536., 32768., 3)  # rows * frame_width = 2^31: checked before any pointer is touched
    st, msg = call(ctx, huge, good)
    assert st == B.RM_ERR_DIMENSIONS and "2^31" in msg
    fresh = pkg.backend.Context(0)
    try:
        assert call(fresh, p, good)[0] == B.RM_ERR_NO_SCENE
    finally:
        fresh.close()
    # the host variant checks every entry of the table, and names the row
    before = ctx.launch_stats()
    for row, col, value, word in ((0, 0, 1., "offset"), (1, 0, -1e-9, "offset"), (2, 1, 1., "offset"), (3, 1, nan, "finite"),
                                  (1, 2, inf, "finite"), (2, 2, 0.9, "disc"), (3, 3, -1.5, "disc")):
        bad = LR.lens_table(4)
        bad[row, col] = value
        assert not LR.table_ok(bad)
        st = L.rm_render_lens(ctx.ptr, C.byref(p), C.byref(good), bad.ctypes.data_as(D), host.ctypes.data_as(D), None)
        msg = L.rm_last_error(ctx.ptr).decode()
        assert st == E and "table row %d" % row in msg and word in msg, msg
    rim = LR.lens_table(4)
    rim[0, 2:] = (1., 1e-7)                                         # u u + v v = 1 + 1e-14: within the check's 1e-12
    assert L.rm_render_lens(ctx.ptr, C.byref(p), C.byref(good), rim.ctypes.data_as(D), host.copy().ctypes.data_as(D), None) == 0
    assert np.all(host == 7.25) and ctx.launch_stats() == before
    # what is tolerated: RM_FLAG_FAST_FP (ignored: the lens kernel is the strict flavour), and a frame without a whole patch row
    strict = lens_frame(pkg, ctx, 64, 64, 3, LR.APERTURE, LR.FOCUS, host_table)
    fast = lens_frame(pkg, ctx, 64, 64, 3, LR.APERTURE, LR.FOCUS, host_table, flags=B.RM_FLAG_FAST_FP)
    assert fast.tobytes() == strict.tobytes() and strict.any()
    short = lens_frame(pkg, ctx, 64, 31, 3, LR.APERTURE, LR.FOCUS, host_table, fill=7.25)
    assert np.all(short == 7.25)                                     # rows == 0: RM_OK, nothing done
    h31 = np.full((31, 64, 3), 7.25)
    ctx.render_lens(pkg.backend.make_params(workloads.FOV, 31., 64., 3), h31, LR.APERTURE, LR.FOCUS, host_table)
    assert np.all(h31 == 7.25)
