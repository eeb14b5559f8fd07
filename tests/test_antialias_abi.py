"""CPU-side checks of the adaptive anti-aliasing (include/rusty_marcher_amd.h, "adaptive anti-aliasing").

1. The three entry points are exported, bound by ctypes, the Rust shim and the C++ mirror with the header's shapes, rm_refine
   is 16 bytes everywhere, rm_build_info says " antialias", rm_refine_workspace returns the stated sizes, a NULL context is
   refused, and the Python wrappers raise before the library is called.
2. tests/antialias_reference.py -- the yardstick of the GPU tests -- does what the header states on hand-made frames.
3. It is pinned on the oracle's frames: at the threshold the GPU tests use the masks are neither empty nor full, hold the
   committed number of pixels, and NO pixel's contrast lies within 1e-6 of the threshold -- the condition under which
   tests/test_gpu_antialias.py may demand the mask exactly."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import antialias_reference as AR
import radiance_reference as RR
import test_rust_binding as RB
import workloads

FUNCTIONS = ["rm_refine_workspace", "rm_refine_device", "rm_render_antialiased"]


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_antialias_abi"))


# ---------------------------------------------------------------- the ABI
def test_antialias_symbols_are_exported_and_bound(pkg):
    L = pkg.lib()
    for name in FUNCTIONS:
        assert hasattr(L, name), "library does not export %s" % name
        assert name in pkg._lib.SIGNATURES
    for name in ("refine_workspace", "refine_device", "render_antialiased"):
        assert callable(getattr(pkg.backend.Context, name))
    assert callable(pkg.Renderer.render_antialiased)


def test_rm_refine_is_16_bytes_in_c_ctypes_and_rust(pkg, entry, tmp_path):
    src = tmp_path / "refine.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rusty_marcher_amd.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu\\n", sizeof(rm_refine), offsetof(rm_refine, n), offsetof(rm_refine, _pad), offsetof(rm_refine, threshold));'
                   'return 0;}\n')
    exe = tmp_path / "refine"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(entry.ROOT, "include"),
                           str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == [16, 0, 4, 8]
    S = pkg._lib.rm_refine
    assert C.sizeof(S) == 16 and S.n.offset == 0 and S._pad.offset == 4 and S.threshold.offset == 8
    c, r = RB.header_structs(), RB.rust_structs()
    assert c["rm_refine"] == r["RmRefine"] == [("n", "u32"), ("_pad", "u32"), ("threshold", "f64")]


def test_antialias_functions_have_the_header_shapes_in_the_rust_shim_and_the_cpp_mirror(entry):
    c, r = RB.header_functions(), RB.rust_functions()
    for name in FUNCTIONS:
        assert name in c and name in r, name
        assert c[name] == r[name], "%s: header %s, gpu.rs %s" % (name, c[name], r[name])
    assert c["rm_refine_workspace"] == ("i32", ["ptr", "ptr"])
    assert c["rm_refine_device"] == ("i32", ["ptr"] * 7)
    assert c["rm_render_antialiased"] == ("i32", ["ptr"] * 6)
    text = open(RB.RUST).read()
    assert re.search(r"pub fn render_antialiased\(\s*&mut self", text) and "rm_render_antialiased(self.ctx" in text
    hpp = open(os.path.join(entry.PKG_DIR, "host", "rusty_marcher.hpp")).read()
    assert re.search(r"render_antialiased\(framebuffer::FrameBuffer", hpp) and "rm_render_antialiased(" in hpp


def test_cpp_mirror_compiles_with_the_antialiased_render(entry, tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "rusty_marcher.hpp"\nusing namespace rusty_marcher;\n'
                   'std::string frame(renderer::Renderer &r, framebuffer::FrameBuffer &fb, const scene::Scene &sc) {'
                   ' return r.render_antialiased(fb, sc, 3u, 0.125); }\n'
                   'int main() { return sizeof(rm_refine) == 16 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(entry.ROOT, "include"),
                           "-I", os.path.join(entry.PKG_DIR, "host"), str(src)])


def test_build_info_announces_antialias(pkg):
    L = pkg.lib()
    assert " antialias" in L.rm_build_info().decode()
    assert L.rm_abi_version() == 5


def test_refine_workspace_sizes(pkg):
    L, B, K = pkg.lib(), pkg._lib, pkg.backend
    for w, h, rows in ((64, 64, 64), (96, 80, 64), (1920, 1080, 1056)):
        p = K.make_params(workloads.FOV, float(h), float(w), 3)
        b = C.c_size_t(0)
        assert L.rm_refine_workspace(C.byref(p), C.byref(b)) == 0
        want = 4 * (1 + rows * w)
        want += -want % 256
        assert b.value == want and want % 256 == 0 and want - 4 * (1 + rows * w) < 256
        assert K.Context.refine_workspace(_NoContext(L), p) == want
    assert [4 * (1 + 64 * 64), 4 * (1 + 1056 * 1920)] == [16388, 8110084]     # ... rounded up: 16640 and 8110336
    p = K.make_params(workloads.FOV, 64., 100., 3)
    b = C.c_size_t(77)
    assert L.rm_refine_workspace(C.byref(p), C.byref(b)) == B.RM_ERR_DIMENSIONS and b.value == 77
    assert L.rm_refine_workspace(None, C.byref(b)) == B.RM_ERR_INVALID_ARG
    assert L.rm_refine_workspace(C.byref(p), None) == B.RM_ERR_INVALID_ARG


class _NoContext:
    """A Context without an rm_ctx: for the calls that need none."""
    device, ptr = 0, None

    def __init__(self, L):
        self.L = L


def test_antialias_entry_points_refuse_null_context(pkg):
    L, B = pkg.lib(), pkg._lib
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 3)
    r = B.rm_refine(2, 0, 0.125)
    frame = np.full((64, 64, 3), 7.25)
    n = C.c_uint32(99)
    assert L.rm_refine_device(None, C.byref(p), C.byref(r), None, None, None, None) == B.RM_ERR_INVALID_ARG
    assert b"NULL ctx" in L.rm_last_error(None)
    assert L.rm_render_antialiased(None, C.byref(p), C.byref(r), frame.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n), None) == B.RM_ERR_INVALID_ARG
    assert b"NULL ctx" in L.rm_last_error(None)
    assert np.all(frame == 7.25) and n.value == 99                    # nothing written


class _NoLibrary:
    """A Context whose library must not be reached: the wrappers refuse before they call it."""
    device, ptr = 0, None

    class L:
        def __getattr__(self, name):
            raise AssertionError("the library was called: %s" % name)
    L = L()


def test_python_wrappers_check_before_the_library_sees_anything(pkg):
    import torch
    K, ctx = pkg.backend, _NoLibrary()
    p = K.make_params(workloads.FOV, 64., 64., 3)
    host = np.zeros((64, 64, 3))
    t = torch.zeros((64, 64, 3), dtype=torch.float64)
    for n, thr in ((0, 0.125), (9, 0.125), (-1, 0.125), (2.5, 0.125), (True, 0.125), (2, float("nan")), (2, np.nan)):
        with pytest.raises(ValueError):
            K.Context.render_antialiased(ctx, p, host, n, thr)
        with pytest.raises(ValueError):
            K.Context.refine_device(ctx, p, t, n, thr)
        with pytest.raises(ValueError):
            pkg.create_renderer(workloads.FOV, 64., 64.).render_antialiased(None, None, n, thr)
    # the frame: a float64 torch tensor of the frame's shape on the context's device, contiguous; the mask likewise, uint8
    ctx.refine_workspace = lambda params: 16640
    for frame in (host, t.float(), t, torch.zeros((64, 32, 3), dtype=torch.float64)):
        with pytest.raises(ValueError):                               # numpy; float32; on the CPU; wrong shape
            K.Context.refine_device(ctx, p, frame, 2, 0.125)
    assert K._refine(8, -1.).n == 8 and K._refine(1, float("inf")).threshold == float("inf") and K._refine(2., 0).n == 2


# ---------------------------------------------------------------- the yardstick does what the header states
def test_contrast_and_mask_on_hand_made_frames():
    f = np.zeros((4, 3, 3))
    f[1, 1] = [0.5, -2., 0.25]
    c = AR.contrast(f, 4)
    assert c[1, 1] == 2. and c[0, 1] == c[2, 1] == c[1, 0] == c[1, 2] == 2. and c[0, 0] == c[3, 1] == 0.      # no diagonal neighbours
    # the rows below `rows` are not looked at: row rows - 1 has no lower neighbour
    assert AR.contrast(f, 1)[0].tolist() == [0., 0., 0.] and AR.contrast(f, 2)[0].tolist() == [0., 2., 0.]
    # a pixel without a neighbour has contrast 0
    assert AR.contrast(np.full((1, 1, 3), 9.), 1).tolist() == [[0.]]
    # raw radiance, neither normalised nor clamped
    g = np.zeros((1, 2, 3)); g[0, 1, 2] = 1e6
    assert AR.contrast(g, 1).tolist() == [[1e6, 1e6]]
    # a NaN makes its comparisons false: the NaN pixel and its neighbours see the other neighbours only
    h = np.zeros((1, 3, 3)); h[0, 1, 0] = np.nan; h[0, 1, 1] = 3.; h[0, 2, 1] = 1.
    assert AR.contrast(h, 1).tolist() == [[3., 3., 2.]]
    # the ends of the threshold
    assert not AR.mask(f, 4, np.inf).any() and AR.mask(f, 4, -1.).all() and AR.mask(np.full((1, 1, 3), 9.), 1, -1.).all()
    assert AR.mask(f, 4, 2.).sum() == 0 and AR.mask(f, 4, 1.9999).sum() == 5           # strictly greater
    assert AR.nearest_to(f, 4, 1.5) == 0.5


def test_refined_frames_on_hand_made_samples():
    rng = np.random.default_rng(5)
    f = rng.uniform(size=(34, 4, 3))
    m = np.zeros((32, 4), bool); m[3, 1] = m[31, 3] = True
    s = rng.uniform(size=(2, 9, 3))
    out = AR.refined(f, m, s)
    seq = s[1, 0]
    for t in range(1, 9):
        seq = seq + s[1, t]
    assert out[31, 3].tobytes() == (seq / 9.).tobytes()
    keep = np.ones((34, 4), bool); keep[3, 1] = keep[31, 3] = False
    assert out[keep].tobytes() == f[keep].tobytes() and out[32:].tobytes() == f[32:].tobytes()
    # every pixel's samples in the [y][x][j][i] order: the listed pixels' are picked out
    every = rng.uniform(size=(32 * 4, 4, 3))
    assert AR.refined(f, m, every).tobytes() == AR.refined(f, m, every[m.ravel()]).tobytes()
    # the positions are the rows of supersample_positions, i inner
    xy = AR.positions(m, 2).reshape(2, 4, 2)
    assert xy[0].tolist() == [[1., 3.], [1.5, 3.], [1., 3.5], [1.5, 3.5]] and xy[1, 3].tolist() == [3.5, 31.5]
    # a full mask is the supersampled frame
    full = AR.refined(f, np.ones((32, 4), bool), every)
    assert np.abs(full[:32] - every.reshape(32, 4, 4, 3).sum(axis=2) / 4.).max() < 1e-15


# ---------------------------------------------------------------- ... and is pinned on the oracle's frames
@pytest.mark.parametrize("key", list(AR.FRAMES), ids=lambda k: "%s-%dx%d-depth%d" % k)
def test_masks_of_the_oracle_frames_are_decided_with_room(pkg, O, orc, key):
    name, w, h, depth = key
    Y = AR.Yardstick(pkg, O, orc)
    f = Y.frame(name, w, h, depth)
    rows = AR.rows_of(h)
    m = AR.mask(f, rows, AR.THRESHOLD)
    near = AR.nearest_to(f, rows, AR.THRESHOLD)
    print("%s %dx%d depth %d: %d of %d pixels refined at %g, the nearest contrast %.3e away" % (name, w, h, depth, int(m.sum()), m.size, AR.THRESHOLD, near))
    assert 0 < m.sum() < m.size
    assert near > AR.MARGIN, "a contrast lies within %g of the threshold: the GPU's mask could differ in that pixel" % AR.MARGIN
    assert int(m.sum()) == AR.FRAMES[key]


def test_the_oriented_frame_of_the_yardstick_is_orc_render_under_the_fixed_view(pkg, O, orc):
    Y = AR.Yardstick(pkg, O, orc)
    fixed = Y.frame("demo", 64, 64, 3)
    as_view = Y.frame("demo", 64, 64, 3, (Y.eye("demo"), RR.FIXED_VIEW))
    assert fixed.tobytes() == as_view.tobytes()


def test_a_frame_refined_everywhere_is_the_supersampled_frame(pkg, O, orc):
    Y = AR.Yardstick(pkg, O, orc)
    m, out = Y.refined("demo", 32, 32, 3, 2, -1.)
    assert m.all()
    xy = RR.supersample_positions(32, 32, 2)
    rgb = orc.cast(Y.scene("demo")[1], Y.eye("demo"), RR.sample_directions(xy, orc.renderer(32, 32)), 3, normalize=True)
    assert np.abs(out - rgb.reshape(32, 32, 4, 3).sum(axis=2) / 4.).max() < 1e-15
    # ... and n = 1 gives the rendered frame back
    _, one = Y.refined("demo", 32, 32, 3, 1, -1.)
    assert one.tobytes() == Y.frame("demo", 32, 32, 3).tobytes()
