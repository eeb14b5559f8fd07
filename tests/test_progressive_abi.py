"""CPU-side checks of the progressive frames (include/rusty_marcher_amd.h, "progressive frames").

1. The three entry points are exported and bound by ctypes, the Rust shim and the C++ mirror with the header's shapes,
   rm_build_info says " progressive", a NULL context is refused, and the Python wrappers raise before the library is called.
2. rm_lens_sequence is tests/progressive_reference.py's numpy restatement bit for bit, every one of its 65,536 rows satisfies
   the table conditions, its prefixes of 36 and 1,296 rows are stratified (counted on the integers), and its refusals are returned.
3. tests/progressive_reference.py -- the yardstick of the GPU tests -- folds as the header states and is not vacuous: at the
   settings the GPU tests use, 192 samples are another picture than the first 4 in the committed number of pixels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lens_reference as LR
import progressive_reference as PR
import radiance_reference as RR
import test_rust_binding as RB
import workloads

FUNCTIONS = ["rm_lens_sequence", "rm_accumulate_lens_device", "rm_render_progressive"]
D = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_progressive_abi"))


# ---------------------------------------------------------------- the ABI
def test_progressive_symbols_are_exported_and_bound(pkg, entry):
    L = pkg.lib()
    header = open(os.path.join(entry.ROOT, "include", "rusty_marcher_amd.h")).read()
    lib_py = open(os.path.join(entry.PKG_DIR, "_lib.py")).read()
    for name in FUNCTIONS:
        assert hasattr(L, name), "library does not export %s" % name
        assert name in pkg._lib.SIGNATURES and '"%s"' % name in lib_py
        assert re.search(r"^rm_status %s\(" % name, header, flags=re.M), name
    assert "#define RM_PROGRESSIVE_MAX_SAMPLES 65536u" in header and "progressive frames" in header
    for name in ("lens_sequence", "accumulate_lens_device", "render_progressive"):
        assert callable(getattr(pkg.backend.Context, name))
    assert callable(pkg.Renderer.render_progressive)
    assert pkg.backend.PROGRESSIVE_MAX_SAMPLES == PR.MAX_SAMPLES == 65536


def test_progressive_functions_have_the_header_shapes_in_the_rust_shim_and_the_cpp_mirror(entry):
    c, r = RB.header_functions(), RB.rust_functions()
    for name in FUNCTIONS:
        assert name in c and name in r, name
        assert c[name] == r[name], "%s: header %s, gpu.rs %s" % (name, c[name], r[name])
    assert c["rm_lens_sequence"] == ("i32", ["u32", "u32", "ptr"])
    assert c["rm_accumulate_lens_device"] == ("i32", ["ptr"] * 4 + ["u32"] + ["ptr"] * 4)
    assert c["rm_render_progressive"] == ("i32", ["ptr"] * 3 + ["i32"] + ["ptr"] * 4)
    text = open(RB.RUST).read()
    assert re.search(r"pub fn render_progressive\(\s*&mut self", text) and "rm_render_progressive(self.ctx" in text
    assert re.search(r"pub fn accumulate_lens\(\s*&mut self", text) and "rm_accumulate_lens_device(self.ctx" in text
    assert "rm_lens_sequence(first, count" in text
    hpp = open(os.path.join(entry.PKG_DIR, "host", "rusty_marcher.hpp")).read()
    assert re.search(r"render_progressive\(framebuffer::FrameBuffer", hpp) and "rm_render_progressive(ctx_" in hpp and "last_samples" in hpp


def test_cpp_mirror_compiles_with_the_progressive_render(entry, tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "rusty_marcher.hpp"\nusing namespace rusty_marcher;\n'
                   'std::string tick(renderer::Renderer &r, framebuffer::FrameBuffer &fb, const scene::Scene &sc) {'
                   ' r.render_progressive(fb, sc, 0.4, 5., 8u); return r.render_progressive(fb, sc, 0.4, 5., 8u, true); }\n'
                   'int main() { return RM_PROGRESSIVE_MAX_SAMPLES == 65536u ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(entry.ROOT, "include"),
                           "-I", os.path.join(entry.PKG_DIR, "host"), str(src)])


def test_build_info_announces_progressive(pkg):
    L = pkg.lib()
    assert " progressive" in L.rm_build_info().decode()
    assert L.rm_abi_version() == 5


def test_progressive_entry_points_refuse_null_context(pkg):
    L, B = pkg.lib(), pkg._lib
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 3)
    lens = B.rm_lens(LR.APERTURE, LR.FOCUS, 4, 0)
    frame, bytes8, total = np.full((64, 64, 3), 7.25), np.full((64, 64, 3), 7, np.uint8), C.c_uint32(77)
    assert L.rm_accumulate_lens_device(None, C.byref(p), C.byref(lens), None, 0, None, None, None, None) == B.RM_ERR_INVALID_ARG
    assert b"NULL ctx" in L.rm_last_error(None)
    assert L.rm_render_progressive(None, C.byref(p), C.byref(lens), 0, frame.ctypes.data_as(D), bytes8.ctypes.data_as(C.POINTER(C.c_uint8)),
                                   C.byref(total), None) == B.RM_ERR_INVALID_ARG
    assert b"NULL ctx" in L.rm_last_error(None)
    assert np.all(frame == 7.25) and np.all(bytes8 == 7) and total.value == 77       # nothing written


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
    nan, inf = float("nan"), float("inf")
    for aperture, focus, n in ((-0.1, 5., 4), (nan, 5., 4), (inf, 5., 4), (0.4, 0., 4), (0.4, -1., 4), (0.4, nan, 4), (0.4, inf, 4),
                               (0.4, 5., 0), (0.4, 5., 65), (0.4, 5., 2.5), (0.4, 5., True)):
        with pytest.raises(ValueError):
            pkg.create_renderer(workloads.FOV, 64., 64.).render_progressive(None, None, aperture, focus, n)
        with pytest.raises(ValueError):
            K.Context.render_progressive(ctx, p, aperture, focus, n)
    for host_rgb, host_rgb8 in ((np.zeros((32, 64, 3)), None), (np.zeros((64, 64, 3), np.float32), None), ([0.] * 12288, None),
                                (None, np.zeros((64, 64, 3))), (None, np.zeros((64, 32, 3), np.uint8)),
                                (np.zeros((64, 64, 6))[:, :, ::2], None)):
        with pytest.raises(ValueError):                               # too small; float32; a list; float64 bytes; too small; strided
            K.Context.render_progressive(ctx, p, 0.4, 5., 4, host_rgb=host_rgb, host_rgb8=host_rgb8)
    for first, count in ((-1, 4), (0, -1), (65536, 1), (65473, 64), (0, 65537), (1.5, 1), (0, True)):
        with pytest.raises(ValueError):
            K.Context.lens_sequence(ctx, first, count)
    # the device call: float64 sum (and mean) and uint8 bytes of the frame's shape on the context's device, contiguous
    t = torch.zeros((64, 64, 3), dtype=torch.float64)
    good = PR.lens_sequence(0, 4)
    for kw in (dict(sum=np.zeros((64, 64, 3))), dict(sum=t.float()), dict(sum=t), dict(sum=torch.zeros((64, 32, 3), dtype=torch.float64)),
               dict(sum=None)):
        with pytest.raises(ValueError):                               # numpy; float32; on the CPU; wrong shape; missing
            K.Context.accumulate_lens_device(ctx, p, kw["sum"], 0.4, 5., good, 0)


# ---------------------------------------------------------------- rm_lens_sequence
def library_sequence(pkg, first, count):
    t = np.full((count + 1, 4), -7.)
    assert pkg.lib().rm_lens_sequence(first, count, t.ctypes.data_as(D)) == 0
    assert np.all(t[count] == -7.)                                    # nothing behind the rows asked for
    return t[:count]


class _NoContext:
    """A Context without an rm_ctx: for the calls that need none."""
    device, ptr = 0, None

    def __init__(self, L):
        self.L = L


def test_lens_sequence_is_the_numpy_restatement_bit_for_bit(pkg):
    for first, count in ((0, 4096), (65472, 64), (1000, 7)):
        got, ref = library_sequence(pkg, first, count), PR.lens_sequence(first, count)
        assert got.tobytes() == ref.tobytes(), "first = %d: rows %s differ" % (first, first + np.flatnonzero((got != ref).any(axis=1)))
    assert pkg.backend.Context.lens_sequence(_NoContext(pkg.lib()), 1000, 7).tobytes() == PR.lens_sequence(1000, 7).tobytes()
    # a slice is the rows of the whole, wherever it begins
    assert library_sequence(pkg, 1000, 7).tobytes() == library_sequence(pkg, 0, 4096)[1000:1007].tobytes()
    h = np.sqrt(np.float64(.5))
    assert library_sequence(pkg, 0, 1).tolist() == [[0., 0., -h, -h]]
    # row 1: phi_2 = 1/2, phi_3 = 1/3, a = 2 * (1/5) - 1, b = 2 * (1/7) - 1
    a, b = 2. * (np.float64(1.) / 5.) - 1., 2. * (np.float64(1.) / 7.) - 1.
    assert library_sequence(pkg, 1, 1).tolist() == [[0.5, np.float64(1.) / 3., a * np.sqrt(1. - b * b / 2.), b * np.sqrt(1. - a * a / 2.)]]
    # the integers stay exact: every q is a power of its base just above 65535, far below 7^8 < 2^53
    assert max(PR.digit_reversed(65535, b)[1] for b in (2, 3, 5, 7)) <= 7 ** 8 < 2 ** 53


def test_every_row_of_the_sequence_is_a_valid_table_row(pkg):
    t = library_sequence(pkg, 0, 65536)
    assert LR.table_ok(t)
    assert (t[:, :2] >= 0.).all() and (t[:, :2] < 1.).all()
    assert (t[:, 2] ** 2 + t[:, 3] ** 2).max() <= 1.0000000000000002   # (within the table check's 1e-12)
    # ... in slices of a launch too: what rm_render_progressive stages is what rm_render_lens would accept
    for first in (0, 64, 65472):
        assert LR.table_ok(library_sequence(pkg, first, 64))


def test_prefixes_of_the_sequence_are_stratified():
    """On the integer pairs (r, q), not the rounded doubles: the first 36 rows put one point in each of the 4 x 9 cells of
    (dx, dy), the first 1,296 one in each of the 16 x 81."""
    for n, cx, cy in ((36, 4, 9), (1296, 16, 81)):
        cells = set()
        for s in range(n):
            (r2, q2), (r3, q3) = PR.digit_reversed(s, 2), PR.digit_reversed(s, 3)
            cells.add(((r2 * cx) // q2, (r3 * cy) // q3))
        assert len(cells) == n == cx * cy
    assert PR.digit_reversed(0, 2) == (0, 1) and PR.digit_reversed(6, 2) == (3, 8) and PR.digit_reversed(5, 3) == (7, 9)


def test_lens_sequence_refusals(pkg):
    L, B = pkg.lib(), pkg._lib
    t = np.full((65, 4), -7.)
    for first, count in ((65536, 1), (65473, 64), (0, 65537), (2 ** 32 - 1, 2), (2 ** 32 - 1, 2 ** 32 - 1)):
        assert L.rm_lens_sequence(first, count, t.ctypes.data_as(D)) == B.RM_ERR_INVALID_ARG
        assert b"first + count" in L.rm_last_error(None)
    assert L.rm_lens_sequence(0, 4, None) == B.RM_ERR_INVALID_ARG and b"NULL table" in L.rm_last_error(None)
    assert np.all(t == -7.)                                           # nothing written
    assert L.rm_lens_sequence(12, 0, None) == 0 and L.rm_lens_sequence(65536, 0, None) == 0
    assert L.rm_lens_sequence(65536, 0, t.ctypes.data_as(D)) == 0 and np.all(t == -7.)
    assert L.rm_lens_sequence(65535, 1, t.ctypes.data_as(D)) == 0 and np.all(t[1:] == -7.) and not (t[0] == -7.).any()


# ---------------------------------------------------------------- the yardstick does what the header states
def test_accumulate_and_to_bytes_on_hand_made_numbers():
    s = np.random.default_rng(5).uniform(size=(3, 6, 3))
    # one pass from nothing: the lens resolve, and a first sample of -0 stays -0 (the sum does not start from 0. +)
    total, mean = PR.accumulate(None, s, 0)
    assert mean.tobytes() == LR.resolve(s).tobytes()
    z = np.zeros((1, 1, 3))
    z[0, 0, 0] = -0.
    assert np.signbit(PR.accumulate(np.full((1, 3), np.nan), z, 0)[0][0, 0])
    # passes over slices are one left fold; the previous sum is not read under n_before == 0
    a, _ = PR.accumulate(np.full((3, 3), np.nan), s[:, :2], 0)
    b, mb = PR.accumulate(a, s[:, 2:], 2)
    assert b.tobytes() == total.tobytes() and mb.tobytes() == mean.tobytes()
    seq = s[1, 0]
    for t in range(1, 6):
        seq = seq + s[1, t]
    assert total[1].tobytes() == seq.tobytes() and mean[1].tobytes() == (seq / 6.).tobytes()
    # the mean divides by the whole count
    assert PR.accumulate(np.array([[3., 6., 9.]]), np.array([[[1., 2., 3.]]]), 3)[1].tolist() == [[1., 2., 3.]]
    # to_vec: clamped to [0, 1], scaled, truncated; fmax / fmin drop a NaN
    m = np.array([-0.5, 0., 0.5, 0.999, 1., 1.5, 2. / 255., float("nan"), float("inf")])
    assert PR.to_bytes(m).tolist() == [0, 0, 127, 254, 255, 255, 2, 0, 255]
    assert PR.to_bytes(m).dtype == np.uint8


def test_192_samples_are_another_picture_than_4(pkg, O, orc):
    """Non-vacuity of the yardstick alone: the frames the GPU tests compare are not all the same picture."""
    Y = PR.Yardstick(pkg, O, orc)
    table = PR.lens_sequence(0, 192)
    _, late = Y.progressive("demo", 32, 32, 3, LR.APERTURE, LR.FOCUS, table, (4,) + (47,) * 4)
    _, early = Y.progressive("demo", 32, 32, 3, LR.APERTURE, LR.FOCUS, table[:4], (4,))
    differ = (np.abs(late - early) > 0.05).any(axis=2)
    print("demo 32x32, aperture %g, focus %g: %d pixels differ by more than 0.05 between 4 and 192 samples"
          % (LR.APERTURE, LR.FOCUS, int(differ.sum())))
    assert int(differ.sum()) == PR.REFINED and PR.REFINED >= 50
    # ... and the first pass of the long run is the short run, byte for byte: a prefix is a prefix
    s = PR.samples(orc, Y.scene("demo")[1], Y.eye("demo"), None, 32, 32, 3, LR.APERTURE, LR.FOCUS, table[:4])
    assert PR.accumulate(None, s, 0)[1].reshape(32, 32, 3).tobytes() == early.tobytes()
    # the demo frame has channels above 1 (a highlight): the clamp of to_bytes has something to do in the GPU tests
    assert (late > 1.).any() and (PR.to_bytes(late) == 255).any()
