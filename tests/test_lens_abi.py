"""CPU-side checks of the thin-lens camera (include/rusty_marcher_amd.h, "thin-lens camera").

1. The three entry points are exported and bound by ctypes, the Rust shim and the C++ mirror with the header's shapes, rm_lens
   is 24 bytes everywhere, rm_build_info says " lens", a NULL context is refused, and the Python wrappers raise before the
   library is called.
2. rm_lens_table is tests/lens_reference.py's numpy restatement bit for bit for every n in 1..64, every row of every table
   satisfies the table conditions, and its refusals are returned.
3. tests/lens_reference.py -- the yardstick of the GPU tests -- is pinned on orc_render (aperture 0, one sample) and is not
   vacuous: at the settings the GPU tests use, the lens frame differs from the aperture-0 frame in the committed number of pixels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lens_reference as LR
import radiance_reference as RR
import test_rust_binding as RB
import workloads

FUNCTIONS = ["rm_lens_table", "rm_render_lens_device", "rm_render_lens"]


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_lens_abi"))


# ---------------------------------------------------------------- the ABI
def test_lens_symbols_are_exported_and_bound(pkg):
    L = pkg.lib()
    for name in FUNCTIONS:
        assert hasattr(L, name), "library does not export %s" % name
        assert name in pkg._lib.SIGNATURES
    for name in ("lens_table", "render_lens_device", "render_lens"):
        assert callable(getattr(pkg.backend.Context, name))
    assert callable(pkg.Renderer.render_depth_of_field)


def test_rm_lens_is_24_bytes_in_c_ctypes_and_rust(pkg, entry, tmp_path):
    src = tmp_path / "lens.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rusty_marcher_amd.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(rm_lens), offsetof(rm_lens, aperture), offsetof(rm_lens, focus),'
                   ' offsetof(rm_lens, n_samples), offsetof(rm_lens, _pad));'
                   'return 0;}\n')
    exe = tmp_path / "lens"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(entry.ROOT, "include"),
                           str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == [24, 0, 8, 16, 20]
    S = pkg._lib.rm_lens
    assert C.sizeof(S) == 24 and (S.aperture.offset, S.focus.offset, S.n_samples.offset, S._pad.offset) == (0, 8, 16, 20)
    c, r = RB.header_structs(), RB.rust_structs()
    assert c["rm_lens"] == r["RmLens"] == [("aperture", "f64"), ("focus", "f64"), ("n_samples", "u32"), ("_pad", "u32")]


def test_lens_functions_have_the_header_shapes_in_the_rust_shim_and_the_cpp_mirror(entry):
    c, r = RB.header_functions(), RB.rust_functions()
    for name in FUNCTIONS:
        assert name in c and name in r, name
        assert c[name] == r[name], "%s: header %s, gpu.rs %s" % (name, c[name], r[name])
    assert c["rm_lens_table"] == ("i32", ["u32", "ptr"])
    assert c["rm_render_lens_device"] == ("i32", ["ptr"] * 6)
    assert c["rm_render_lens"] == ("i32", ["ptr"] * 6)
    text = open(RB.RUST).read()
    assert re.search(r"pub fn render_lens\(\s*&mut self", text) and "rm_render_lens(self.ctx" in text and "rm_lens_table(" in text
    hpp = open(os.path.join(entry.PKG_DIR, "host", "rusty_marcher.hpp")).read()
    assert re.search(r"render_lens\(framebuffer::FrameBuffer", hpp) and "rm_render_lens(" in hpp and "rm_lens_table(" in hpp


def test_cpp_mirror_compiles_with_the_lens_render(entry, tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "rusty_marcher.hpp"\nusing namespace rusty_marcher;\n'
                   'std::string frame(renderer::Renderer &r, framebuffer::FrameBuffer &fb, const scene::Scene &sc) {'
                   ' return r.render_lens(fb, sc, 0.4, 5., 16u); }\n'
                   'int main() { return sizeof(rm_lens) == 24 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(entry.ROOT, "include"),
                           "-I", os.path.join(entry.PKG_DIR, "host"), str(src)])


def test_build_info_announces_lens(pkg):
    L = pkg.lib()
    assert " lens" in L.rm_build_info().decode()
    assert L.rm_abi_version() == 5


def test_lens_entry_points_refuse_null_context(pkg):
    L, B = pkg.lib(), pkg._lib
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 3)
    lens = B.rm_lens(LR.APERTURE, LR.FOCUS, 4, 0)
    table = LR.lens_table(4)
    frame = np.full((64, 64, 3), 7.25)
    D = C.POINTER(C.c_double)
    assert L.rm_render_lens_device(None, C.byref(p), C.byref(lens), None, None, None) == B.RM_ERR_INVALID_ARG
    assert b"NULL ctx" in L.rm_last_error(None)
    assert L.rm_render_lens(None, C.byref(p), C.byref(lens), table.ctypes.data_as(D), frame.ctypes.data_as(D), None) == B.RM_ERR_INVALID_ARG
    assert b"NULL ctx" in L.rm_last_error(None)
    assert np.all(frame == 7.25)                                      # nothing written


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
    good = LR.lens_table(4)
    nan, inf = float("nan"), float("inf")
    for aperture, focus, n in ((-0.1, 5., 4), (nan, 5., 4), (inf, 5., 4), (0.4, 0., 4), (0.4, -1., 4), (0.4, nan, 4), (0.4, inf, 4),
                               (0.4, 5., 0), (0.4, 5., 65), (0.4, 5., 2.5), (0.4, 5., True)):
        with pytest.raises(ValueError):
            pkg.create_renderer(workloads.FOV, 64., 64.).render_depth_of_field(None, None, aperture, focus, n)
        with pytest.raises(ValueError):
            K._lens(aperture, focus, n)
    for n in (0, 65, 2.5, True):
        with pytest.raises(ValueError):
            K.Context.lens_table(ctx, n)
    for aperture, focus in ((-0.1, 5.), (0.4, 0.), (nan, 5.), (0.4, inf)):
        with pytest.raises(ValueError):
            K.Context.render_lens(ctx, p, host, aperture, focus, good)
    bad = []
    for col, value in ((0, 1.), (0, -1e-9), (1, 1.), (1, nan), (2, 1.5), (3, inf)):
        b = good.copy()
        b[1, col] = value
        assert not LR.table_ok(b)
        bad.append(b)
    bad += [good[:, :3], good.ravel(), np.zeros((0, 4)), np.zeros((65, 4))]
    for b in bad:
        with pytest.raises(ValueError):
            K.Context.render_lens(ctx, p, host, 0.4, 5., b)
    with pytest.raises(ValueError):
        K.Context.render_lens(ctx, p, np.zeros((32, 64, 3)), 0.4, 5., good)                  # a frame too small for the rows
    # the device frame: a float64 torch tensor of the frame's shape on the context's device, contiguous
    for frame in (host, t.float(), t, torch.zeros((64, 32, 3), dtype=torch.float64)):
        with pytest.raises(ValueError):                               # numpy; float32; on the CPU; wrong shape
            K.Context.render_lens_device(ctx, p, frame, 0.4, 5., good)
    lens = K._lens(0, 5, 64.)
    assert (lens.aperture, lens.focus, lens.n_samples) == (0., 5., 64)


# ---------------------------------------------------------------- rm_lens_table
def library_table(pkg, n):
    t = np.full((n, 4), -7.)
    assert pkg.lib().rm_lens_table(n, t.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return t


def test_lens_table_is_the_numpy_restatement_bit_for_bit(pkg):
    K = pkg.backend
    for n in range(1, 65):
        got, ref = library_table(pkg, n), LR.lens_table(n)
        assert got.tobytes() == ref.tobytes(), "n = %d: rows %s differ" % (n, np.flatnonzero((got != ref).any(axis=1)))
        assert LR.table_ok(got), n
        assert (got[:, 2] ** 2 + got[:, 3] ** 2 <= 1.).all(), n         # ... with nothing owed to the check's 1e-12
        assert K.Context.lens_table(_NoContext(pkg.lib()), n).tobytes() == ref.tobytes()
    assert library_table(pkg, 1).tolist() == [[0., 0., 0., 0.]]
    # m = ceil(sqrt(n)): 5 samples lie in a 3 x 3 grid, i inner; the lens cell is the pixel cell turned by a quarter
    t5 = library_table(pkg, 5)
    assert t5[:, 0].tolist() == [0., 1. / 3., 2. / 3., 0., 1. / 3.] and t5[:, 1].tolist() == [0., 0., 0., 1. / 3., 1. / 3.]
    t4 = library_table(pkg, 4)
    a, b = np.float64(1.) / 2. - 1., np.float64(3.) / 2. - 1.          # row 0: i = j = 0 -> a = 1/2 - 1, b = (2 (2 - 1 - 0) + 1) / 2 - 1
    assert (t4[0, 2], t4[0, 3]) == (a * np.sqrt(1. - b * b / 2.), b * np.sqrt(1. - a * a / 2.))
    # no two rows of a full grid share a lens point or an offset
    t16 = library_table(pkg, 16)
    assert len({tuple(r) for r in t16[:, :2].tolist()}) == 16 and len({tuple(r) for r in t16[:, 2:].tolist()}) == 16


class _NoContext:
    """A Context without an rm_ctx: for the calls that need none."""
    device, ptr = 0, None

    def __init__(self, L):
        self.L = L


def test_lens_table_refusals(pkg):
    L, B = pkg.lib(), pkg._lib
    t = np.full((65, 4), -7.)
    D = C.POINTER(C.c_double)
    for n in (0, 65, 2 ** 32 - 1):
        assert L.rm_lens_table(n, t.ctypes.data_as(D)) == B.RM_ERR_INVALID_ARG
        assert b"n_samples" in L.rm_last_error(None)
    assert L.rm_lens_table(4, None) == B.RM_ERR_INVALID_ARG and b"NULL table" in L.rm_last_error(None)
    assert np.all(t == -7.)                                           # nothing written
    assert L.rm_lens_table(64, t.ctypes.data_as(D)) == 0 and np.all(t[64] == -7.) and not (t[:64] == -7.).any()


# ---------------------------------------------------------------- the yardstick does what the header states
def test_lens_rays_on_hand_made_numbers():
    class R:
        width, height, half_fov, ratio = 4., 2., 0.5, 2.
    table = np.array([[0., 0., 0., 0.], [0.5, 0.25, 1., 0.], [0., 0., 0., -1.]])
    eye = (1., 2., 3.)
    o, d = LR.lens_rays(4, 2, R, eye, None, 0.5, 10., table)
    o, d = o.reshape(2, 4, 3, 3), d.reshape(2, 4, 3, 3)
    # row 0 of the table: the centre of the lens, the direction is D * focus
    assert o[1, 3, 0].tolist() == [1., 2., 3.]
    D = RR.sample_directions(np.array([[3., 1.]]), R)[0]
    assert d[1, 3, 0].tolist() == [(1. + D[0] * 10.) - 1., (2. + D[1] * 10.) - 2., (3. + D[2] * 10.) - 3.]
    # row 1: half a unit to the right of the camera; the focus point is that of the sample (3.5, 1.25)
    assert o[1, 3, 1].tolist() == [1.5, 2., 3.]
    D = RR.sample_directions(np.array([[3.5, 1.25]]), R)[0]
    assert D[2] == -1. and d[1, 3, 1].tolist() == [(1. + D[0] * 10.) - 1.5, (2. + D[1] * 10.) - 2., -10.]
    # row 2: half a unit below
    assert o[0, 0, 2].tolist() == [1., 1.5, 3.]
    # aperture 0: the sample rays themselves
    o0, d0 = LR.lens_rays(4, 2, R, eye, None, 0., 10., table)
    assert np.all(o0 == np.array(eye)) and d0.reshape(2, 4, 3, 3)[1, 3, 1].tolist() == D.tolist()
    # an oriented basis: the lens point moves along its right and up, the focus point along its D
    basis = ((0., 0., -1.), (0., 1., 0.), (-1., 0., 0.))
    ob, db = LR.lens_rays(4, 2, R, eye, basis, 0.5, 10., table)
    assert ob.reshape(2, 4, 3, 3)[0, 0, 1].tolist() == [1., 2., 2.5] and ob.reshape(2, 4, 3, 3)[0, 0, 2].tolist() == [1., 1.5, 3.]
    Db = RR.sample_directions(np.array([[0., 0.]]), R, basis)[0]
    assert Db[0] == -1. and db.reshape(2, 4, 3, 3)[0, 0, 0, 0] == (1. + -10.) - 1.
    # the resolve: table order, one division
    s = np.random.default_rng(3).uniform(size=(2, 5, 3))
    seq = s[1, 0]
    for t in range(1, 5):
        seq = seq + s[1, t]
    assert LR.resolve(s)[1].tobytes() == (seq / 5.).tobytes()


def test_supersample_and_random_tables():
    t = LR.supersample_table(3)
    assert t[:, 0].tolist() == [0., 1. / 3., 2. / 3.] * 3 and t[:, 1].tolist() == [0.] * 3 + [1. / 3.] * 3 + [2. / 3.] * 3
    assert not t[:, 2:].any() and LR.table_ok(t)
    r = LR.random_table(np.random.default_rng(11), 7)
    assert r.shape == (7, 4) and LR.table_ok(r) and r[0, 2:].tolist() == [1., 0.]


# ---------------------------------------------------------------- ... and is pinned on the oracle
def test_aperture_0_with_one_sample_is_orc_render_bit_for_bit(pkg, O, orc):
    Y = LR.Yardstick(pkg, O, orc)
    f = Y.frame("demo", 64, 64, 3, 0., LR.FOCUS, LR.lens_table(1))
    assert f.tobytes() == O.render(Y.scene("demo")[1], 64, 64, fov=workloads.FOV, max_depth=3).tobytes()
    # ... and under the fixed view given as a basis
    g = Y.frame("demo", 64, 64, 3, 0., LR.FOCUS, LR.lens_table(1), (Y.eye("demo"), RR.FIXED_VIEW))
    assert g.tobytes() == f.tobytes()


def test_the_lens_blurs_what_is_out_of_focus(pkg, O, orc):
    """Non-vacuity: at the GPU tests' settings the lens frame is another picture than the aperture-0 frame of the same table."""
    Y = LR.Yardstick(pkg, O, orc)
    table = LR.lens_table(16)
    lens = Y.frame("demo", 64, 64, 3, LR.APERTURE, LR.FOCUS, table)
    sharp = Y.frame("demo", 64, 64, 3, 0., LR.FOCUS, table)
    differ = (np.abs(lens - sharp) > 0.05).any(axis=2)
    print("demo 64x64, 16 samples, aperture %g, focus %g: %d pixels differ by more than 0.05 from the aperture-0 frame"
          % (LR.APERTURE, LR.FOCUS, int(differ.sum())))
    assert int(differ.sum()) == LR.BLURRED and LR.BLURRED >= 100
    assert Y.eye("demo") == (0., 0., 0.)                             # the plane in focus, z = -5, passes through the glass sphere's centre
