"""CPU-side checks of the variance-guided filter (include/rusty_marcher_amd.h, "variance-guided filter"): no GPU.

1. The three entry points are exported, bound by ctypes and present in the header with shapes equal to the Rust shim's and in
   the C++ mirror; rm_denoise is 40 bytes everywhere; rm_build_info says " denoise" and the ABI is still 5.
2. rm_denoise_workspace is a function of params alone and refuses what it must; a NULL context is refused by name with nothing
   written.
3. The Python wrappers refuse every range of rm_denoise, and tensors that are not the context's, before the library is called.
   (The library's own refusals need a context, which needs a GPU: tests/test_gpu_denoise.py names every one of them.)
4. The C++ mirror compiles with the three calls in use."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import test_rust_binding as RB
import workloads

FUNCTIONS = ["rm_denoise_workspace", "rm_denoise_device", "rm_render_denoised"]


# ---------------------------------------------------------------- 1. the ABI
def test_denoise_symbols_are_exported_and_bound(pkg, entry):
    L, B = pkg.lib(), pkg._lib
    header = open(os.path.join(entry.ROOT, "include", "rusty_marcher_amd.h")).read()
    c, r = RB.header_functions(), RB.rust_functions()
    for name in FUNCTIONS:
        assert hasattr(L, name) and name in B.SIGNATURES, name
        assert re.search(r"^rm_status +%s\(" % name, header, flags=re.M), name
        assert c[name] == r[name], "%s: header %s, gpu.rs %s" % (name, c[name], r[name])
        assert len(B.SIGNATURES[name][1]) == len(c[name][1]), name
    assert c["rm_denoise_workspace"] == c["rm_converge_workspace"] == ("i32", ["ptr", "ptr"])
    assert c["rm_denoise_device"] == ("i32", ["ptr"] * 12)
    assert c["rm_render_denoised"] == ("i32", ["ptr", "ptr", "ptr", "i32", "ptr", "ptr", "ptr"])
    assert B.SIGNATURES["rm_render_denoised"][1][3] is C.c_int
    info = L.rm_build_info().decode()
    assert " denoise" in info.split(" converge")[0] and info.endswith(" converge") and L.rm_abi_version() == 5
    assert "variance-guided filter" in header and "THE GUIDE IS THE PINHOLE VIEW" in header
    for name in ("denoise_workspace", "denoise_device", "render_denoised"):
        assert callable(getattr(pkg.backend.Context, name))
    assert callable(pkg.renderer.Renderer.render_denoised)
    mirror = open(os.path.join(entry.PKG_DIR, "host", "rusty_marcher.hpp")).read()
    rust = open(RB.RUST).read()
    for name in FUNCTIONS:
        assert name + "(" in mirror, name
    assert "pub fn denoise_device(" in rust and "pub fn render_denoised(" in rust


def test_rm_denoise_is_40_bytes_everywhere(pkg, entry, tmp_path):
    B = pkg._lib
    assert C.sizeof(B.rm_denoise) == 40
    names = ["sigma_l", "sigma_z", "epsilon", "fallback_variance", "iterations", "normal_squarings"]
    assert [f[0] for f in B.rm_denoise._fields_] == names
    assert (B.rm_denoise.iterations.offset, B.rm_denoise.normal_squarings.offset) == (32, 36)
    hs, rs = RB.header_structs(), RB.rust_structs()
    assert hs["rm_denoise"] == rs["RmDenoise"] and [n for n, _ in hs["rm_denoise"]] == names
    header = open(os.path.join(entry.ROOT, "include", "rusty_marcher_amd.h")).read()
    assert re.search(r"\} rm_denoise; +/\* 40 bytes \*/", header)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include "rusty_marcher_amd.h"\n'
                   '_Static_assert(sizeof(rm_denoise) == 40 && offsetof(rm_denoise, iterations) == 32 && offsetof(rm_denoise, normal_squarings) == 36, "rm_denoise");\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(entry.ROOT, "include"), str(src)])
    # the starting values are the same in the three bindings
    rust = open(RB.RUST).read()
    assert "RmDenoise { sigma_l: 4., sigma_z: 0.1, epsilon: 1e-10, fallback_variance: 1., iterations: 5, normal_squarings: 5 }" in rust
    mirror = open(os.path.join(entry.PKG_DIR, "host", "rusty_marcher.hpp")).read()
    assert "rm_denoise{4., .1, 1e-10, 1., 5u, 5u}" in mirror
    ctl = pkg.backend._denoise(4., .1, 1e-10, 1., 5, 5)
    assert (ctl.sigma_l, ctl.sigma_z, ctl.epsilon, ctl.fallback_variance, ctl.iterations, ctl.normal_squarings) == (4., .1, 1e-10, 1., 5, 5)


# ---------------------------------------------------------------- 2. the workspace; a NULL context
def test_the_workspace_is_a_function_of_params_alone(pkg):
    L, B = pkg.lib(), pkg._lib
    for h, w in ((32, 32), (96, 96), (40, 64), (1056, 1920), (31, 64)):
        p = pkg.backend.make_params(workloads.FOV, float(h), float(w), 3)
        b = C.c_size_t(77)
        assert L.rm_denoise_workspace(C.byref(p), C.byref(b)) == B.RM_OK
        pixels = (h - h % 32) * w
        # two planes of 4 doubles, the guide's 8 words, rounded up to 256 B, and 256 B so that it is never empty
        assert b.value == (pixels * 16 * 8 + 255) // 256 * 256 + 256 and b.value % 256 == 0
        p.max_depth, p.flags = 9, 1                                     # (nothing else of params is looked at)
        b2 = C.c_size_t(0)
        assert L.rm_denoise_workspace(C.byref(p), C.byref(b2)) == B.RM_OK and b2.value == b.value
    p = pkg.backend.make_params(workloads.FOV, 64., 48., 3)
    b = C.c_size_t(77)
    assert L.rm_denoise_workspace(C.byref(p), C.byref(b)) == B.RM_ERR_DIMENSIONS and b.value == 77
    assert b"rm_denoise_workspace: frame width is not a multiple of 32" in L.rm_last_error(None)
    assert L.rm_denoise_workspace(None, C.byref(b)) == B.RM_ERR_INVALID_ARG and b.value == 77
    assert L.rm_denoise_workspace(C.byref(p), None) == B.RM_ERR_INVALID_ARG
    assert b"rm_denoise_workspace: NULL argument" in L.rm_last_error(None)


def test_the_entry_points_refuse_a_null_context_and_write_nothing(pkg):
    L, B = pkg.lib(), pkg._lib
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 3)
    ctl = B.rm_denoise(4., .1, 1e-10, 1., 5, 5)
    E = B.RM_ERR_INVALID_ARG
    out = np.full((64, 64, 3), 7.25)
    D = out.ctypes.data_as(C.c_void_p)
    assert L.rm_denoise_device(None, C.byref(p), C.byref(ctl), D, D, D, None, D, D, D, D, None) == E
    assert b"rm_denoise_device: NULL ctx" in L.rm_last_error(None)
    timing = B.rm_timing()
    timing.kernel_ms = 5.5
    bytes8 = np.full((64, 64, 3), 9, np.uint8)
    assert L.rm_render_denoised(None, C.byref(p), C.byref(ctl), 1, out.ctypes.data_as(C.POINTER(C.c_double)),
                                bytes8.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(timing)) == E
    assert b"rm_render_denoised: NULL ctx" in L.rm_last_error(None)
    assert np.all(out == 7.25) and np.all(bytes8 == 9) and timing.kernel_ms == 5.5


# ---------------------------------------------------------------- 3. the Python wrappers
class _NoLibrary:
    """A Context whose library must not be reached: the wrappers refuse before they call it."""
    device, ptr = 0, None

    class L:
        def __getattr__(self, name):
            raise AssertionError("the library was called: %s" % name)
    L = L()


BAD_CONTROLS = [("sigma_l", -1.), ("sigma_l", float("nan")), ("sigma_l", float("inf")), ("sigma_z", 0.), ("sigma_z", -.1),
                ("sigma_z", float("nan")), ("epsilon", 0.), ("epsilon", float("inf")), ("epsilon", float("nan")),
                ("fallback_variance", -1e-300), ("fallback_variance", float("nan")), ("iterations", 6), ("iterations", -1),
                ("iterations", 2.5), ("iterations", True), ("normal_squarings", 9), ("normal_squarings", -1)]


@pytest.mark.parametrize("name,value", BAD_CONTROLS)
def test_the_wrappers_refuse_every_range_of_rm_denoise(pkg, name, value):
    K = pkg.backend
    good = dict(sigma_l=4., sigma_z=.1, epsilon=1e-10, fallback_variance=1., iterations=5, normal_squarings=5)
    assert K._denoise(**good).iterations == 5
    assert K._denoise(**dict(good, sigma_l=0., fallback_variance=0., iterations=0, normal_squarings=0)).sigma_l == 0.   # the ranges' ends are in
    assert K._denoise(**dict(good, normal_squarings=8)).normal_squarings == 8
    bad = dict(good, **{name: value})
    with pytest.raises(ValueError, match=name):
        K._denoise(**bad)
    p = K.make_params(workloads.FOV, 64., 64., 3)
    with pytest.raises(ValueError, match=name):
        K.Context.render_denoised(_NoLibrary(), p, **bad)
    r = pkg.create_renderer(workloads.FOV, 64., 64.)
    with pytest.raises(ValueError, match=name):
        r.render_denoised(pkg.create_frame_buffer(64, 64), None, **{k: v for k, v in bad.items()})


def test_denoise_device_checks_its_tensors_before_the_library_sees_anything(pkg):
    import torch
    K = pkg.backend
    ctx = _NoLibrary()
    p = K.make_params(workloads.FOV, 64., 64., 3)
    t = torch.zeros((64, 64, 3), dtype=torch.float64)
    for s in (np.zeros((64, 64, 3)), t.float(), t, None):               # (nothing here is a tensor of the context's device)
        with pytest.raises(ValueError, match="sum must"):
            K.Context.denoise_device(ctx, p, s, t, t, t)


# ---------------------------------------------------------------- 4. the C++ mirror
def test_the_mirror_compiles_with_the_denoise_calls(entry, tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "rusty_marcher.hpp"\n'
                   'static_assert(sizeof(rm_denoise) == 40, "rm_denoise is 40 bytes");\n'
                   'std::string use(rusty_marcher::renderer::Renderer &g, rusty_marcher::framebuffer::FrameBuffer &frame,\n'
                   '                const rusty_marcher::scene::Scene &sc, const rm_params &p, void *d) {\n'
                   '    const rm_denoise ctl{4., .1, 1e-10, 1., 3u, 5u};\n'
                   '    if (g.denoise_workspace(p) == 0u) return "";\n'
                   '    g.denoise_device(p, ctl, d, d, d, nullptr, d, d, nullptr, nullptr, nullptr);\n'
                   '    g.render_denoised(frame, sc, ctl, false);\n'
                   '    return g.render_denoised(frame, sc);\n'
                   '}\n'
                   'int main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(entry.ROOT, "include"),
                           "-I", os.path.join(entry.PKG_DIR, "host"), str(src)])
