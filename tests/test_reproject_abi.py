"""CPU-side checks of the temporal reprojection (include/rusty_marcher_amd.h, "temporal reprojection"): no GPU.

1. The three entry points are exported, bound by ctypes and present in the header with shapes equal to the Rust shim's and in
   the C++ mirror; rm_view is 96 bytes, rm_reproject and rm_history_report 24 everywhere; rm_build_info says " reproject" and the
   ABI is still 5.
2. A NULL context is refused by name with nothing written.
3. The Python wrappers refuse every range of rm_reproject, and tensors that are not the context's, before the library is called.
   (The library's own refusals need a context, which needs a GPU: tests/test_gpu_reproject.py names every one of them.)
4. The C++ mirror compiles with the three calls in use."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import test_rust_binding as RB
import workloads

FUNCTIONS = ["rm_reproject_device", "rm_converge_history", "rm_converge_history_info"]


# ---------------------------------------------------------------- 1. the ABI
def test_reproject_symbols_are_exported_and_bound(pkg, entry):
    L, B = pkg.lib(), pkg._lib
    header = open(os.path.join(entry.ROOT, "include", "rusty_marcher_amd.h")).read()
    c, r = RB.header_functions(), RB.rust_functions()
    for name in FUNCTIONS:
        assert hasattr(L, name) and name in B.SIGNATURES, name
        assert re.search(r"^rm_status +%s\(" % name, header, flags=re.M), name
        assert c[name] == r[name], "%s: header %s, gpu.rs %s" % (name, c[name], r[name])
        assert len(B.SIGNATURES[name][1]) == len(c[name][1]), name
    assert c["rm_reproject_device"] == ("i32", ["ptr"] * 15)
    assert c["rm_converge_history"] == c["rm_converge_history_info"] == ("i32", ["ptr", "ptr"])
    info = L.rm_build_info().decode()
    assert " reproject" in info.split(" converge")[0] and info.endswith(" converge") and L.rm_abi_version() == 5
    assert "temporal reprojection" in header and "never a fault" in header.split("temporal reprojection")[1]
    assert "A REPROJECTED FRAME TRADES THAT PROMISE FOR HISTORY" in header
    for name in ("reproject_device", "converge_history", "history_info"):
        assert callable(getattr(pkg.backend.Context, name))
    assert callable(pkg.renderer.Renderer.keep_history) and callable(pkg.renderer.Renderer.drop_history)
    mirror = open(os.path.join(entry.PKG_DIR, "host", "rusty_marcher.hpp")).read()
    rust = open(RB.RUST).read()
    for name in FUNCTIONS:
        assert name + "(" in mirror, name
    assert "pub fn reproject_device(" in rust and "pub fn converge_history(" in rust and "pub fn history_info(" in rust


def test_the_structs_are_96_24_and_24_bytes_everywhere(pkg, entry, tmp_path):
    B = pkg._lib
    assert (C.sizeof(B.rm_view), C.sizeof(B.rm_reproject), C.sizeof(B.rm_history_report)) == (96, 24, 24)
    assert [f[0] for f in B.rm_view._fields_] == ["position", "basis"] and B.rm_view.basis.offset == 24
    assert [f[0] for f in B.rm_reproject._fields_] == ["sigma_z", "min_normal_dot", "max_history", "_pad"]
    assert B.rm_reproject.max_history.offset == 16
    names = ["reprojections", "last_reprojected", "carried", "without", "_pad"]
    assert [f[0] for f in B.rm_history_report._fields_] == names
    assert (B.rm_history_report.last_reprojected.offset, B.rm_history_report.carried.offset, B.rm_history_report.without.offset) == (8, 12, 16)
    hs, rs = RB.header_structs(), RB.rust_structs()
    assert hs["rm_view"] == rs["RmView"] and hs["rm_reproject"] == rs["RmReproject"] and hs["rm_history_report"] == rs["RmHistoryReport"]
    assert [n for n, _ in hs["rm_history_report"]] == names
    header = open(os.path.join(entry.ROOT, "include", "rusty_marcher_amd.h")).read()
    assert re.search(r"\} rm_view; +/\* 96 bytes", header) and re.search(r"\} rm_reproject; +/\* 24 bytes \*/", header)
    assert re.search(r"\} rm_history_report; +/\* 24 bytes \*/", header)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include "rusty_marcher_amd.h"\n'
                   '_Static_assert(sizeof(rm_view) == 96 && offsetof(rm_view, basis) == 24, "rm_view");\n'
                   '_Static_assert(sizeof(rm_reproject) == 24 && offsetof(rm_reproject, max_history) == 16, "rm_reproject");\n'
                   '_Static_assert(sizeof(rm_history_report) == 24 && offsetof(rm_history_report, without) == 16, "rm_history_report");\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(entry.ROOT, "include"), str(src)])
    # the starting values are the same in the three bindings
    rust = open(RB.RUST).read()
    assert "RmReproject { sigma_z: 0.1, min_normal_dot: 0.9, max_history: 32, _pad: 0 }" in rust
    mirror = open(os.path.join(entry.PKG_DIR, "host", "rusty_marcher.hpp")).read()
    assert "rm_reproject{.1, .9, 32u, 0u}" in mirror
    ctl = pkg.backend._reproject(.1, .9, 32)
    assert (ctl.sigma_z, ctl.min_normal_dot, ctl.max_history) == (.1, .9, 32)
    import inspect
    for f in (pkg.backend.Context.reproject_device, pkg.renderer.Renderer.keep_history):
        d = {k: v.default for k, v in inspect.signature(f).parameters.items()}
        assert (d["sigma_z"], d["min_normal_dot"], d["max_history"]) == (.1, .9, 32)


# ---------------------------------------------------------------- 2. a NULL context
def test_the_entry_points_refuse_a_null_context_and_write_nothing(pkg):
    L, B = pkg.lib(), pkg._lib
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 3)
    ctl = B.rm_reproject(.1, .9, 32, 0)
    view = B.rm_view(B.rm_vec3(0., 0., 0.), B.rm_camera_basis(B.rm_vec3(1., 0., 0.), B.rm_vec3(0., 1., 0.), B.rm_vec3(0., 0., -1.)))
    E = B.RM_ERR_INVALID_ARG
    out = np.full((64, 64, 9), 7.25)
    D = out.ctypes.data_as(C.c_void_p)
    assert L.rm_reproject_device(None, C.byref(p), C.byref(ctl), C.byref(view), D, D, D, D, D, D, D, D, D, D, None) == E
    assert b"rm_reproject_device: NULL ctx" in L.rm_last_error(None)
    assert np.all(out == 7.25)
    assert L.rm_converge_history(None, C.byref(ctl)) == E
    assert b"rm_converge_history: NULL ctx" in L.rm_last_error(None)
    rep = B.rm_history_report(5, 6, 7, 8, 9)
    assert L.rm_converge_history_info(None, C.byref(rep)) == E
    assert b"rm_converge_history_info: NULL ctx" in L.rm_last_error(None)
    assert (rep.reprojections, rep.last_reprojected, rep.carried, rep.without) == (5, 6, 7, 8)


# ---------------------------------------------------------------- 3. the Python wrappers
class _NoLibrary:
    """A Context whose library must not be reached: the wrappers refuse before they call it."""
    device, ptr = 0, None

    class L:
        def __getattr__(self, name):
            raise AssertionError("the library was called: %s" % name)
    L = L()


BAD_CONTROLS = [("sigma_z", 0.), ("sigma_z", -.1), ("sigma_z", float("nan")), ("sigma_z", float("inf")), ("min_normal_dot", 1.),
                ("min_normal_dot", -1.5), ("min_normal_dot", float("nan")), ("min_normal_dot", float("inf")), ("max_history", 0),
                ("max_history", 65537), ("max_history", -1), ("max_history", 2.5), ("max_history", True)]


@pytest.mark.parametrize("name,value", BAD_CONTROLS)
def test_the_wrappers_refuse_every_range_of_rm_reproject(pkg, name, value):
    K = pkg.backend
    good = dict(sigma_z=.1, min_normal_dot=.9, max_history=32)
    assert K._reproject(**good).max_history == 32
    ends = K._reproject(sigma_z=1e-300, min_normal_dot=-1., max_history=1)                  # the ranges' ends are in
    assert ends.min_normal_dot == -1. and ends.max_history == 1
    assert K._reproject(.1, .9, K.PROGRESSIVE_MAX_SAMPLES).max_history == 65536
    bad = dict(good, **{name: value})
    with pytest.raises(ValueError, match=name):
        K._reproject(**bad)
    with pytest.raises(ValueError, match=name):
        K.Context.converge_history(_NoLibrary(), bad)
    r = pkg.create_renderer(workloads.FOV, 64., 64.)
    with pytest.raises(ValueError, match=name):
        r.keep_history(**bad)


def test_reproject_device_checks_its_tensors_before_the_library_sees_anything(pkg):
    import torch
    K = pkg.backend
    ctx = _NoLibrary()
    p = K.make_params(workloads.FOV, 64., 64., 3)
    t = torch.zeros((64, 64, 3), dtype=torch.float64)
    view = (K._lib.rm_vec3(0., 0., 0.), ((1., 0., 0.), (0., 1., 0.), (0., 0., -1.)))
    for s in (np.zeros((64, 64, 3)), t.float(), t, None):               # (nothing here is a tensor of the context's device)
        with pytest.raises(ValueError, match="prev_total must"):
            K.Context.reproject_device(ctx, p, s, t, t, t, t, view, t, t, t)
    v = K._view(view)
    assert isinstance(v, K._lib.rm_view) and v.basis.forward.z == -1. and K._view(v) is v


# ---------------------------------------------------------------- 4. the C++ mirror
def test_the_mirror_compiles_with_the_reproject_calls(entry, tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "rusty_marcher.hpp"\n'
                   'static_assert(sizeof(rm_view) == 96 && sizeof(rm_reproject) == 24 && sizeof(rm_history_report) == 24, "sizes");\n'
                   'uint64_t use(rusty_marcher::renderer::Renderer &g, const rm_params &p, void *d, const void *s) {\n'
                   '    const rm_reproject ctl{.1, .9, 8u, 0u};\n'
                   '    const rm_view view{{0., 0., 0.}, {{1., 0., 0.}, {0., 1., 0.}, {0., 0., -1.}}};\n'
                   '    g.reproject_device(p, ctl, view, s, s, s, s, s, d, d, d, nullptr, nullptr, nullptr);\n'
                   '    g.converge_history(&ctl);\n'
                   '    g.keep_history();\n'
                   '    g.drop_history();\n'
                   '    return g.history_info().reprojections;\n'
                   '}\n'
                   'int main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(entry.ROOT, "include"),
                           "-I", os.path.join(entry.PKG_DIR, "host"), str(src)])
