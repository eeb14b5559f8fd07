"""CPU-side checks of the swept hierarchies under a moving camera (include/rusty_marcher_amd.h, "swept hierarchies under a moving
camera"): no GPU.

1. The three entry points are exported, bound by ctypes and present in the header with shapes equal to the Rust shim's; each
   device call's argument list is its flat camera sibling's with the handle behind n_shapes; rm_build_info says " swept-camera"
   and the ABI is still 5; rm_swept_tick_report is 8 bytes.
2. A NULL context is refused by name with nothing written.
3. The Python wrappers refuse a sum that is no device tensor, wrong table shapes, a closed or foreign handle and a missing
   shape table without a handle before the library is called.
4. The C++ mirror compiles with the three calls in use."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import progressive_reference as PR
import test_rust_binding as RB
import workloads

DEVICE_CALLS = (("rm_accumulate_camera_swept_device", "rm_accumulate_camera_device", 9),
                ("rm_accumulate_converging_camera_swept_device", "rm_accumulate_converging_camera_device", 11))
FUNCTIONS = [c[0] for c in DEVICE_CALLS] + ["rm_swept_tick_info"]


# ---------------------------------------------------------------- 1. the ABI
def test_camera_swept_symbols_are_exported_and_bound(pkg, entry):
    L, B = pkg.lib(), pkg._lib
    header = open(os.path.join(entry.ROOT, "include", "rusty_marcher_amd.h")).read()
    c, r = RB.header_functions(), RB.rust_functions()
    for name in FUNCTIONS:
        assert hasattr(L, name) and name in B.SIGNATURES, name
        assert re.search(r"^rm_status +%s\(" % name, header, flags=re.M), name
        assert c[name] == r[name], "%s: header %s, gpu.rs %s" % (name, c[name], r[name])
        assert len(B.SIGNATURES[name][1]) == len(c[name][1]), name
    # the two device calls are their flat camera siblings with the handle behind n_shapes
    for swept, flat, at in DEVICE_CALLS:
        want = list(c[flat][1])
        assert want[at - 1] == "u32"                                    # (n_shapes)
        want.insert(at, "ptr")
        assert c[swept] == (c[flat][0], want)
        ctypes_flat = list(B.SIGNATURES[flat][1])
        ctypes_flat.insert(at, C.c_void_p)
        assert list(B.SIGNATURES[swept][1]) == ctypes_flat
    assert c["rm_swept_tick_info"] == ("i32", ["ptr", "ptr"])
    info = L.rm_build_info()
    assert b" swept-camera" in info and b" swept-hierarchy" in info and info.endswith(b" converge") and L.rm_abi_version() == 5
    assert "swept hierarchies under a moving camera" in header and "RM_SWEPT_BVH=0 returns all six" in header
    for name in ("accumulate_camera_swept_device", "accumulate_converging_camera_swept_device", "swept_tick_info"):
        assert callable(getattr(pkg.backend.Context, name))
    mirror = open(os.path.join(entry.PKG_DIR, "host", "rusty_marcher.hpp")).read()
    for name in FUNCTIONS:
        assert name + "(" in mirror, name


def test_the_tick_report_is_8_bytes_everywhere(pkg, entry):
    B = pkg._lib
    assert C.sizeof(B.rm_swept_tick_report) == 8
    assert [f[0] for f in B.rm_swept_tick_report._fields_] == ["walked_swept", "builds"]
    assert B.rm_swept_tick_report.builds.offset == 4
    hs, rs = RB.header_structs(), RB.rust_structs()
    assert hs["rm_swept_tick_report"] == rs["RmSweptTickReport"] and len(hs["rm_swept_tick_report"]) == 2
    header = open(os.path.join(entry.ROOT, "include", "rusty_marcher_amd.h")).read()
    assert re.search(r"\} rm_swept_tick_report; +/\* 8 bytes \*/", header)


# ---------------------------------------------------------------- 2. a NULL context
def test_the_entry_points_refuse_a_null_context_and_write_nothing(pkg):
    L, B = pkg.lib(), pkg._lib
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 3)
    lens, conv = B.rm_lens(0.4, 5., 4, 0), B.rm_converge(0.1, 16, 64)
    E = B.RM_ERR_INVALID_ARG
    out = np.full((64, 64, 3), 7.25)
    D = out.ctypes.data_as(C.c_void_p)
    assert L.rm_accumulate_camera_swept_device(None, C.byref(p), C.byref(lens), None, None, None, 2, None, 3, None, 0, D, D, None, None) == E
    assert b"rm_accumulate_camera_swept_device: NULL ctx" in L.rm_last_error(None)
    frame = B.rm_converge_frame(D, D, D, D, D, None, None)
    assert L.rm_accumulate_converging_camera_swept_device(None, C.byref(p), C.byref(lens), C.byref(conv), None, 64, None, None, 2, None, 3, None, 1,
                                                          C.byref(frame), None) == E
    assert b"rm_accumulate_converging_camera_swept_device: NULL ctx" in L.rm_last_error(None)
    rep = B.rm_swept_tick_report(77, 78)
    assert L.rm_swept_tick_info(None, C.byref(rep)) == E and (rep.walked_swept, rep.builds) == (77, 78)
    assert b"rm_swept_tick_info: NULL ctx" in L.rm_last_error(None)
    assert np.all(out == 7.25)


# ---------------------------------------------------------------- 3. the Python wrappers
class _NoLibrary:
    """A Context whose library must not be reached: the wrappers refuse before they call it."""
    device, ptr = 0, None

    class L:
        def __getattr__(self, name):
            raise AssertionError("the library was called: %s" % name)
    L = L()


def test_python_wrappers_check_before_the_library_sees_anything(pkg):
    import torch
    K = pkg.backend
    # (the two handle helpers are the Context's own: they call no library either)
    ctx = type("NoLibrary", (_NoLibrary,), {"_swept_for": K.Context._swept_for, "_camera_swept_for": K.Context._camera_swept_for})()
    p = K.make_params(workloads.FOV, 64., 64., 3)
    t = torch.zeros((64, 64, 3), dtype=torch.float64)
    table, lights, shapes, camera = PR.lens_sequence(0, 4), np.zeros((4, 2, 3)), np.zeros((4, 5, 3)), np.zeros((4, 12))
    for s in (np.zeros((64, 64, 3)), t.float(), t, None):               # (a sum that is no tensor of the context's device)
        with pytest.raises(ValueError):
            K.Context.accumulate_camera_swept_device(ctx, p, s, 0.4, 5., table, camera, lights, shapes, 0)
        with pytest.raises(ValueError):
            K.Context.accumulate_converging_camera_swept_device(ctx, p, s, t, t, 0.4, 5., 4, table, camera, lights, shapes, 0.1, 8, 16, True)
    # the tables' shapes: the checks both wrappers run in front of the handle and the call
    cpu = torch.device("cpu")
    for rows in (np.zeros((4, 11)), np.zeros((3, 12)), np.full((4, 12), float("nan")), np.zeros(48), torch.zeros((4, 12), dtype=torch.float32)):
        with pytest.raises(ValueError, match="camera_rows"):
            K._camera_rows_tensor(rows, 4, cpu)
    for bad in (np.zeros((4, 5)), np.zeros((3, 5, 3)), np.zeros((4, 5, 2)), torch.zeros((4, 5, 3), dtype=torch.float32)):
        with pytest.raises(ValueError, match="shape_offsets"):
            K._offset_tensor(bad, "shape_offsets", "n_shapes", 4, cpu)
    good = K._offset_tensor(shapes, "shape_offsets", "n_shapes", 4, cpu)
    assert good.shape == (4, 5, 3)
    # the handle: closed, another context's, no Swept at all; and no shape table to build one from
    closed = K.Swept(ctx, None)
    foreign = K.Swept(_NoLibrary(), C.c_void_p(1))
    for handle in (closed, foreign, 7, C.c_void_p(1)):
        with pytest.raises(ValueError, match="open Swept handle of this context"):
            K.Context._camera_swept_for(ctx, handle, good)
    with pytest.raises(ValueError, match="shape_offsets is None and no swept handle is given"):
        K.Context._camera_swept_for(ctx, None, None)
    own = K.Swept(ctx, C.c_void_p(1))
    assert K.Context._swept_for(ctx, own, good) is own
    own.ptr = None                                                      # (nothing to free: the handle was never the library's)


def test_bad_tables_and_handles_stop_both_wrappers_in_front_of_the_library(pkg, monkeypatch):
    """The same refusals driven through accumulate_camera_swept_device and accumulate_converging_camera_swept_device themselves.
    The one check that needs a GPU, that the output buffers live on the context's device, is stood in for (the wrappers' first
    step, _accumulate_args / _converging_args; the test above holds it); every later step is the wrappers' own, on host tensors.
    The library of the context raises when touched, so a wrapper that skipped a check, or ran it behind the call, fails here;
    and with everything in order both wrappers do reach the library, so no refusal below is owed to the stand-in."""
    import torch
    K = pkg.backend
    ctx = type("NoLibrary", (_NoLibrary,), {"_swept_for": K.Context._swept_for, "_camera_swept_for": K.Context._camera_swept_for})()
    p = K.make_params(workloads.FOV, 64., 64., 3)
    t = torch.zeros((64, 64, 3), dtype=torch.float64)
    lens_table = torch.from_numpy(PR.lens_sequence(0, 4))
    monkeypatch.setattr(K, "_accumulate_args", lambda device, params, sum, aperture, focus, table, *rest: (K._lens(aperture, focus, 4), lens_table))
    monkeypatch.setattr(K, "_converging_args", lambda c, params, sum, stats, count, aperture, focus, n, table, tol, lo, hi, *rest:
                        (K._lens(aperture, focus, n), K._converge(tol, lo, hi, n, 4), lens_table, None))
    table, lights, shapes, camera = PR.lens_sequence(0, 4), np.zeros((4, 2, 3)), np.zeros((4, 5, 3)), np.zeros((4, 12))
    handle = K.Swept(ctx, C.c_void_p(1))

    def plain(camera=camera, lights=lights, shapes=shapes, swept=handle):
        K.Context.accumulate_camera_swept_device(ctx, p, t, 0.4, 5., table, camera, lights, shapes, 0, swept=swept)

    def converging(camera=camera, lights=lights, shapes=shapes, swept=handle):
        K.Context.accumulate_converging_camera_swept_device(ctx, p, t, t, t, 0.4, 5., 4, table, camera, lights, shapes, 0.1, 4, 4, True, swept=swept)

    try:
        for call in (plain, converging):
            for rows in (np.zeros((4, 11)), np.zeros((3, 12)), np.full((4, 12), float("nan")), np.zeros(48), torch.zeros((4, 12), dtype=torch.float32)):
                with pytest.raises(ValueError, match="camera_rows"):
                    call(camera=rows)
            for bad in (np.zeros((4, 5)), np.zeros((3, 5, 3)), np.zeros((4, 5, 2)), torch.zeros((4, 5, 3), dtype=torch.float32),
                        np.full((4, 5, 3), float("inf"))):
                with pytest.raises(ValueError, match="shape_offsets"):
                    call(shapes=bad)
                with pytest.raises(ValueError, match="light_offsets"):
                    call(lights=bad)
            for swept in (K.Swept(ctx, None), K.Swept(_NoLibrary(), C.c_void_p(1)), 7):
                with pytest.raises(ValueError, match="open Swept handle of this context"):
                    call(swept=swept)
            with pytest.raises(ValueError, match="shape_offsets is None and no swept handle is given"):
                call(shapes=None, swept=None)
            with pytest.raises(AssertionError, match="the library was called: rm_accumulate_(converging_)?camera_swept_device"):
                call()                                                  # in order: now, and only now, the library is asked
            with pytest.raises(AssertionError, match="the library was called: rm_accumulate_(converging_)?camera_swept_device"):
                call(shapes=None)                                       # ... and a missing table under a handle is left to it to name
    finally:
        handle.ptr = None                                               # (nothing to free: the handle was never the library's)


# ---------------------------------------------------------------- 4. the C++ mirror
def test_the_mirror_compiles_with_the_camera_swept_calls(entry, tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "rusty_marcher.hpp"\n'
                   'static_assert(sizeof(rm_swept_tick_report) == 8, "rm_swept_tick_report is 8 bytes");\n'
                   'template <class G> uint32_t pass(G &g, const rm_params &p, const rm_lens &lens, const rm_converge &conv,\n'
                   '                                 const rm_converge_frame &bufs, const rm_swept *s, void *d) {\n'
                   '    g.accumulate_camera_swept_device(p, lens, d, d, d, 2u, d, 3u, s, 0u, d, d, d, nullptr);\n'
                   '    g.accumulate_converging_camera_swept_device(p, lens, conv, d, 64u, d, d, 2u, d, 3u, s, true, bufs, nullptr);\n'
                   '    const rm_swept_tick_report r = g.swept_tick_info();\n'
                   '    return r.walked_swept + r.builds;\n'
                   '}\n'
                   'int main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(entry.ROOT, "include"),
                           "-I", os.path.join(entry.PKG_DIR, "host"), str(src)])
    src.write_text('#include "rusty_marcher.hpp"\n'
                   'uint32_t use(rusty_marcher::renderer::Renderer &g, const rm_params &p, const rm_lens &lens, const rm_converge &conv, const rm_converge_frame &bufs,\n'
                   '             const rm_swept *s, void *d) {\n'
                   '    g.accumulate_camera_swept_device(p, lens, d, d, d, 2u, d, 3u, s, 0u, d, d, d, nullptr);\n'
                   '    g.accumulate_converging_camera_swept_device(p, lens, conv, d, 64u, d, d, 2u, d, 3u, s, true, bufs, nullptr);\n'
                   '    return g.swept_tick_info().builds;\n'
                   '}\n'
                   'int main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(entry.ROOT, "include"),
                           "-I", os.path.join(entry.PKG_DIR, "host"), str(src)])
