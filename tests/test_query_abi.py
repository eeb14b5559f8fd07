"""CPU-side checks of the ray-query entry points (include/rusty_marcher_amd.h, "ray queries"): exported, bound by
ctypes / the C++ mirror / the Rust shim with the header's shapes, rm_hit laid out as declared, announced by
rm_build_info, and loud without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import test_rust_binding as RB

QUERY_FUNCTIONS = ["rm_intersect_rays", "rm_occluded_rays", "rm_intersect_rays_device", "rm_occluded_rays_device",
                   "rm_pick", "rm_primary_hits_device"]


def test_query_symbols_are_exported_and_bound(pkg):
    L = pkg.lib()
    for name in QUERY_FUNCTIONS:
        assert hasattr(L, name), "library does not export %s" % name
        assert name in pkg._lib.SIGNATURES


def test_rm_hit_is_72_bytes_in_c_and_in_the_mirrors(pkg, entry, tmp_path):
    src = tmp_path / "hit.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rusty_marcher_amd.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(rm_hit), offsetof(rm_hit, point), offsetof(rm_hit, normal),'
                   ' offsetof(rm_hit, shape), offsetof(rm_hit, element), offsetof(rm_hit, hit), offsetof(rm_hit, _pad));'
                   'return 0;}\n')
    exe = tmp_path / "hit"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(entry.ROOT, "include"),
                           str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [72, 8, 32, 56, 60, 64, 68]
    H = pkg._lib.rm_hit
    assert C.sizeof(H) == 72
    assert [getattr(H, f).offset for f in ("point", "normal", "shape", "element", "hit", "_pad")] == sizes[1:]
    dt = pkg.backend.HIT_DTYPE
    assert dt.itemsize == 72
    assert [dt.fields[f][1] for f in ("point", "normal", "shape", "element", "hit", "_pad")] == sizes[1:]


def test_rust_rm_hit_has_the_header_fields_in_order():
    c, r = RB.header_structs(), RB.rust_structs()
    assert "rm_hit" in c and "RmHit" in r
    assert c["rm_hit"] == r["RmHit"]
    assert [n for n, _ in c["rm_hit"]] == ["t", "point", "normal", "shape", "element", "hit", "_pad"]


def test_query_functions_have_the_header_shapes_in_the_rust_shim():
    c, r = RB.header_functions(), RB.rust_functions()
    for name in QUERY_FUNCTIONS:
        assert name in c and name in r, name
        assert c[name] == r[name], "%s: header %s, gpu.rs %s" % (name, c[name], r[name])
    assert c["rm_pick"] == ("i32", ["ptr", "ptr", "u32", "u32", "ptr"])
    text = open(RB.RUST).read()
    assert re.search(r"pub fn pick\(\s*&mut self", text) and "Option<RmHit>" in text


def test_cpp_mirror_has_a_pick_helper(entry):
    text = open(os.path.join(entry.PKG_DIR, "host", "rusty_marcher.hpp")).read()
    assert re.search(r"rm_hit pick\(", text) and "rm_pick(" in text


def test_build_info_announces_the_queries(pkg):
    L = pkg.lib()
    assert " queries" in L.rm_build_info().decode()
    assert L.rm_abi_version() == 5


def test_query_entry_points_refuse_null_context(pkg):
    L, B = pkg.lib(), pkg._lib
    E = B.RM_ERR_INVALID_ARG
    v = (B.rm_vec3 * 1)(B.rm_vec3(0., 0., 0.))
    hits = (B.rm_hit * 1)()
    occ = (C.c_uint8 * 1)()
    assert L.rm_intersect_rays(None, v, v, 1, hits) == E
    assert L.rm_occluded_rays(None, v, v, 1, occ) == E
    assert L.rm_intersect_rays_device(None, None, None, 1, None, None) == E
    assert L.rm_occluded_rays_device(None, None, None, 1, None, None) == E
    assert L.rm_pick(None, None, 0, 0, None) == E
    assert L.rm_primary_hits_device(None, None, None, None) == E
    assert L.rm_last_error(None) is not None


def test_queries_without_gpu_fail_loudly(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.BackendError) as e:
        pkg.backend.Context(0)
    assert e.value.status == pkg._lib.RM_ERR_NO_DEVICE
    with pytest.raises(pkg.BackendError):
        pkg.create_renderer(1.5, 64., 64.).pick(pkg.create_frame_buffer(64, 64), pkg.Scene.create_default(), 3, 4)


def test_python_ray_arrays_are_checked_before_the_library_sees_them(pkg):
    with pytest.raises(ValueError):
        pkg.backend._rays(np.zeros((4, 3)), np.zeros((5, 3)))
    with pytest.raises(ValueError):
        pkg.backend._rays(np.zeros((4, 2)), np.zeros((4, 2)))
    o, d = pkg.backend._rays([[0, 0, 0]], [[0, 0, -1]])
    assert o.dtype == np.float64 and d.shape == (1, 3)
