"""CPU-side checks of the ranged ray queries (include/rusty_marcher_amd.h, "ranged ray queries").

1. tests/ranged_reference.py -- the numpy yardstick of the GPU tests -- is pinned to the oracle: with [0, +inf] on every ray
   it gives the hit, the shape and the point of orc_find_closest_intersect and the answer of orc_intersect_shape_set,
   exactly, on the demo scene and the Cornell box.
2. The eight entry points are exported, bound by ctypes and the Rust shim with the header's shapes, rm_range is 16 bytes
   everywhere, rm_build_info says " ranges", a NULL context is refused, and the Python wrappers check their arrays."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ranged_reference as RR
import test_gpu_query as GQ
import test_rust_binding as RB
import workloads

RANGED_FUNCTIONS = ["rm_intersect_rays_ranged", "rm_occluded_rays_ranged", "rm_intersect_rays_ranged_device",
                    "rm_occluded_rays_ranged_device", "rm_visible_segments", "rm_visible_segments_device",
                    "rm_lights_visible", "rm_lights_visible_device"]


@pytest.fixture(scope="module")
def batch(O, entry, tmp_path_factory):
    d = tmp_path_factory.mktemp("orc_batch_ranged")
    src, so = d / "orc_batch.c", d / "orc_batch.so"
    src.write_text(GQ.BATCH_C)
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-shared", "-fPIC",
                           "-I", os.path.join(entry.ROOT, "oracle"), str(src), "-o", str(so)])
    return GQ.OracleBatch(O, C.CDLL(str(so)))


def rays_for(name, desc, rng, n):
    """n rays in the padded bounds of the scene; a quarter of them start inside a sphere (demo) or aim at a random point of
    a random triangle (Cornell: most of its walls lie along z, blind rays find few hits)."""
    lo, hi = GQ.bounds_of(desc)
    o, d = GQ.random_rays(rng, n, lo, hi)
    k = n // 4
    if name == "demo":
        o[:k] = GQ.inside_spheres(rng, desc, k)
    else:
        tri = np.array([[[v.x, v.y, v.z] for v in desc.triangles[i].vertices] for i in range(desc.n_triangles)])
        pick, b = rng.integers(0, len(tri), k), rng.dirichlet((1., 1., 1.), k)
        d[:k] = GQ.unit((tri[pick] * b[:, :, None]).sum(axis=1) - o[:k])
    return o, d


@pytest.mark.parametrize("name", ["demo", "cornell"])
def test_helper_with_the_full_range_is_the_oracle(pkg, O, batch, name):
    scene, oscene = workloads.product_scene(pkg, name), workloads.oracle_scene(O, name)
    handle = scene.flatten()
    desc = handle.desc()
    ref = RR.Scene(desc)
    o, d = rays_for(name, desc, np.random.default_rng(20261018), 20000)
    hit, shape, point, normal = batch.closest(oscene, o, d)
    got = ref.closest(o, d, (0., np.inf))
    assert np.array_equal(got["hit"], hit), "%d hit / miss decisions differ" % int((got["hit"] != hit).sum())
    m = hit == 1
    assert 0.05 * len(o) < m.sum() < len(o)
    assert np.array_equal(got["shape"][m] % 256, shape[m])
    assert np.array_equal(got["point"][m], point[m]), "points differ from the oracle's"
    assert np.array_equal(got["normal"][m], normal[m]), "normals differ from the oracle's"
    assert np.array_equal(o[m] + d[m] * got["t"][m][:, None], point[m])
    occ, _ = ref.occluded(o, d, (0., np.inf))
    assert np.array_equal(occ, batch.occluded(oscene, o, d).astype(bool))
    assert np.array_equal(occ, m)                                  # over [0, +inf] a closest hit and an occluder are one thing


def test_helper_range_rule_on_one_sphere(pkg):
    """The rule itself, on numbers one can do by hand: a sphere of radius 2 at z = -10, a ray down -z through
    its centre: roots 8 and 12."""
    s = pkg.Scene.new()
    s.shapes.append(pkg.sphere.create(pkg.Vec3f(0., 0., -10.), 2., pkg.Reflectance()))
    handle = s.flatten()
    ref = RR.Scene(handle.desc())
    o, d = np.zeros((5, 3)), np.tile([0., 0., -1.], (5, 1))
    r = np.array([[0., np.inf], [9., np.inf], [0., 7.], [9., 11.], [8., 8.]])
    got = ref.closest(o, d, r)
    assert got["hit"].tolist() == [1, 1, 0, 0, 1]
    assert got["t"].tolist() == [8., 12., 0., 0., 8.]
    assert got["normal"][1].tolist() == [0., 0., -1.] and got["normal"][0].tolist() == [0., 0., 1.]
    assert ref.occluded(o, d, r)[0].tolist() == [True, True, False, False, True]
    assert got["near_end"].tolist() == [False, False, False, False, True]
    vis, _ = ref.visible(np.array([[0., 0., 0.], [0., 0., 0.], [0., 0., 0.]]), np.array([[0., 0., -20.], [0., 0., -7.], [0., 0., -20.]]),
                         np.array(0.))
    assert vis.tolist() == [False, True, False]
    assert ref.visible(np.zeros((1, 3)), np.array([[0., 0., -20.]]), 10.5)[0].tolist() == [True]      # an empty range sees


# ---------------------------------------------------------------- the ABI
def test_ranged_symbols_are_exported_and_bound(pkg):
    L = pkg.lib()
    for name in RANGED_FUNCTIONS:
        assert hasattr(L, name), "library does not export %s" % name
        assert name in pkg._lib.SIGNATURES
    assert (pkg._lib.RM_LIGHTS_AS_RENDERED, pkg._lib.RM_LIGHTS_CLIPPED) == (0, 1)


def test_rm_range_is_16_bytes_in_c_ctypes_and_rust(pkg, entry, tmp_path):
    src = tmp_path / "range.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rusty_marcher_amd.h"\nint main(void){'
                   'printf("%zu %zu %u %u\\n", sizeof(rm_range), offsetof(rm_range, t_max), RM_LIGHTS_AS_RENDERED, RM_LIGHTS_CLIPPED);'
                   'return 0;}\n')
    exe = tmp_path / "range"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(entry.ROOT, "include"),
                           str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == [16, 8, 0, 1]
    R = pkg._lib.rm_range
    assert C.sizeof(R) == 16 and R.t_max.offset == 8
    c, r = RB.header_structs(), RB.rust_structs()
    assert c["rm_range"] == r["RmRange"] == [("t_min", "f64"), ("t_max", "f64")]


def test_ranged_functions_have_the_header_shapes_in_the_rust_shim_and_the_cpp_mirror(entry):
    c, r = RB.header_functions(), RB.rust_functions()
    for name in RANGED_FUNCTIONS:
        assert name in c and name in r, name
        assert c[name] == r[name], "%s: header %s, gpu.rs %s" % (name, c[name], r[name])
    assert c["rm_visible_segments"] == ("i32", ["ptr", "ptr", "ptr", "u32", "f64", "ptr"])
    assert c["rm_lights_visible"] == ("i32", ["ptr", "ptr", "ptr", "u32", "u32", "u32", "ptr"])
    text = open(RB.RUST).read()
    assert re.search(r"pub fn visible\(\s*&mut self", text) and re.search(r"pub fn lit_by\(\s*&mut self", text)
    hpp = open(os.path.join(entry.PKG_DIR, "host", "rusty_marcher.hpp")).read()
    assert re.search(r"bool visible\(", hpp) and "rm_visible_segments(" in hpp
    assert re.search(r"lit_by\(", hpp) and "rm_lights_visible(" in hpp


def test_build_info_announces_the_ranges(pkg):
    L = pkg.lib()
    assert " ranges" in L.rm_build_info().decode()
    assert L.rm_abi_version() == 5


def test_ranged_entry_points_refuse_null_context(pkg):
    L, B = pkg.lib(), pkg._lib
    E = B.RM_ERR_INVALID_ARG
    v = (B.rm_vec3 * 1)(B.rm_vec3(0., 0., -1.))
    rg = (B.rm_range * 1)(B.rm_range(0., 1.))
    hits = (B.rm_hit * 1)()
    out = (C.c_uint8 * 1)()
    assert L.rm_intersect_rays_ranged(None, v, v, rg, 1, hits) == E
    assert L.rm_occluded_rays_ranged(None, v, v, rg, 1, out) == E
    assert L.rm_intersect_rays_ranged_device(None, None, None, None, 1, None, None) == E
    assert L.rm_occluded_rays_ranged_device(None, None, None, None, 1, None, None) == E
    assert L.rm_visible_segments(None, v, v, 1, 0., out) == E
    assert L.rm_visible_segments_device(None, None, None, 1, 0., None, None) == E
    assert L.rm_lights_visible(None, v, v, 1, 1, 0, out) == E
    assert L.rm_lights_visible_device(None, None, None, 1, 1, 0, None, None) == E
    assert b"NULL ctx" in L.rm_last_error(None)


def test_python_ranges_and_pairs_are_checked_before_the_library_sees_them(pkg):
    K = pkg.backend
    with pytest.raises(ValueError):
        K._ranges(np.zeros((5, 2)), 4)
    with pytest.raises(ValueError):
        K._ranges(np.zeros((4, 3)), 4)
    with pytest.raises(ValueError):
        K._ranges([1., 2., 3.], 4)
    r = K._ranges((0., np.inf), 3)
    assert r.shape == (3, 2) and r.dtype == np.float64 and r.flags["C_CONTIGUOUS"] and r[2].tolist() == [0., np.inf]
    assert K._ranges(np.arange(8).reshape(4, 2), 4).dtype == np.float64
    with pytest.raises(ValueError):
        K._pairs(np.zeros((4, 3)), np.zeros((5, 3)), ("a", "b"))
    with pytest.raises(ValueError):
        K._pairs(np.zeros((4, 2)), np.zeros((4, 2)), ("points", "normals"))
    a, b = K._pairs([[0, 0, 0]], [[0, 0, -1]], ("a", "b"))
    assert a.dtype == np.float64 and b.shape == (1, 3)
