"""CPU-side checks of the radiance queries (include/rusty_marcher_amd.h, "radiance queries").

1. The four entry points are exported, bound by ctypes, the Rust shim and the C++ mirror with the header's shapes,
   rm_shading is 32 bytes everywhere, rm_build_info says " radiance", a NULL context is refused, and the Python wrappers
   check their arrays before the library sees them.
2. tests/radiance_reference.py -- the yardstick of the GPU tests -- is pinned to the oracle: its sample directions at integer
   positions, normalised by orc_normalized, are orc_backproject's bit for bit, and cast on the demo scene they are
   orc_render's frame bit for bit.
3. The ray sets the GPU tests use are not vacuous: asserted here on the oracle alone, with the committed seeds."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import radiance_reference as RR
import test_rust_binding as RB
import workloads

RADIANCE_FUNCTIONS = ["rm_radiance_rays", "rm_radiance_rays_device", "rm_radiance_samples", "rm_radiance_samples_device"]


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_radiance_abi"))


# ---------------------------------------------------------------- the ABI
def test_radiance_symbols_are_exported_and_bound(pkg):
    L = pkg.lib()
    for name in RADIANCE_FUNCTIONS:
        assert hasattr(L, name), "library does not export %s" % name
        assert name in pkg._lib.SIGNATURES
    for name in ("radiance", "radiance_device", "radiance_samples", "radiance_samples_device"):
        assert callable(getattr(pkg.backend.Context, name))
    assert callable(pkg.Renderer.render_supersampled)


def test_rm_shading_is_32_bytes_in_c_ctypes_and_rust(pkg, entry, tmp_path):
    src = tmp_path / "shading.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rusty_marcher_amd.h"\nint main(void){'
                   'printf("%zu %zu %zu\\n", sizeof(rm_shading), offsetof(rm_shading, max_depth), offsetof(rm_shading, _pad));'
                   'return 0;}\n')
    exe = tmp_path / "shading"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(entry.ROOT, "include"),
                           str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == [32, 24, 28]
    S = pkg._lib.rm_shading
    assert C.sizeof(S) == 32 and S.max_depth.offset == 24 and S._pad.offset == 28
    c, r = RB.header_structs(), RB.rust_structs()
    assert c["rm_shading"] == r["RmShading"] == [("background", "struct:RmVec3"), ("max_depth", "u32"), ("_pad", "u32")]


def test_radiance_functions_have_the_header_shapes_in_the_rust_shim_and_the_cpp_mirror(entry):
    c, r = RB.header_functions(), RB.rust_functions()
    for name in RADIANCE_FUNCTIONS:
        assert name in c and name in r, name
        assert c[name] == r[name], "%s: header %s, gpu.rs %s" % (name, c[name], r[name])
    assert c["rm_radiance_rays"] == ("i32", ["ptr", "ptr", "ptr", "u32", "ptr", "ptr"])
    assert c["rm_radiance_rays_device"] == ("i32", ["ptr", "ptr", "ptr", "u32", "ptr", "ptr", "ptr"])
    assert c["rm_radiance_samples"] == ("i32", ["ptr", "ptr", "ptr", "u32", "ptr"])
    assert c["rm_radiance_samples_device"] == ("i32", ["ptr", "ptr", "ptr", "u32", "ptr", "ptr"])
    text = open(RB.RUST).read()
    assert re.search(r"pub fn radiance\(\s*&mut self", text) and re.search(r"pub fn radiance_samples\(\s*&mut self", text)
    hpp = open(os.path.join(entry.PKG_DIR, "host", "rusty_marcher.hpp")).read()
    assert re.search(r"radiance\(const scene::Scene", hpp) and "rm_radiance_rays(" in hpp
    assert re.search(r"radiance_samples\(", hpp) and "rm_radiance_samples(" in hpp


def test_cpp_mirror_compiles_with_the_radiance_calls(entry, tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "rusty_marcher.hpp"\nint main() { return sizeof(rm_shading) == 32 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(entry.ROOT, "include"),
                           "-I", os.path.join(entry.PKG_DIR, "host"), str(src)])


def test_build_info_announces_radiance(pkg):
    L = pkg.lib()
    assert " radiance" in L.rm_build_info().decode()
    assert L.rm_abi_version() == 5


def test_radiance_entry_points_refuse_null_context(pkg):
    L, B = pkg.lib(), pkg._lib
    E = B.RM_ERR_INVALID_ARG
    v = (B.rm_vec3 * 1)(B.rm_vec3(0., 0., -1.))
    sh = B.rm_shading(B.rm_vec3(.1, .1, .1), 3, 0)
    p = pkg.backend.make_params(workloads.FOV, 64., 96., 3)
    xy = (C.c_double * 2)(1., 1.)
    assert L.rm_radiance_rays(None, v, v, 1, C.byref(sh), v) == E
    assert L.rm_radiance_rays_device(None, None, None, 1, C.byref(sh), None, None) == E
    assert L.rm_radiance_samples(None, C.byref(p), xy, 1, v) == E
    assert L.rm_radiance_samples_device(None, C.byref(p), None, 1, None, None) == E
    assert b"NULL ctx" in L.rm_last_error(None)
    assert v[0].z == -1.                                             # nothing written


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
    Ctx = K.Context
    ctx._device_rays = lambda *a, **k: Ctx._device_rays(ctx, *a, **k)
    p = K.make_params(workloads.FOV, 64., 96., 3)
    good = np.zeros((4, 3))
    for o, d in ((np.zeros((4, 2)), np.zeros((4, 2))), (np.zeros((4, 3)), np.zeros((5, 3))), (np.zeros(3), np.zeros(3))):
        with pytest.raises(ValueError):
            Ctx.radiance(ctx, o, d)
    for depth in (-1, 2.5):
        with pytest.raises(ValueError):
            Ctx.radiance(ctx, good, good, max_depth=depth)
    with pytest.raises((ValueError, TypeError)):
        Ctx.radiance(ctx, good, good, background=(0.1, 0.1))
    for xy in (np.zeros((4, 3)), np.zeros(4), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            Ctx.radiance_samples(ctx, p, xy)
    assert K._samples([[1, 2], [3, 4]]).dtype == np.float64 and K._samples(np.zeros((0, 2))).shape == (0, 2)
    # device variants: torch tensors, float64, (N, 3) / (N, 2), on the context's device, contiguous
    t3, t2 = torch.zeros((4, 3), dtype=torch.float64), torch.zeros((4, 2), dtype=torch.float64)
    for o, d in ((good, good), (t3.float(), t3.float()), (t3, t3), (torch.zeros((4, 2), dtype=torch.float64),) * 2):
        with pytest.raises(ValueError):                               # numpy; float32; on the CPU; wrong shape
            Ctx.radiance_device(ctx, o, d)
    for xy in (np.zeros((4, 2)), t2.float(), t2, torch.zeros((4, 3), dtype=torch.float64)):
        with pytest.raises(ValueError):
            Ctx.radiance_samples_device(ctx, p, xy)
    r = pkg.create_renderer(workloads.FOV, 64., 64.)
    for n in (0, 9, -1, 1.5):
        with pytest.raises(ValueError):
            r.render_supersampled(None, None, n)


# ---------------------------------------------------------------- the yardstick is pinned
@pytest.mark.parametrize("w,h", [(96, 64), (1920, 1080)])
def test_sample_directions_at_integer_positions_are_backproject(orc, w, h):
    d = RR.sample_directions(RR.pixel_positions(w, h), orc.renderer(w, h))
    assert np.array_equal(d[:, 2], -np.ones(w * h))
    got = orc.normalized(d)
    ref = orc.backproject(w, h).reshape(-1, 3)
    assert got.tobytes() == ref.tobytes(), "%d directions differ from orc_backproject" % int((got != ref).any(axis=1).sum())
    # ... and the fixed view written as a basis gives the same numbers (x * 1 + y * 0 and + -1 are exact)
    db = RR.sample_directions(RR.pixel_positions(w, h), orc.renderer(w, h), RR.FIXED_VIEW)
    assert np.array_equal(db, d)


def test_casting_the_sample_directions_is_orc_render(O, orc):
    oscene = workloads.oracle_scene(O, "demo")
    d = RR.sample_directions(RR.pixel_positions(64, 64), orc.renderer(64, 64))
    cam = oscene.c.camera.tup()
    got = orc.cast(oscene, cam, d, 3, normalize=True).reshape(64, 64, 3)
    ref = O.render(oscene, 64, 64, fov=workloads.FOV, max_depth=3)
    assert got.tobytes() == ref.tobytes()
    assert (ref.sum(axis=2) > 0).mean() > 0.25


def test_supersample_positions_are_the_samples_the_issue_states():
    xy = RR.supersample_positions(3, 2, 2).reshape(2, 3, 2, 2, 2)
    assert xy[1, 2, 0, 0].tolist() == [2., 1.] and xy[1, 2, 1, 0].tolist() == [2., 1.5] and xy[1, 2, 0, 1].tolist() == [2.5, 1.]
    assert np.array_equal(RR.supersample_positions(5, 4, 1), RR.pixel_positions(5, 4))
    x3 = RR.supersample_positions(7, 1, 3).reshape(7, 3, 3, 2)
    assert x3[6, 0, 2, 0] == 6. + 2. / 3.


# ---------------------------------------------------------------- the ray sets are not vacuous
@pytest.mark.parametrize("name", ["demo", "cornell", "synthetic256"])
def test_ray_sets_shade_something(pkg, O, orc, name):
    scene, oscene = workloads.product_scene(pkg, name), workloads.oracle_scene(O, name)
    desc = scene.flatten().desc()
    o, d = RR.rays_for(name, desc, np.random.default_rng(RR.SEEDS[name]))
    assert o.shape == d.shape == (RR.N_RAYS, 3)
    assert np.abs((d * d).sum(axis=1) - 1.).max() < 1e-12
    rgb, first, shape = orc.cast(oscene, o, d, 3, want_first=True)
    assert np.array_equal(shape >= 0, first >= 0)
    lit = (rgb != 0.).any(axis=1)
    assert lit.sum() >= RR.N_RAYS // 4 + 1, "%s: only %d of %d rays return radiance" % (name, int(lit.sum()), RR.N_RAYS)
    assert (first == -1).sum() > 0                                   # ... and some leave the scene
    assert np.array_equal(rgb[first == -1], np.zeros(((first == -1).sum(), 3)))
    if name == "demo":
        assert (first == 1).sum() >= 100, "only %d rays with a glass first hit" % int((first == 1).sum())


def test_pane_rays_reach_the_caps(pkg, O, orc):
    _, oscene = RR.pane_stack(pkg, O)
    o, d = RR.pane_rays(np.random.default_rng(RR.SEEDS["panes"]))
    assert np.abs((d * d).sum(axis=1) - 1.).max() < 1e-12
    by_depth = {k: orc.cast(oscene, o, d, k) for k in (0, 1, 2, 6, 17, 32)}
    assert np.all(by_depth[0] == 0.1)
    # (the stack is 13 panes and a sphere deep: the levels between 6 and 17 are really reached, none beyond)
    for a, b in ((1, 2), (2, 6), (6, 17)):
        assert (np.abs(by_depth[a] - by_depth[b]).max(axis=1) > 1e-9).sum() > 100, "caps %d and %d give the same picture" % (a, b)
