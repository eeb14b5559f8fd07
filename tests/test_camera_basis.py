"""CPU-side checks of the oriented camera (include/rusty_marcher_amd.h, "the oriented camera"): the host arithmetic --
look-at, turn, the orthonormality check -- against numpy, rm_camera_basis laid out as declared in C, ctypes and the Rust
shim, the entry points' refusals, and the Python Scene's optional basis.  Nothing here needs a GPU."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import test_rust_binding as RB

CAMERA_FUNCTIONS = ["rm_camera_orient", "rm_camera_look_at", "rm_camera_get", "rm_camera_basis_look_at",
                    "rm_camera_basis_turn", "rm_camera_basis_check"]
FIXED = np.array([[1., 0., 0.], [0., 1., 0.], [0., 0., -1.]])


def as_array(b):
    return np.array([[v.x, v.y, v.z] for v in (b.right, b.up, b.forward)])


def make_basis(pkg, m):
    B = pkg._lib
    return B.rm_camera_basis(*[B.rm_vec3(*[float(c) for c in row]) for row in m])


def look_at(pkg, eye, target, up):
    """(status, basis)"""
    B = pkg._lib
    out = B.rm_camera_basis()
    st = pkg.lib().rm_camera_basis_look_at(B.rm_vec3(*eye), B.rm_vec3(*target), B.rm_vec3(*up), C.byref(out))
    return st, out


def turn(pkg, basis, yaw, pitch, roll):
    out = pkg._lib.rm_camera_basis()
    st = pkg.lib().rm_camera_basis_turn(C.byref(basis), yaw, pitch, roll, C.byref(out))
    return st, out


def test_camera_symbols_are_exported_and_bound(pkg):
    L = pkg.lib()
    for name in CAMERA_FUNCTIONS:
        assert hasattr(L, name), "library does not export %s" % name
        assert name in pkg._lib.SIGNATURES
    assert " camera" in L.rm_build_info().decode()
    assert L.rm_abi_version() == 5


def test_look_at_of_the_fixed_view_is_the_fixed_view(pkg):
    st, b = look_at(pkg, (0., 0., 0.), (0., 0., -1.), (0., 1., 0.))
    assert st == 0
    got = as_array(b)
    # == component by component (a -0 a cross product leaves compares equal to 0)
    assert all(got[i, j] == FIXED[i, j] for i in range(3) for j in range(3)), got
    assert pkg.lib().rm_camera_basis_check(C.byref(b)) == 0


def test_look_at_against_numpy_for_a_thousand_random_views(pkg):
    rng = np.random.default_rng(20261016)
    L = pkg.lib()
    n = 0
    while n < 1000:
        eye, target, up = rng.uniform(-50., 50., 3), rng.uniform(-50., 50., 3), rng.normal(size=3)
        d = target - eye
        if np.linalg.norm(d) < 1e-3 or np.linalg.norm(up) < 1e-3:
            continue
        f = d / np.linalg.norm(d)
        angle = math.atan2(np.linalg.norm(np.cross(f, up)), abs(float(np.dot(f, up))))     # off the line of sight, either way
        if angle <= 0.1:
            continue
        n += 1
        st, b = look_at(pkg, eye, target, up)
        assert st == 0
        assert L.rm_camera_basis_check(C.byref(b)) == 0
        m = as_array(b)
        assert np.abs(m[2] - f).max() <= 1e-14
        assert float(np.dot(m[1], up)) > 0.
        # right-handed as documented: up = right x forward
        assert np.abs(np.cross(m[0], m[2]) - m[1]).max() <= 1e-14


def test_look_at_refusals(pkg):
    E = pkg._lib.RM_ERR_INVALID_ARG
    assert look_at(pkg, (1., 2., 3.), (1., 2., 3.), (0., 1., 0.))[0] == E            # eye == target
    assert look_at(pkg, (0., 0., 0.), (0., 5., 0.), (0., 1., 0.))[0] == E            # up_hint along the line of sight
    assert look_at(pkg, (0., 0., 0.), (0., 5., 0.), (0., -2., 0.))[0] == E           # ... or against it
    assert look_at(pkg, (0., 0., 0.), (0., 0., -1.), (0., 0., 0.))[0] == E           # no up_hint at all
    assert look_at(pkg, (float("nan"), 0., 0.), (0., 0., -1.), (0., 1., 0.))[0] == E
    assert look_at(pkg, (0., 0., 0.), (float("inf"), 0., -1.), (0., 1., 0.))[0] == E
    assert look_at(pkg, (0., 0., 0.), (0., 0., -1.), (0., float("nan"), 0.))[0] == E
    assert b"up_hint" in pkg.lib().rm_last_error(None)
    B = pkg._lib
    assert pkg.lib().rm_camera_basis_look_at(B.rm_vec3(0., 0., 0.), B.rm_vec3(0., 0., -1.), B.rm_vec3(0., 1., 0.), None) == E


def test_turn_by_nothing_returns_its_input(pkg):
    rng = np.random.default_rng(7)
    for _ in range(50):
        st, b = look_at(pkg, rng.uniform(-10, 10, 3), rng.uniform(-10, 10, 3), (0.1, 1., 0.2))
        assert st == 0
        st, t = turn(pkg, b, 0., 0., 0.)
        assert st == 0
        assert np.abs(as_array(t) - as_array(b)).max() <= 1e-14


def test_a_thousand_small_turns_stay_orthonormal(pkg):
    L = pkg.lib()
    b = make_basis(pkg, FIXED)
    for i in range(1000):
        st, b = turn(pkg, b, 0.01, 0.01 if i % 2 else -0.007, 0.01 if i % 3 else -0.01)
        assert st == 0
        assert L.rm_camera_basis_check(C.byref(b)) == 0
    m = as_array(b)
    assert np.abs(m @ m.T - np.eye(3)).max() <= 1e-12
    assert np.abs(np.cross(m[0], m[2]) - m[1]).max() <= 1e-12        # still right-handed


def test_turn_sign_conventions(pkg):
    fixed = make_basis(pkg, FIXED)
    # positive yaw turns left: the fixed view (down -z) yawed by pi/2 looks down -x
    st, b = turn(pkg, fixed, math.pi / 2., 0., 0.)
    assert st == 0
    m = as_array(b)
    assert np.abs(m[2] - [-1., 0., 0.]).max() <= 1e-14
    assert np.abs(m[1] - [0., 1., 0.]).max() <= 1e-14
    assert np.abs(m[0] - [0., 0., -1.]).max() <= 1e-14
    # positive pitch looks up
    m = as_array(turn(pkg, fixed, 0., math.pi / 2., 0.)[1])
    assert np.abs(m[2] - [0., 1., 0.]).max() <= 1e-14 and np.abs(m[0] - [1., 0., 0.]).max() <= 1e-14
    # positive roll tips up towards right
    m = as_array(turn(pkg, fixed, 0., 0., math.pi / 2.)[1])
    assert np.abs(m[1] - [1., 0., 0.]).max() <= 1e-14 and np.abs(m[2] - [0., 0., -1.]).max() <= 1e-14
    # a mirrored basis stays mirrored
    left = make_basis(pkg, FIXED * np.array([[-1.], [1.], [1.]]))
    m = as_array(turn(pkg, left, 0.3, 0.2, 0.1)[1])
    assert np.abs(np.cross(m[0], m[2]) + m[1]).max() <= 1e-14
    # in == out is allowed
    b = make_basis(pkg, FIXED)
    assert pkg.lib().rm_camera_basis_turn(C.byref(b), 0.25, 0., 0., C.byref(b)) == 0
    assert abs(b.forward.x + math.sin(0.25)) <= 1e-14


def test_basis_check_bounds(pkg):
    L, E = pkg.lib(), pkg._lib.RM_ERR_INVALID_ARG
    assert L.rm_camera_basis_check(C.byref(make_basis(pkg, FIXED))) == 0
    assert L.rm_camera_basis_check(C.byref(make_basis(pkg, FIXED * np.array([[-1.], [1.], [1.]])))) == 0     # left-handed: accepted
    skew = FIXED.copy(); skew[0] = [1., 1e-6, 0.]
    assert L.rm_camera_basis_check(C.byref(make_basis(pkg, skew))) == E
    assert L.rm_camera_basis_check(C.byref(make_basis(pkg, FIXED * 1.001))) == E
    nan = FIXED.copy(); nan[1, 1] = float("nan")
    assert L.rm_camera_basis_check(C.byref(make_basis(pkg, nan))) == E
    inf = FIXED.copy(); inf[2, 0] = float("inf")
    assert L.rm_camera_basis_check(C.byref(make_basis(pkg, inf))) == E
    assert L.rm_camera_basis_check(None) == E
    # within the bounds: a squared length 5e-13 off
    near = FIXED.copy(); near[0, 0] = 1. + 2.5e-13
    assert L.rm_camera_basis_check(C.byref(make_basis(pkg, near))) == 0
    assert turn(pkg, make_basis(pkg, skew), 0.1, 0., 0.)[0] == E
    assert L.rm_camera_basis_turn(None, 0., 0., 0., None) == E
    assert turn(pkg, make_basis(pkg, FIXED), float("nan"), 0., 0.)[0] == E


def test_rm_camera_basis_is_72_bytes_in_c_ctypes_and_rust(pkg, entry, tmp_path):
    src = tmp_path / "basis.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rusty_marcher_amd.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu\\n", sizeof(rm_camera_basis), offsetof(rm_camera_basis, right),'
                   ' offsetof(rm_camera_basis, up), offsetof(rm_camera_basis, forward));return 0;}\n')
    exe = tmp_path / "basis"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(entry.ROOT, "include"),
                           str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == [72, 0, 24, 48]
    T = pkg._lib.rm_camera_basis
    assert C.sizeof(T) == 72
    assert [getattr(T, f).offset for f in ("right", "up", "forward")] == [0, 24, 48]
    c, r = RB.header_structs(), RB.rust_structs()
    assert "rm_camera_basis" in c and "RmCameraBasis" in r
    assert c["rm_camera_basis"] == r["RmCameraBasis"]
    assert [n for n, _ in c["rm_camera_basis"]] == ["right", "up", "forward"]
    assert "#[repr(C)]" in re.search(r"((?:#\[[^\]]*\]\s*)+)pub struct RmCameraBasis", open(RB.RUST).read()).group(1)


def test_camera_functions_have_the_header_shapes_in_the_mirrors(entry):
    c, r = RB.header_functions(), RB.rust_functions()
    for name in CAMERA_FUNCTIONS:
        assert name in c and name in r, name
        assert c[name] == r[name], "%s: header %s, gpu.rs %s" % (name, c[name], r[name])
    assert c["rm_camera_look_at"] == ("i32", ["ptr", "struct:RmVec3", "struct:RmVec3", "struct:RmVec3"])
    assert c["rm_camera_basis_turn"] == ("i32", ["ptr", "f64", "f64", "f64", "ptr"])
    rust = open(RB.RUST).read()
    assert re.search(r"pub fn look_at\(\s*&mut self", rust) and re.search(r"pub fn orient\(\s*&mut self", rust)
    hpp = open(os.path.join(entry.PKG_DIR, "host", "rusty_marcher.hpp")).read()
    assert "rm_camera_orient(" in hpp and re.search(r"rm_camera_basis look_at\(", hpp)


def test_context_entry_points_refuse_null_with_a_status(pkg):
    L, B = pkg.lib(), pkg._lib
    E = B.RM_ERR_INVALID_ARG
    b = make_basis(pkg, FIXED)
    assert L.rm_camera_orient(None, C.byref(b)) == E
    assert L.rm_camera_orient(None, None) == E
    assert L.rm_camera_look_at(None, B.rm_vec3(0., 0., 0.), B.rm_vec3(0., 0., -1.), B.rm_vec3(0., 1., 0.)) == E
    assert L.rm_camera_get(None, None, None, None) == E
    assert b"NULL ctx" in L.rm_last_error(None)


def test_without_a_gpu_init_still_fails_loudly(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    ctx = C.c_void_p()
    assert pkg.lib().rm_init(0, C.byref(ctx)) == pkg._lib.RM_ERR_NO_DEVICE
    assert b"no CPU fallback" in pkg.lib().rm_last_error(None)
    s = pkg.Scene.create_default()
    s.look_at((0., 0., -16.))
    with pytest.raises(pkg.BackendError):
        pkg.create_renderer(1.5, 64., 64.).render(pkg.create_frame_buffer(64, 64), s)


def test_scene_carries_an_optional_basis(pkg):
    s = pkg.Scene.create_default()
    assert s.basis is None
    s.camera = pkg.Vec3f(25., 10., 5.)
    s.look_at((0., 0., -16.))
    m = as_array(s.basis)
    eye = np.array([s.camera.x, s.camera.y, s.camera.z])
    f = np.array([0., 0., -16.]) - eye
    assert np.abs(m[2] - f / np.linalg.norm(f)).max() <= 1e-14
    before = m.copy()
    s.turn(yaw=0.2)
    after = as_array(s.basis)
    assert np.abs(after[1] - before[1]).max() <= 1e-14                 # yaw: about up
    assert abs(float(np.dot(after[2], before[2])) - math.cos(0.2)) <= 1e-14
    t = pkg.Scene.new()
    t.turn(yaw=math.pi / 2.)                                           # from the fixed view
    assert np.abs(as_array(t.basis)[2] - [-1., 0., 0.]).max() <= 1e-14
    with pytest.raises(pkg.BackendError):
        t.look_at((t.camera.x, t.camera.y, t.camera.z))                # eye == target
