"""CPU-side checks of the moving shapes (include/rusty_marcher_amd.h, "moving shapes").

1. The two entry points are exported and bound by ctypes, the Rust shim and the C++ mirror with the header's shapes,
   rm_build_info says " moving-shapes" and the ABI is still 5, a NULL context is refused with nothing written, and the Python
   wrappers raise before the library is called.
2. tests/moving_reference.py -- the yardstick of the GPU tests -- is motion_reference.samples byte for byte when every shape
   offset is zero and when only spheres have one, moves a triangle as the oracle's own orc_triangle_offset does, moves of a
   polygon the plane point and the vertices alone, and is not vacuous: the frames the GPU tests compare differ from the frames
   with only the spheres moving in the committed numbers of pixels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lens_reference as LR
import motion_reference as MR
import moving_reference as MV
import progressive_reference as PR
import radiance_reference as RR
import soft_reference as SR
import test_rust_binding as RB
import variant_matrix as VM
import workloads

FUNCTIONS = ["rm_accumulate_moving_device", "rm_render_progressive_moving"]
D, U8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_moving_abi"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return MV.Yardstick(pkg, O, orc)


@pytest.fixture(scope="module")
def matrix(pkg, O, orc):
    return VM.Matrix(pkg, O, orc)


# ---------------------------------------------------------------- the ABI
def test_moving_symbols_are_exported_and_bound(pkg, entry):
    L = pkg.lib()
    header = open(os.path.join(entry.ROOT, "include", "rusty_marcher_amd.h")).read()
    lib_py = open(os.path.join(entry.PKG_DIR, "_lib.py")).read()
    for name in FUNCTIONS:
        assert hasattr(L, name), "library does not export %s" % name
        assert name in pkg._lib.SIGNATURES and '"%s"' % name in lib_py
        assert re.search(r"^rm_status %s\(" % name, header, flags=re.M), name
    assert "moving shapes" in header and "moving spheres" in header
    for name in ("accumulate_moving_device", "render_progressive_moving"):
        assert callable(getattr(pkg.backend.Context, name))
    assert callable(pkg.Renderer.render_progressive_moving) and callable(pkg.Renderer.render_moving_shapes)


def test_moving_functions_have_the_header_shapes_in_the_rust_shim_and_the_cpp_mirror(entry):
    c, r = RB.header_functions(), RB.rust_functions()
    for name in FUNCTIONS:
        assert name in c and name in r, name
        assert c[name] == r[name], "%s: header %s, gpu.rs %s" % (name, c[name], r[name])
    assert c["rm_accumulate_moving_device"] == c["rm_accumulate_motion_device"] == ("i32", ["ptr"] * 5 + ["u32", "ptr", "u32", "u32"] + ["ptr"] * 4)
    assert c["rm_render_progressive_moving"] == c["rm_render_progressive_motion"] == ("i32", ["ptr"] * 4 + ["u32", "ptr", "u32", "f64", "i32"] + ["ptr"] * 4)
    text = open(RB.RUST).read()
    assert re.search(r"pub fn render_progressive_moving\(\s*&mut self", text) and "rm_render_progressive_moving(self.ctx" in text
    assert re.search(r"pub fn accumulate_moving\(\s*&mut self", text) and "rm_accumulate_moving_device(self.ctx" in text
    hpp = open(os.path.join(entry.PKG_DIR, "host", "rusty_marcher.hpp")).read()
    assert re.search(r"render_progressive_moving\(framebuffer::FrameBuffer", hpp) and "rm_render_progressive_moving" in hpp


def test_cpp_mirror_compiles_with_the_moving_render(entry, tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "rusty_marcher.hpp"\nusing namespace rusty_marcher;\n'
                   'std::string tick(renderer::Renderer &r, framebuffer::FrameBuffer &fb, const scene::Scene &sc) {'
                   ' std::vector<Vec3f> v(sc.shapes.size(), Vec3f{0., 1., 0.}); v[0] = Vec3f{1., 0., 0.5};'
                   ' r.render_progressive_moving(fb, sc, v, 1., 8u); r.render_progressive_motion(fb, sc, v, 1., 8u);'
                   ' return r.render_progressive_moving(fb, sc, v, 0.5, 8u, {1.5, 0.}, 0.4, 5., true); }\n'
                   'int main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(entry.ROOT, "include"),
                           "-I", os.path.join(entry.PKG_DIR, "host"), str(src)])


def test_build_info_announces_moving_shapes(pkg):
    L = pkg.lib()
    info = L.rm_build_info().decode()
    assert " moving-shapes" in info and " motion" in info
    assert L.rm_abi_version() == 5


def test_moving_entry_points_refuse_null_context(pkg):
    L, B = pkg.lib(), pkg._lib
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 3)
    lens = B.rm_lens(LR.APERTURE, LR.FOCUS, 4, 0)
    v = np.ascontiguousarray([[2., -1., 0.5], [0., 1., 0.], [-0.125, 3., -7.]])
    frame, bytes8, total = np.full((64, 64, 3), 7.25), np.full((64, 64, 3), 7, np.uint8), C.c_uint32(77)
    assert L.rm_accumulate_moving_device(None, C.byref(p), C.byref(lens), None, None, 2, None, 3, 0, None, None, None, None) == B.RM_ERR_INVALID_ARG
    assert b"rm_accumulate_moving_device: NULL ctx" in L.rm_last_error(None)
    assert L.rm_render_progressive_moving(None, C.byref(p), C.byref(lens), None, 0, v.ctypes.data_as(C.POINTER(B.rm_vec3)), 3, 1., 0,
                                          frame.ctypes.data_as(D), bytes8.ctypes.data_as(U8), C.byref(total), None) == B.RM_ERR_INVALID_ARG
    assert b"rm_render_progressive_moving: NULL ctx" in L.rm_last_error(None)
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
    demo = pkg.Scene.create_default()
    n = len(demo.shapes)
    good = [pkg.Vec3f(1., 0., 0.5)] * n                                # a velocity on every shape, the floor too
    r, fb = pkg.create_renderer(workloads.FOV, 64., 64.), pkg.create_frame_buffer(64, 64)
    for bad in ([(nan, 0., 0.)] + [None] * (n - 1), [(0., inf, 0.)] + [None] * (n - 1), [(1., 2.)] + [None] * (n - 1), 1.5, None, "12"):
        with pytest.raises(ValueError):
            K.Context.render_progressive_moving(ctx, p, bad, 1., 0.4, 5., 4)
        with pytest.raises(ValueError):
            r.render_progressive_moving(fb, demo, bad, 1., 4)
        with pytest.raises(ValueError):
            r.render_moving_shapes(fb, demo, bad, 1., 4)
    for bad in ([], good[:-1], good + [None]):
        with pytest.raises(ValueError, match="one velocity a shape"):
            r.render_progressive_moving(fb, demo, bad, 1., 4)
        with pytest.raises(ValueError, match="one velocity a shape"):
            r.render_moving_shapes(fb, demo, bad, 1., 4)
    for shutter in (-0.1, nan, inf, "1", None, True):
        with pytest.raises(ValueError, match="shutter"):
            K.Context.render_progressive_moving(ctx, p, good, shutter, 0.4, 5., 4)
        with pytest.raises(ValueError, match="shutter"):
            r.render_progressive_moving(fb, demo, good, shutter, 4)
    for radii in ((-0.1, 1.), (nan, 1.), "12", 1.5):
        with pytest.raises(ValueError):
            K.Context.render_progressive_moving(ctx, p, good, 1., 0.4, 5., 4, radii=radii)
        with pytest.raises(ValueError):
            r.render_progressive_moving(fb, demo, good, 1., 4, light_radii=radii)
    with pytest.raises(ValueError, match="one radius a light"):
        r.render_progressive_moving(fb, demo, good, 1., 4, light_radii=(1.5,))
    for aperture, focus, ns in ((-0.1, 5., 4), (0.4, 0., 4), (0.4, 5., 0), (0.4, 5., 65), (0.4, 5., 2.5)):
        with pytest.raises(ValueError):
            K.Context.render_progressive_moving(ctx, p, good, 1., aperture, focus, ns)
        with pytest.raises(ValueError):
            r.render_progressive_moving(fb, demo, good, 1., ns, aperture=aperture, focus=focus)
    for ns in (0, -1, 65537, 2.5, True):
        with pytest.raises(ValueError):
            r.render_moving_shapes(fb, demo, good, 1., ns)
    for host_rgb, host_rgb8 in ((np.zeros((32, 64, 3)), None), (np.zeros((64, 64, 3), np.float32), None), (None, np.zeros((64, 32, 3), np.uint8))):
        with pytest.raises(ValueError):
            K.Context.render_progressive_moving(ctx, p, good, 1., 0.4, 5., 4, host_rgb=host_rgb, host_rgb8=host_rgb8)
    t = torch.zeros((64, 64, 3), dtype=torch.float64)
    table, lights, shapes = PR.lens_sequence(0, 4), np.zeros((4, 2, 3)), np.zeros((4, n, 3))
    for s in (np.zeros((64, 64, 3)), t.float(), t, torch.zeros((64, 32, 3), dtype=torch.float64), None):
        with pytest.raises(ValueError):
            K.Context.accumulate_moving_device(ctx, p, s, 0.4, 5., table, lights, shapes, 0)


# ---------------------------------------------------------------- the yardstick
def test_the_test_velocities_move_every_shape_and_keep_the_spheres(Y):
    for name in ("demo", "cornell", "pool"):
        kinds = Y.kinds(name)
        v = MV.velocities(kinds, MV.SPEED[name])
        assert v.shape == (len(kinds), 3) and (v != 0.).any(axis=1).all()
        spheres = np.array(kinds) == MV.ORC_SPHERE
        assert v[spheres].tobytes() == MR.velocities(kinds)[spheres].tobytes()
    one = MV.velocities(Y.kinds("cornell"), MV.SPEED["cornell"], MV.CORNELL_MOVER)
    assert list(np.flatnonzero((one != 0.).any(axis=1))) == [MV.CORNELL_MOVER]


def test_zero_and_sphere_only_offsets_are_the_motion_yardstick_byte_for_byte(O, orc, Y):
    table = PR.lens_sequence(0, 8)
    for name, aperture in (("demo", 0.), ("demo", LR.APERTURE), ("cornell", LR.APERTURE), ("pool", 0.)):
        oscene, eye, kinds = Y.scene(name)[1], Y.eye(name), Y.kinds(name)
        lights = SR.light_sequence(0, 8, (1.5,) * Y.n_lights(name))
        for zero in (0., -0.):
            z = np.full((8, len(kinds), 3), zero)
            a = MV.samples(O, orc, oscene, eye, None, 32, 32, 3, aperture, LR.FOCUS, table, lights, z)
            b = MR.samples(O, orc, oscene, eye, None, 32, 32, 3, aperture, LR.FOCUS, table, lights, z)
            assert a.tobytes() == b.tobytes(), name
        only = MV.spheres_only(MR.motion_sequence(0, 8, MV.velocities(kinds, MV.SPEED[name]), MV.SHUTTER), kinds)
        a = MV.samples(O, orc, oscene, eye, None, 32, 32, 3, aperture, LR.FOCUS, table, lights, only)
        b = MR.samples(O, orc, oscene, eye, None, 32, 32, 3, aperture, LR.FOCUS, table, lights, only)
        assert a.tobytes() == b.tobytes() and a.any(), name
    assert MV.ORC_SPHERE in Y.kinds("demo") and MV.ORC_SPHERE in Y.kinds("pool")


def test_a_moved_triangle_is_the_oracles_own_offset_bit_for_bit(O, Y):
    L = O.lib()
    src = Y.scene("cornell")[1].c
    rng = np.random.default_rng(20261941)
    for k in range(src.n_shapes):
        s = src.shapes[k]
        assert s.kind == MV.ORC_OBJ
        for i in range(s.n_triangles):
            off = rng.uniform(-300., 300., 3) * (1. if i % 3 else 1e-7)
            ours = MV.moved_triangle(O, s.triangles[i], off)
            theirs = O.Triangle.from_buffer_copy(bytes(s.triangles[i]))
            L.orc_triangle_offset(C.byref(theirs), O.v3(off))
            assert bytes(ours) == bytes(theirs), (k, i)
            assert bytes(ours) != bytes(s.triangles[i])
            assert ours.normal.tup() == s.triangles[i].normal.tup()
    # ... and so is every triangle of a MovedScene, whose other Objs stand where they stood
    row = np.zeros((src.n_shapes, 3))
    row[MV.CORNELL_MOVER] = (12.5, -3., 7.)
    moved = MV.MovedScene(O, Y.scene("cornell")[1], np.zeros((src.n_lights, 3)), row)
    for k in range(src.n_shapes):
        a, b = src.shapes[k], moved.c.shapes[k]
        assert a.n_triangles == b.n_triangles and C.addressof(a.triangles.contents) != C.addressof(b.triangles.contents)
        assert C.addressof(a.reflectances.contents) == C.addressof(b.reflectances.contents)       # the materials are the scene's
        for i in range(a.n_triangles):
            theirs = O.Triangle.from_buffer_copy(bytes(a.triangles[i]))
            if k == MV.CORNELL_MOVER:
                L.orc_triangle_offset(C.byref(theirs), O.v3(row[k]))
            assert bytes(b.triangles[i]) == bytes(theirs), (k, i)


def test_a_moved_polygon_differs_in_the_plane_point_and_the_vertices_alone(O, Y):
    oscene = Y.scene("pool")[1]                                       # a quad, a pentagon, a hexagon, a sphere
    src = oscene.c
    assert Y.kinds("pool") == [1, 1, 1, MV.ORC_SPHERE]
    assert [int(src.shapes[k].n_vertices) for k in range(3)] == [4, 5, 6]
    size = C.sizeof(O.Shape)
    before = C.string_at(src.shapes, size * src.n_shapes)
    soff = np.array([[0.5, -0.25, 3.], [1e-9, 7., -2.], [-4., 0., 0.125], [3.5, 0.25, -1.]])
    moved = MV.MovedScene(O, oscene, np.zeros((src.n_lights, 3)), soff)
    assert C.string_at(src.shapes, size * src.n_shapes) == before                        # the source is left alone
    for k in range(3):
        a, b = src.shapes[k], moved.c.shapes[k]
        assert C.addressof(a.vertices.contents) != C.addressof(b.vertices.contents)      # vertices of its own
        assert b.plane_point.tup() == tuple(np.array(a.plane_point.tup()) + soff[k])
        for i in range(a.n_vertices):
            assert b.vertices[i].tup() == tuple(np.array(a.vertices[i].tup()) + soff[k])
        assert b.plane_normal.tup() == a.plane_normal.tup()
        back = O.Shape.from_buffer_copy(C.string_at(C.addressof(b), size))
        back.plane_point, back.vertices = a.plane_point, a.vertices
        assert bytes(back) == before[k * size:(k + 1) * size]                             # every other byte the source's
    # a ray at the pentagon's centre meets it where it stands, and not once it has moved 7 up
    L = O.lib()

    def first_hit(scene_c, target):
        hit = O.Intersection()
        got = L.orc_find_closest_intersect(O.v3(0., 0., 0.), L.orc_normalized(O.v3(target)), scene_c.shapes, scene_c.n_shapes, C.byref(hit), None)
        return hit.reflectance.diffuse_color.tup() if got else None
    centre = np.mean(np.array(MV.POOL_PENTAGON), axis=0)
    assert first_hit(src, centre) == MV.POOL_PENTAGON_MATERIAL["diffuse_color"]
    assert first_hit(moved.c, centre) != MV.POOL_PENTAGON_MATERIAL["diffuse_color"]
    assert first_hit(moved.c, centre + soff[1]) == MV.POOL_PENTAGON_MATERIAL["diffuse_color"]


def moving_and_spheres_only(Y, name, depth, rows, aperture, focus, v):
    table = PR.lens_sequence(0, rows)
    lights = np.zeros((rows, Y.n_lights(name), 3))
    shapes = MR.motion_sequence(0, rows, v, MV.SHUTTER)
    _, moving = Y.moving(name, 32, 32, depth, aperture, focus, table, lights, shapes, (rows,))
    _, motion = Y.motion(name, 32, 32, depth, aperture, focus, table, lights, MV.spheres_only(shapes, Y.kinds(name)), (rows,))
    return int((np.abs(moving - motion) > 0.05).any(axis=2).sum())


@pytest.mark.parametrize("name", sorted(MV.BLURRED))
def test_moving_frames_are_another_picture_than_the_moving_spheres(Y, name):
    """Non-vacuity of the yardstick alone, at the settings the GPU tests use: a pinhole, point lights, shutter 1."""
    depth, rows, pixels = MV.BLURRED[name]
    scene = "cornell" if name == "cornell-one" else name
    v = MV.velocities(Y.kinds(scene), MV.SPEED[scene], MV.CORNELL_MOVER if name == "cornell-one" else None)
    differ = moving_and_spheres_only(Y, scene, depth, rows, 0., LR.FOCUS, v)
    print("%s 32x32, depth %d, %d rows: %d pixels differ from the frame with only the spheres moving by more than 0.05" % (name, depth, rows, differ))
    assert differ == pixels and pixels > VM.SHARE * 32 * 32


@pytest.mark.parametrize("cell", VM.CELLS, ids=VM.cell_id)
def test_moving_frames_of_the_matrix_cells_are_another_picture(Y, matrix, cell):
    bvh, generic, depth = cell
    name = VM.register(Y, matrix.name(bvh, generic), matrix.pair(bvh, generic))
    differ = moving_and_spheres_only(Y, name, depth, MV.CELL_ROWS, VM.APERTURE, VM.FOCUS, MV.velocities(Y.kinds(name), MV.CELL_SPEED))
    print("%s: %d pixels differ from the frame with only the spheres moving by more than 0.05" % (VM.cell_id(cell), differ))
    assert differ == MV.BLURRED_CELLS[VM.cell_id(cell)] and differ > VM.SHARE * VM.W * VM.H
