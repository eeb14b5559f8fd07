"""Swept hierarchies under a moving camera on the GPU (-m gpu): rm_accumulate_camera_swept_device through the C ABI and the
Python bindings, against the flat passes of rm_accumulate_camera_device given the same four tables -- byte for byte, as the
header says -- against rm_accumulate_swept_device where the camera stands, and against tests/camera_motion_reference.py within
TIGHT = 1e-9 on every channel of every pixel (n TIGHT of a sum of n samples).

The context is oriented and the camera both translates and turns.  Frames are 32 x 32 (64 x 64 for the chain scenes, whose trees
are deep), a pass casts 3 to 8 rows, depth 5 takes the kernels with 4 parked rays a lane, depth 6 those with 32."""
import ctypes as C

import numpy as np
import pytest

import camera_motion_reference as CM
import hierarchy_reference as HR
import moving_reference as MV
import radiance_reference as RR
import swept_reference as SW
import test_gpu_lens as GL
import test_gpu_motion as GM
import test_gpu_moving as GMV
import test_gpu_progressive as GP
import test_gpu_swept as GSW

pytestmark = pytest.mark.gpu

NAN, BYTE = GP.NAN, GP.BYTE
same, held = GMV.same, GM.held
FIXED = RR.FIXED_VIEW
CASES, case_id, scene_of, tables = GSW.CASES, GSW.case_id, GSW.scene_of, GSW.tables
VIEW, DEFAULT_VIEW = GSW.VIEW, GSW.DEFAULT_VIEW
TURN = (0.05, -0.03, 0.02)                                              # how the context is oriented: a turn of the fixed view
CAMERA_TURN = (0.15, 0.05, -0.1)                                        # yaw, pitch and roll of the camera over the shutter
FLAT, SWEPT = "accumulate_camera_device", "accumulate_camera_swept_device"


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_camera_swept"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return CM.Yardstick(pkg, O, orc)


def oriented(pkg, c, scene):
    """Uploads the scene and turns the context's view -> its basis as a tuple.  The caller puts the fixed view back."""
    GL.upload(c, scene)
    c.orient(pkg.backend.basis_turn(FIXED, *TURN))
    _, basis, on = c.camera()
    assert on
    return RR.basis_tuple(basis)


def camera_of(c, name, n):
    """Rows 0 .. n of the library's camera sequence from the context's basis: a camera that translates by a sixth of the scene's
    test speed and turns."""
    speed = MV.SPEED.get(name, MV.CELL_SPEED) / 6.
    return c.camera_sequence(0, n, (speed, 0.4 * speed, -0.5 * speed), MV.SHUTTER, CAMERA_TURN)


def run(pkg, c, name, depth, table, camera, lights, shapes, sizes, call, **kw):
    """GSW.run with a camera table: passes of the sizes `sizes` over consecutive slices of the four tables, into buffers that
    held NaN (and BYTE) -> (sum, mean, bytes) as numpy."""
    import torch
    side, fov, aperture, focus = VIEW.get(name, DEFAULT_VIEW)
    p = pkg.backend.make_params(fov, float(side), float(side), depth)
    total = torch.full((side, side, 3), NAN, dtype=torch.float64, device="cuda:0")
    mean = torch.full((side, side, 3), NAN, dtype=torch.float64, device="cuda:0")
    rgb8 = torch.full((side, side, 3), BYTE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    done = 0
    assert sum(sizes) == len(table) == len(camera) == len(lights) == len(shapes)
    for n in sizes:
        rows = slice(done, done + n)
        getattr(c, call)(p, total, aperture, focus, np.ascontiguousarray(table[rows]), np.ascontiguousarray(camera[rows]),
                         np.ascontiguousarray(lights[rows]), np.ascontiguousarray(shapes[rows]), done, mean=mean, rgb8=rgb8, **kw)
        done += n
    torch.cuda.synchronize()
    return total.cpu().numpy(), mean.cpu().numpy(), rgb8.cpu().numpy()


# ---------------------------------------------------------------- 1. the flat pass's bytes
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_a_swept_camera_pass_leaves_the_flat_camera_passs_bytes(pkg, ctx, Y, case):
    """Every scene, both stacks and, on the matrix's scenes, both powers: 3 + 5 rows of the library's four sequences with the test
    velocities.  The handle is the binding's own, from the shape table's extents.  `seventeen` and `thirteen` end in a partial
    last leaf: a rule asked for a primitive the leaf does not hold would read behind the pid map's end."""
    name, generic, depth = case
    key, scene = scene_of(Y, name, generic)
    try:
        oriented(pkg, ctx, scene)
        table, lights, shapes, _ = tables(ctx, Y, key, name, 8)
        camera = camera_of(ctx, name, 8)
        assert (shapes != 0.).any() and (camera[1:, :3] != 0.).any() and (camera[1:, 3:] != camera[0, 3:]).any()
        flat = run(pkg, ctx, name, depth, table, camera, lights, shapes, (3, 5), FLAT)
        swept = run(pkg, ctx, name, depth, table, camera, lights, shapes, (3, 5), SWEPT)
    finally:
        ctx.orient(None)
    same(swept, flat, case_id(case))
    assert flat[1].any() and len(np.unique(flat[2])) > 4                # a picture, not a background


# ---------------------------------------------------------------- 2. parity with the yardstick
@pytest.mark.parametrize("name,depth", [("matrix-spheres", 5), ("matrix-mesh", 5), ("cornell", 3)])
def test_swept_camera_frames_match_the_yardstick(pkg, ctx, Y, name, depth):
    key, scene = scene_of(Y, name)
    try:
        oriented(pkg, ctx, scene)
        table, lights, shapes, _ = tables(ctx, Y, key, name, 8)
        camera = camera_of(ctx, name, 8)
        got = run(pkg, ctx, name, depth, table, camera, lights, shapes, (8,), SWEPT)
    finally:
        ctx.orient(None)
    _, _, aperture, focus = DEFAULT_VIEW
    ref_sum, ref_mean = Y.camera(key, 32, 32, depth, aperture, focus, table, camera, lights, shapes, (8,))
    held(got, ref_sum, ref_mean, 8, "%s depth %d, 8 rows through a swept hierarchy under a moving camera" % (name, depth))


# ---------------------------------------------------------------- 3. identities
@pytest.mark.parametrize("name,depth", [("matrix-spheres", 5), ("matrix-mesh", 6)])
def test_standing_rows_are_the_swept_pass_byte_for_byte(pkg, ctx, Y, name, depth):
    """An oriented context and every row its basis with an offset of zero: rm_accumulate_swept_device's bytes."""
    key, scene = scene_of(Y, name)
    try:
        basis = oriented(pkg, ctx, scene)
        table, lights, shapes, _ = tables(ctx, Y, key, name, 8)
        got = run(pkg, ctx, name, depth, table, CM.standing_rows(8, basis), lights, shapes, (3, 5), SWEPT)
        ref = GSW.run(pkg, ctx, name, depth, table, lights, shapes, (3, 5), GSW.SWEPT)
    finally:
        ctx.orient(None)
    same(got, ref, "%s, standing rows" % name)
    assert ref[1].any()


def test_constant_rows_are_the_swept_pass_of_a_context_moved_there(pkg, ctx, Y):
    """Every row the same offset and the same basis B: the swept pass of a context whose camera was set to fl(cam + off) by
    rm_camera_update and to B by rm_camera_orient."""
    key, scene = scene_of(Y, "matrix-mesh")
    GL.upload(ctx, scene)
    try:
        pos, _, _ = ctx.camera()
        cam, off = np.array([pos.x, pos.y, pos.z]), np.array([0.37, -0.6, 0.9])
        B = pkg.backend.basis_turn(FIXED, 0.1, -0.05, 0.05)
        table, lights, shapes, _ = tables(ctx, Y, key, "matrix-mesh", 8)
        got = run(pkg, ctx, "matrix-mesh", 5, table, CM.standing_rows(8, RR.basis_tuple(B), off), lights, shapes, (3, 5), SWEPT)
        ctx.set_camera(tuple(cam + off))
        ctx.orient(B)
        same(got, GSW.run(pkg, ctx, "matrix-mesh", 5, table, lights, shapes, (3, 5), GSW.SWEPT), "constant rows")
        assert got[1].any()
    finally:
        ctx.orient(None)
        GL.upload(ctx, scene)


def test_passes_of_3_5_and_8_rows_are_one_pass_of_16(pkg, ctx, Y):
    key, scene = scene_of(Y, "matrix-spheres")
    try:
        oriented(pkg, ctx, scene)
        table, lights, shapes, v = tables(ctx, Y, key, "matrix-spheres", 16)
        camera = camera_of(ctx, "matrix-spheres", 16)
        handle = ctx.swept(*pkg.backend.swept_motion_extents(v, MV.SHUTTER))
        try:
            one = run(pkg, ctx, "matrix-spheres", 5, table, camera, lights, shapes, (16,), SWEPT, swept=handle)
            three = run(pkg, ctx, "matrix-spheres", 5, table, camera, lights, shapes, (3, 5, 8), SWEPT, swept=handle)
        finally:
            handle.close()
        flat = run(pkg, ctx, "matrix-spheres", 5, table, camera, lights, shapes, (16,), FLAT)
    finally:
        ctx.orient(None)
    same(three, one, "3 + 5 + 8")
    same(one, flat, "16 rows against the flat camera pass")


# ---------------------------------------------------------------- 4. the boxes are consulted
def test_a_row_outside_the_extents_is_missed(pkg, ctx, Y, orc):
    """test_gpu_swept.py's teeth through the new call, with standing camera rows of the fixed view: a handle with extents of zero
    and a table that moves one small sphere of matrix-spheres by several times its radius across the view.  The flat camera pass
    shows it where the row puts it, the swept pass looks for it in boxes about where it was.  The input breaks the header's
    precondition and is safe by its contract: no offset, box or camera row forms an address.  Without this test a kernel that
    quietly walks flat passes every other one.

    Which sphere: the first whose moved self is the closest hit of 8 or more pixel-centre rays the image's own boxes never lead
    to, by tests/hierarchy_reference.py's walk model on the CPU."""
    key, scene = scene_of(Y, "matrix-spheres")
    desc, img = HR.image_of(pkg, scene)
    xy = RR.pixel_positions(32, 32) + 0.5
    d = RR.sample_directions(xy, orc.renderer(32, 32))
    d /= np.linalg.norm(d, axis=1)[:, None]
    o = np.zeros_like(d)
    n_shapes = desc.n_shapes
    chosen = None
    for k in range(n_shapes - 20, n_shapes):                            # the 20 small spheres are the last shapes
        r = float(np.sqrt(desc.spheres[desc.shapes[k].first].radius_square))
        for sign in (1., -1.):
            row = np.zeros((n_shapes, 3))
            row[k, 0] = sign * 5. * r
            ref = SW.MovedRanged(desc, row).closest(o, d, (0., np.inf))
            lost = HR.unreached(img, o, d, HR.pid_of(img, ref["shape"], ref["element"])) & (ref["shape"] == k)
            if lost.sum() >= 8:
                chosen = (k, row, int(lost.sum()))
                break
        if chosen:
            break
    assert chosen, "no small sphere leaves its boxes in plain sight"
    k, row, lost = chosen
    GL.upload(ctx, scene)
    assert not ctx.camera()[2]
    n = 5
    table, lights, camera = ctx.lens_sequence(0, n), np.zeros((n, Y.n_lights(key), 3)), CM.standing_rows(n)
    shapes = np.tile(row, (n, 1, 1))
    still = np.zeros_like(shapes)
    flat = run(pkg, ctx, "pinhole", 3, table, camera, lights, shapes, (n,), FLAT)
    handle = ctx.swept(np.zeros((n_shapes, 3)), np.zeros((n_shapes, 3)))
    try:
        zero = run(pkg, ctx, "pinhole", 3, table, camera, lights, shapes, (n,), SWEPT, swept=handle)
        # (the same handle with rows it does hold is the flat pass: what differs below is the boxes' doing)
        same(run(pkg, ctx, "pinhole", 3, table, camera, lights, still, (n,), SWEPT, swept=handle),
             run(pkg, ctx, "pinhole", 3, table, camera, lights, still, (n,), FLAT), "zero rows, zero extents")
    finally:
        handle.close()
    differ = int((zero[1] != flat[1]).any(axis=2).sum())
    print("shape %d moved out of its boxes: %d pixel centres lose it in the model, %d pixels differ on the GPU" % (k, lost, differ))
    assert not np.isnan(zero[1]).any() and differ >= 1
    same(run(pkg, ctx, "pinhole", 3, table, camera, lights, shapes, (n,), SWEPT), flat, "the same rows under a handle that holds them")


# ---------------------------------------------------------------- 5. images without a hierarchy
def test_a_context_without_hierarchies_takes_the_flat_camera_kernel(pkg, ctx, Y, monkeypatch):
    """RM_DISABLE_BVH=1: the image of matrix-spheres holds no hierarchy; the pass is the flat camera pass, and the bytes are
    those of the context that walks one."""
    key, scene = scene_of(Y, "matrix-spheres")
    B = pkg.backend.basis_turn(FIXED, *TURN)
    try:
        oriented(pkg, ctx, scene)
        table, lights, shapes, _ = tables(ctx, Y, key, "matrix-spheres", 5)
        camera = camera_of(ctx, "matrix-spheres", 5)
        with_bvh = run(pkg, ctx, "matrix-spheres", 5, table, camera, lights, shapes, (5,), SWEPT)
    finally:
        ctx.orient(None)
    monkeypatch.setenv("RM_DISABLE_BVH", "1")
    c = pkg.backend.Context(0)
    try:
        GL.upload(c, scene)
        c.orient(B)
        flat = run(pkg, c, "matrix-spheres", 5, table, camera, lights, shapes, (5,), FLAT)
        same(run(pkg, c, "matrix-spheres", 5, table, camera, lights, shapes, (5,), SWEPT), flat, "RM_DISABLE_BVH=1")
    finally:
        c.close()
    same(with_bvh, flat, "with and without the image's hierarchy")
    assert flat[1].any()


# ---------------------------------------------------------------- 6. refusals
def test_refusals_name_the_offender_and_the_buffers_keep_their_bytes(pkg, ctx, Y):
    """A stale handle, another context's handle, a freed handle and a NULL shape table, through the C ABI itself (the binding
    refuses a closed or foreign handle before the library is called); the three guarded output buffers keep every byte, and the
    context still serves."""
    import torch
    L, B = pkg.lib(), pkg._lib
    key, scene = scene_of(Y, "matrix-mesh")
    other_key, other = scene_of(Y, "thirteen")
    GL.upload(ctx, scene)
    n_shapes, n_lights = Y.n_shapes(key), Y.n_lights(key)
    p = pkg.backend.make_params(GSW.DEFAULT_VIEW[1], 32., 32., 3)
    n, guard = 32 * 32 * 3, 4096
    bufs = [torch.full((n + guard,), NAN, dtype=torch.float64, device="cuda:0"), torch.full((n + guard,), NAN, dtype=torch.float64, device="cuda:0"),
            torch.full((n + guard,), BYTE, dtype=torch.uint8, device="cuda:0")]
    before = [b.cpu().numpy().copy() for b in bufs]
    total, mean, rgb8 = (b[:n].view(32, 32, 3) for b in bufs)
    lens = B.rm_lens(0., 1., 5, 0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")

    def raw(c, swept, shapes_of, lights_of, with_shapes=True):
        """The C call on context `c`; the tables are zeros for a scene of that many shapes and lights."""
        table, camera = dev(c.lens_sequence(0, 5)), dev(CM.standing_rows(5))
        lights, shapes = dev(np.zeros((5, lights_of, 3))), dev(np.zeros((5, shapes_of, 3)))
        st = L.rm_accumulate_camera_swept_device(c.ptr, C.byref(p), C.byref(lens), C.c_void_p(table.data_ptr()), C.c_void_p(camera.data_ptr()),
                                                 C.c_void_p(lights.data_ptr()), lights_of, C.c_void_p(shapes.data_ptr()) if with_shapes else None,
                                                 shapes_of, swept, 0, C.c_void_p(total.data_ptr()), C.c_void_p(mean.data_ptr()),
                                                 C.c_void_p(rgb8.data_ptr()), None)
        torch.cuda.synchronize()
        return st, L.rm_last_error(c.ptr)

    def untouched():
        torch.cuda.synchronize()
        return all(b.cpu().numpy().tobytes() == a.tobytes() for b, a in zip(bufs, before))

    who = b"rm_accumulate_camera_swept_device: "
    handle = ctx.swept(np.zeros((n_shapes, 3)), np.zeros((n_shapes, 3)))
    c2 = pkg.backend.Context(0)
    try:
        GL.upload(c2, scene)
        foreign = c2.swept(np.zeros((n_shapes, 3)), np.zeros((n_shapes, 3)))
        st, err = raw(ctx, foreign.ptr, n_shapes, n_lights)              # another context's
        assert st == B.RM_ERR_INVALID_ARG and err == who + b"swept is not a handle of this context", err
        st, err = raw(ctx, handle.ptr, n_shapes, n_lights, with_shapes=False)   # a NULL shape table
        assert st == B.RM_ERR_INVALID_ARG and err == who + b"NULL shape offsets", err
        st, err = raw(ctx, None, n_shapes, n_lights)                     # no handle at all
        assert st == B.RM_ERR_INVALID_ARG and err == who + b"NULL swept", err
        assert untouched()
        GL.upload(ctx, other)                                            # stale: the scene changed
        st, err = raw(ctx, handle.ptr, Y.n_shapes(other_key), Y.n_lights(other_key))
        assert st == B.RM_ERR_INVALID_ARG and err.startswith(who + b"swept was built before the scene last changed"), err
        GL.upload(ctx, scene)                                            # ... also once the first scene is back
        st, err = raw(ctx, handle.ptr, n_shapes, n_lights)
        assert st == B.RM_ERR_INVALID_ARG and b"before the scene last changed" in err, err
        freed = C.c_void_p(handle.ptr.value)
        handle.close()                                                   # freed: looked up, not looked into
        st, err = raw(ctx, freed, n_shapes, n_lights)
        assert st == B.RM_ERR_INVALID_ARG and err == who + b"swept is not a handle of this context", err
        assert untouched()
        with pytest.raises(ValueError, match="open Swept handle"):      # the binding's own refusals
            ctx.accumulate_camera_swept_device(p, total, 0., 1., ctx.lens_sequence(0, 5), CM.standing_rows(5), np.zeros((5, n_lights, 3)),
                                               np.zeros((5, n_shapes, 3)), 0, swept=handle)
        with pytest.raises(ValueError, match="open Swept handle"):
            ctx.accumulate_camera_swept_device(p, total, 0., 1., ctx.lens_sequence(0, 5), CM.standing_rows(5), np.zeros((5, n_lights, 3)),
                                               np.zeros((5, n_shapes, 3)), 0, swept=foreign)
        assert untouched()
        fresh = ctx.swept(np.zeros((n_shapes, 3)), np.zeros((n_shapes, 3)))
        try:
            st, err = raw(ctx, fresh.ptr, n_shapes, n_lights)            # ... and the context still serves
            assert st == 0, err
        finally:
            fresh.close()
        assert not untouched() and not np.isnan(total.cpu().numpy()).any()
    finally:
        handle.close()
        c2.close()
