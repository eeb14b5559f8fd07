"""The moving camera on the GPU (-m gpu): rm_accumulate_camera_device and rm_render_progressive_camera through the C ABI and the
Python bindings, against tests/camera_motion_reference.py -- row s of every pixel cast by the CPU oracle from the camera of row
s of the camera table against the scene moved by row s of the two offset tables, folded in table order across passes (pinned on
the CPU by tests/test_camera_motion_abi.py) -- and against the frames of rm_accumulate_soft_device and
rm_accumulate_moving_device.

What the header calls byte for byte is demanded byte for byte; against the yardstick every channel of every pixel of the rows a
pass writes is demanded within TIGHT = 1e-9 of the mean (n TIGHT of a sum of n samples), no pixel left out.  Frames are 32 x 32
(32 x 40 where rows matter) and a pass casts at most 16 rows.  Depth 3 takes the kernels with 4 parked rays a lane, depth 6 on
the 256 spheres those with 32 and the sphere hierarchy."""
import numpy as np
import pytest

import camera_motion_reference as CM
import lens_reference as LR
import motion_reference as MR
import moving_reference as MV
import progressive_reference as PR
import radiance_reference as RR
import soft_reference as SR
import test_gpu_lens as GL
import test_gpu_motion as GM
import test_gpu_moving as GV
import test_gpu_progressive as GP
import test_gpu_query as GQ
import test_gpu_soft as GS
import workloads

pytestmark = pytest.mark.gpu

TIGHT = CM.TIGHT
NAN, BYTE = GP.NAN, GP.BYTE
held, same = GM.held, GV.same
FIXED = RR.FIXED_VIEW
# case -> (radii or None for point lights, aperture, shapes move as well): every case of camera_motion_reference.MOTIONS
CASES = {"demo-translate": (None, 0., False), "demo-turn": (None, 0., False), "demo-both": ((1.5, 3.), LR.APERTURE, False),
         "cornell": (None, 0., False), "synthetic256": (None, LR.APERTURE, False), "pool": (SR.PENUMBRA_RADII, LR.APERTURE, True)}


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_camera"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return CM.Yardstick(pkg, O, orc)


def run_camera(pkg, c, w, h, depth, aperture, focus, table, camera, lights, shapes, sizes, want_mean=True, want_bytes=True):
    """Passes of the sizes `sizes` over consecutive slices of the four tables (shapes None: no shape table) on torch's current
    stream, the first with n_before = 0, into buffers that held NaN (and BYTE) -> (sum, mean, bytes) as numpy."""
    import torch
    p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)
    total = torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda:0")
    mean = torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda:0") if want_mean else None
    rgb8 = torch.full((h, w, 3), BYTE, dtype=torch.uint8, device="cuda:0") if want_bytes else None
    torch.cuda.synchronize()
    done = 0
    assert sum(sizes) == len(table) == len(camera) == len(lights) and max(sizes) <= 16
    for n in sizes:
        rows = slice(done, done + n)
        c.accumulate_camera_device(p, total, aperture, focus, np.ascontiguousarray(table[rows]), np.ascontiguousarray(camera[rows]),
                                   np.ascontiguousarray(lights[rows]), None if shapes is None else np.ascontiguousarray(shapes[rows]), done,
                                   mean=mean, rgb8=rgb8)
        done += n
    torch.cuda.synchronize()
    return (total.cpu().numpy(), mean.cpu().numpy() if want_mean else None, rgb8.cpu().numpy() if want_bytes else None)


def library_tables(ctx, Y, case, first, n, basis=FIXED):
    """Rows first .. first + n of the library's four sequences for the case: its motion, its radii, the test velocities."""
    name, depth, velocity, turn = CM.MOTIONS[case]
    radii, aperture, moving = CASES[case]
    lights = ctx.light_sequence(first, n, radii) if radii is not None else np.zeros((n, Y.n_lights(name), 3))
    shapes = ctx.motion_sequence(first, n, MV.velocities(Y.kinds(name), MV.SPEED[name]), CM.SHUTTER) if moving else None
    camera = ctx.camera_sequence(first, n, velocity, CM.SHUTTER, turn, basis)
    assert np.abs(camera - CM.camera_rows(first, n, velocity, turn, basis)).max() < 1e-14
    return ctx.lens_sequence(first, n), camera, lights, shapes


def side_view(ctx, scene):
    """Puts the context at a place beside the scene looking at its middle -> (eye, basis tuple, focus)."""
    lo, hi = GQ.bounds_of(scene.flatten().desc())
    pos, _, _ = ctx.camera()
    eye = np.array([pos.x, pos.y, pos.z]) + np.array([0.12, 0.06, 0.]) * np.linalg.norm(hi - lo)
    ctx.look_at(tuple(eye), tuple((lo + hi) / 2.))
    pos, basis, on = ctx.camera()
    assert on
    return (pos.x, pos.y, pos.z), RR.basis_tuple(basis), float(np.linalg.norm((lo + hi) / 2. - eye))


# ---------------------------------------------------------------- 1. parity with the yardstick
@pytest.mark.parametrize("case", sorted(CASES))
def test_camera_frames_match_the_yardstick(pkg, ctx, Y, case):
    """16 rows of the library's sequences in passes of 8, and 5 rows of tables that are not the library's: another camera, another
    turn and other offsets for every row, so a lane that reads another sample's row, a lens point formed from the context's basis
    or a focus point from the context's camera is another picture.  The pinhole cases are the frames of the non-vacuity pins."""
    name, depth, velocity, turn = CM.MOTIONS[case]
    radii, aperture, moving = CASES[case]
    GL.upload(ctx, Y.scene(name)[0])
    table, camera, lights, shapes = library_tables(ctx, Y, case, 0, 16)
    got = run_camera(pkg, ctx, 32, 32, depth, aperture, LR.FOCUS, table, camera, lights, shapes, (8, 8))
    ref_sum, ref_mean = Y.camera(name, 32, 32, depth, aperture, LR.FOCUS, table, camera, lights, shapes, (8, 8))
    held(got, ref_sum, ref_mean, 16, "%s depth %d, 2 x 8 rows, aperture %g" % (case, depth, aperture))
    if aperture == 0.:
        still = Y.camera(name, 32, 32, depth, 0., LR.FOCUS, table, CM.standing_rows(16), lights, None, (16,))[1]
        moved = int((np.abs(ref_mean - still) > 0.05).any(axis=2).sum())
        print("    %d pixels differ from the standing camera's frame" % moved)
        assert moved == CM.BLURRED[case] > 0.05 * 1024                      # the frame test_camera_motion_abi.py pins
    rng = np.random.default_rng(20261020)
    table = LR.random_table(rng, 5)
    camera = CM.random_rows(rng, 5, MV.SPEED[name] / 6.)
    lights = SR.random_offsets(rng, 5, Y.n_lights(name))
    shapes = MV.random_offsets(rng, 5, Y.kinds(name), MV.SPEED[name] / 3.) if moving else None
    for a in (0., LR.APERTURE):
        got = run_camera(pkg, ctx, 32, 32, depth, a, LR.FOCUS, table, camera, lights, shapes, (5,))
        ref_sum, ref_mean = Y.camera(name, 32, 32, depth, a, LR.FOCUS, table, camera, lights, shapes, (5,))
        held(got, ref_sum, ref_mean, 5, "%s depth %d, 5 random rows, aperture %g" % (case, depth, a))


def test_oriented_context(pkg, ctx, Y):
    """A look_at context: the sequence turns the basis rm_camera_get reports, and the offsets start from its position."""
    scene = Y.scene("demo")[0]
    GL.upload(ctx, scene)
    try:
        eye, basis, focus = side_view(ctx, scene)
        table, lights = ctx.lens_sequence(0, 8), ctx.light_sequence(0, 8, (1.5, 3.))
        camera = ctx.camera_sequence(0, 8, (3., 0., 1.), CM.SHUTTER, (0.2, 0.1, -0.1))
        assert camera.tobytes() == pkg.backend.camera_sequence(0, 8, (3., 0., 1.), CM.SHUTTER, (0.2, 0.1, -0.1), basis).tobytes()
        got = run_camera(pkg, ctx, 32, 32, 3, LR.APERTURE, focus, table, camera, lights, None, (4, 4))
        ref_sum, ref_mean = Y.camera("demo", 32, 32, 3, LR.APERTURE, focus, table, camera, lights, None, (4, 4), eye)
        held(got, ref_sum, ref_mean, 8, "demo from the side, 2 x 4 rows")
        fixed = Y.camera("demo", 32, 32, 3, LR.APERTURE, focus, table, camera, lights, None, (4, 4))[1]
        assert GL.worst(ref_mean, fixed) > 0.05                        # ... and it is another picture than from the scene's camera
    finally:
        ctx.orient(None)


# ---------------------------------------------------------------- 2. what the header calls byte for byte
@pytest.mark.parametrize("name,depth", [("demo", 3), ("cornell", 3), ("synthetic256", 6)])
def test_standing_rows_are_the_underlying_pass_byte_for_byte(pkg, ctx, Y, name, depth, monkeypatch):
    """An oriented context and every row its basis with an offset of zero, +0. in the first pass and -0. in the second, two passes
    of 5 samples (four idle lanes): without a shape table rm_accumulate_soft_device's bytes, with one
    rm_accumulate_moving_device's.  Without a shape table the 256 spheres keep their hierarchy: the same bytes with RM_DISABLE_BVH=1."""
    scene = Y.scene(name)[0]
    GL.upload(ctx, scene)
    try:
        eye, basis, focus = side_view(ctx, scene)
        table = ctx.lens_sequence(0, 10)
        lights = ctx.light_sequence(0, 10, (1.5,) * Y.n_lights(name))
        shapes = ctx.motion_sequence(0, 10, MV.velocities(Y.kinds(name), MV.SPEED[name]), CM.SHUTTER)
        camera = CM.standing_rows(10, basis)
        camera[5:, :3] = -0.
        soft = GS.run_soft(pkg, ctx, 32, 32, depth, LR.APERTURE, focus, table, lights, (5, 5))
        still = run_camera(pkg, ctx, 32, 32, depth, LR.APERTURE, focus, table, camera, lights, None, (5, 5))
        same(still, soft, "%s, standing rows, static scene" % name)
        moving = GV.run_moving(pkg, ctx, 32, 32, depth, LR.APERTURE, focus, table, lights, shapes, (5, 5))
        both = run_camera(pkg, ctx, 32, 32, depth, LR.APERTURE, focus, table, camera, lights, shapes, (5, 5))
        same(both, moving, "%s, standing rows, moving scene" % name)
        assert soft[1].any() and GL.worst(moving[1], soft[1]) > 0.05
        # the hierarchy against the flat walk, with the camera moving
        camera = ctx.camera_sequence(0, 10, (2., 1., 0.), CM.SHUTTER, (0.1, 0., 0.05))
        free = run_camera(pkg, ctx, 32, 32, depth, LR.APERTURE, focus, table, camera, lights, None, (5, 5))
        monkeypatch.setenv("RM_DISABLE_BVH", "1")
        c = pkg.backend.Context(0)
        try:
            c.upload(scene.flatten())
            c.look_at(eye, tuple(np.asarray(eye) + focus * np.asarray(basis[2])))
            assert bytes(c.camera()[1]) == bytes(ctx.camera()[1])
            flat = run_camera(pkg, c, 32, 32, depth, LR.APERTURE, focus, table, camera, lights, None, (5, 5))
        finally:
            c.close()
        same(flat, free, "%s, RM_DISABLE_BVH=1" % name)
    finally:
        ctx.orient(None)


def test_constant_rows_are_the_pass_of_a_context_moved_there(pkg, ctx, Y):
    """Every row the same offset and the same basis B: byte for byte the underlying pass of a context whose camera was set to
    fl(cam + off) by rm_camera_update and to B by rm_camera_orient."""
    scene = Y.scene("pool")[0]
    GL.upload(ctx, scene)
    try:
        pos, _, _ = ctx.camera()
        cam = np.array([pos.x, pos.y, pos.z])
        off = np.array([0.37, -1.1, 2.3])
        B = pkg.backend.basis_turn(FIXED, 0.2, -0.1, 0.05)
        table, lights = ctx.lens_sequence(0, 10), ctx.light_sequence(0, 10, SR.PENUMBRA_RADII)
        shapes = ctx.motion_sequence(0, 10, MV.velocities(Y.kinds("pool"), MV.SPEED["pool"]), CM.SHUTTER)
        camera = CM.standing_rows(10, RR.basis_tuple(B), off)
        still = run_camera(pkg, ctx, 32, 32, 3, LR.APERTURE, LR.FOCUS, table, camera, lights, None, (5, 5))
        both = run_camera(pkg, ctx, 32, 32, 3, LR.APERTURE, LR.FOCUS, table, camera, lights, shapes, (5, 5))
        ctx.set_camera(tuple(cam + off))
        ctx.orient(B)
        same(still, GS.run_soft(pkg, ctx, 32, 32, 3, LR.APERTURE, LR.FOCUS, table, lights, (5, 5)), "constant rows, static scene")
        same(both, GV.run_moving(pkg, ctx, 32, 32, 3, LR.APERTURE, LR.FOCUS, table, lights, shapes, (5, 5)), "constant rows, moving scene")
    finally:
        ctx.orient(None)
        GL.upload(ctx, scene)


def test_the_fixed_views_rows_under_a_context_that_is_not_oriented(pkg, ctx, Y):
    """The pass uses the oriented formula with the rows as given: against the fixed view's pass a zero direction component may
    change its sign (by is -0 on the row sy = height / 2), so the comparison is held to TIGHT, not to bytes."""
    GL.upload(ctx, Y.scene("demo")[0])
    assert not ctx.camera()[2]
    table, lights = ctx.lens_sequence(0, 8), ctx.light_sequence(0, 8, (1.5, 3.))
    soft = GS.run_soft(pkg, ctx, 32, 32, 3, LR.APERTURE, LR.FOCUS, table, lights, (8,))
    got = run_camera(pkg, ctx, 32, 32, 3, LR.APERTURE, LR.FOCUS, table, CM.standing_rows(8), lights, None, (8,))
    held(got, soft[0], soft[1], 8, "the fixed view's rows against the fixed view's pass")


# ---------------------------------------------------------------- 3. slicing, guard rows, a NaN row
def test_passes_of_3_5_and_8_rows_are_one_pass_of_16_byte_for_byte(pkg, ctx, Y):
    GL.upload(ctx, Y.scene("pool")[0])
    table, camera, lights, shapes = library_tables(ctx, Y, "pool", 0, 16)
    for g in (None, shapes):
        one = run_camera(pkg, ctx, 32, 32, 3, LR.APERTURE, LR.FOCUS, table, camera, lights, g, (16,))
        three = run_camera(pkg, ctx, 32, 32, 3, LR.APERTURE, LR.FOCUS, table, camera, lights, g, (3, 5, 8))
        same(three, one, "3 + 5 + 8")
        bare = run_camera(pkg, ctx, 32, 32, 3, LR.APERTURE, LR.FOCUS, table, camera, lights, g, (3, 5, 8), want_mean=False, want_bytes=False)
        assert bare[0].tobytes() == one[0].tobytes()                  # the optional outputs change nothing in the sum


def test_rows_below_the_last_patch_row_guards_and_a_nan_row(pkg, ctx, Y):
    """32 x 40: rows = 32.  The three buffers, their eight last rows and a guard region behind each hold NaN / BYTE beforehand;
    the camera table is read from an allocation with NaN rows behind it.  Then a table whose row 2 is NaN: nothing read from a
    camera row is an address, so the pass ends as any other -- the pixels are unspecified (a NaN ray hits nothing), the other
    three rows' share of them is not."""
    import torch
    GL.upload(ctx, Y.scene("pool")[0])
    p = pkg.backend.make_params(workloads.FOV, 40., 32., 3)
    n, guard = 40 * 32 * 3, 4096
    table, camera, lights, shapes = library_tables(ctx, Y, "pool", 0, 12)
    ref_sum, ref_mean = Y.camera("pool", 32, 40, 3, LR.APERTURE, LR.FOCUS, table, camera, lights, shapes, (7, 5))
    bufs = [torch.full((n + guard,), NAN, dtype=torch.float64, device="cuda:0"), torch.full((n + guard,), NAN, dtype=torch.float64, device="cuda:0"),
            torch.full((n + guard,), BYTE, dtype=torch.uint8, device="cuda:0")]
    before = [b.cpu().numpy().copy() for b in bufs]
    total, mean, rgb8 = (b[:n].view(40, 32, 3) for b in bufs)
    done = 0
    for k in (7, 5):
        wide = torch.full((k + 64, 12), NAN, dtype=torch.float64, device="cuda:0")
        wide[:k] = torch.from_numpy(np.ascontiguousarray(camera[done:done + k])).to("cuda:0")
        ctx.accumulate_camera_device(p, total, LR.APERTURE, LR.FOCUS, table[done:done + k], wide[:k], lights[done:done + k], shapes[done:done + k],
                                     done, mean=mean, rgb8=rgb8)
        done += k
    torch.cuda.synchronize()
    after = [b.cpu().numpy() for b in bufs]
    held(tuple(a[:32 * 32 * 3].reshape(32, 32, 3) for a in after), ref_sum[:32], ref_mean[:32], 12, "32 x 40, 7 + 5 rows")
    for a, b in zip(after, before):
        assert a[32 * 32 * 3:].tobytes() == b[32 * 32 * 3:].tobytes()     # rows 32 .. 39 and the guards
    bad = torch.from_numpy(np.ascontiguousarray(camera[:4])).to("cuda:0")
    bad[2] = NAN
    s = torch.zeros((32, 32, 3), dtype=torch.float64, device="cuda:0")
    small = pkg.backend.make_params(workloads.FOV, 32., 32., 3)
    for g in (None, shapes[:4]):
        ctx.accumulate_camera_device(small, s, LR.APERTURE, LR.FOCUS, table[:4], bad, lights[:4], g, 0)
        torch.cuda.synchronize()
        clean = run_camera(pkg, ctx, 32, 32, 3, LR.APERTURE, LR.FOCUS, table[:4], camera[:4], lights[:4], g, (4,))[0]
        got = s.cpu().numpy()
        assert np.isnan(got).any() or (got != clean).any()              # row 2 is another sample, whatever it is


def test_a_capped_grid_changes_nothing(pkg, ctx, Y, monkeypatch):
    """RM_LENS_MAX_BLOCKS = 1 (read at rm_init: a context of its own) caps these kernels' grids too and drives their loop over
    the groups, where the camera's row is fetched."""
    scene = Y.scene("pool")[0]
    GL.upload(ctx, scene)
    table, camera, lights, shapes = library_tables(ctx, Y, "pool", 0, 12)
    free = {bool(g is not None): run_camera(pkg, ctx, 32, 32, 3, LR.APERTURE, LR.FOCUS, table, camera, lights, g, (5, 7)) for g in (None, shapes)}
    monkeypatch.setenv("RM_LENS_MAX_BLOCKS", "1")
    c = pkg.backend.Context(0)
    try:
        c.upload(scene.flatten())
        for g in (None, shapes):
            same(run_camera(pkg, c, 32, 32, 3, LR.APERTURE, LR.FOCUS, table, camera, lights, g, (5, 7)), free[g is not None], "one workgroup")
    finally:
        c.close()


# ---------------------------------------------------------------- 4. the tick
def test_the_tick_continues_begins_again_and_refuses(pkg, ctx, Y):
    L, B = pkg.lib(), pkg._lib
    scene = Y.scene("demo")[0]
    GL.upload(ctx, scene)
    kinds = Y.kinds("demo")
    v = MV.velocities(kinds, MV.SPEED["demo"])
    radii, vel, turn = (1.5, 3.), (4., 0., -2.), (0.2, 0.1, 0.)
    p = pkg.backend.make_params(workloads.FOV, 32., 32., 3)
    table, lights = ctx.lens_sequence(0, 24), ctx.light_sequence(0, 24, radii)
    camera, shapes = ctx.camera_sequence(0, 24, vel, CM.SHUTTER, turn), ctx.motion_sequence(0, 24, v, CM.SHUTTER)
    host, host8 = np.full((32, 32, 3), -3.5), np.full((32, 32, 3), 7, np.uint8)

    def tick(velocity=vel, t=turn, shutter=CM.SHUTTER, vs=None, r=radii, restart=False, **kw):
        return ctx.render_progressive_camera(p, velocity, shutter, LR.APERTURE, LR.FOCUS, 8, t, vs, r, restart, **kw)[1]

    def moving(restart=False, **kw):
        return ctx.render_progressive_moving(p, v, CM.SHUTTER, LR.APERTURE, LR.FOCUS, 8, radii, restart, **kw)[1]

    # three ticks of 8: the frame goes on, and is the device call's over rows [N, N + 8) of the four sequences
    for vs, g in ((None, None), (v, shapes)):
        _, device, device8 = run_camera(pkg, ctx, 32, 32, 3, LR.APERTURE, LR.FOCUS, table, camera, lights, g, (8, 8, 8))
        assert tick(vs=vs, restart=True) == 8 and tick(vs=vs) == 16
        timing, total = ctx.render_progressive_camera(p, vel, CM.SHUTTER, LR.APERTURE, LR.FOCUS, 8, turn, vs, radii, host_rgb=host, host_rgb8=host8)
        assert total == 24 and host.tobytes() == device.tobytes() and host8.tobytes() == device8.tobytes()
        assert timing.kernel_ms > 0. and timing.total_ms >= timing.kernel_ms
    # what begins the frame again, one at a time (each followed by a tick that goes on: 16)
    assert tick(restart=True) == 8 and tick() == 16
    assert tick(velocity=(4., 0., -2.5)) == 8 and tick(velocity=(4., 0., -2.5)) == 16      # a changed velocity
    assert tick() == 8 and tick() == 16
    assert tick(t=(0.2, 0.1, 0.01)) == 8 and tick(t=(0.2, 0.1, 0.01)) == 16                # a changed rate
    assert tick() == 8 and tick() == 16
    assert tick(shutter=0.5) == 8 and tick(shutter=0.5) == 16                              # a changed shutter
    assert tick() == 8 and tick() == 16
    assert tick(vs=v) == 8 and tick(vs=v) == 16                                            # shapes that move are another frame
    assert moving() == 8 and moving() == 16                                                # camera -> moving shapes
    still = np.full((32, 32, 3), -3.5)
    assert moving(host_rgb=still) == 24
    assert still.tobytes() == GV.run_moving(pkg, ctx, 32, 32, 3, LR.APERTURE, LR.FOCUS, table, lights, shapes, (8, 8, 8))[1].tobytes()
    assert tick(vs=v) == 8 and tick(vs=v) == 16                                            # moving shapes -> camera
    assert tick(velocity=(0., 0., 0.), t=(0., 0., 0.), vs=v) == 8                          # a motion of zero is a motion: not the moving shapes' frame
    assert moving() == 8
    assert tick(r=None) == 8 and tick(r=None) == 16                                        # point lights are another frame than radii
    assert tick(restart=True) == 8 and tick() == 16
    # rows == 0: RM_OK, nothing counted, nothing written
    short = pkg.backend.make_params(workloads.FOV, 31., 32., 3)
    host[:] = -3.5
    assert ctx.render_progressive_camera(short, vel, CM.SHUTTER, LR.APERTURE, LR.FOCUS, 8, turn, None, radii, host_rgb=host)[1] == 0 and (host == -3.5).all()
    assert tick() == 24                                                                    # ... and the frame stands
    # refusals leave N and the key alone
    lens = B.rm_lens(LR.APERTURE, LR.FOCUS, 8, 0)
    r64 = np.ascontiguousarray(radii)
    import ctypes as C
    D = C.POINTER(C.c_double)

    def raw(motion, shutter=CM.SHUTTER, vs=None, n_shapes=0, n_lights=2, params=p):
        m = B.rm_camera_motion(B.vec3(motion[:3]), *motion[3:]) if motion is not None else None
        total = C.c_uint32(77)
        st = L.rm_render_progressive_camera(ctx.ptr, C.byref(params), C.byref(lens), r64.ctypes.data_as(D), n_lights,
                                            vs.ctypes.data_as(C.POINTER(B.rm_vec3)) if vs is not None else None, n_shapes, shutter,
                                            C.byref(m) if m is not None else None, 0, None, None, C.byref(total), None)
        assert total.value == 77
        return st, L.rm_last_error(ctx.ptr)

    nan = float("nan")
    good = vel + turn
    for args, text in (((None,), b"NULL motion"), (((nan, 0., 0., 0., 0., 0.),), b"not finite"), (((1., 0., 0., 0., float("inf"), 0.),), b"not finite"),
                       ((good, -1.), b"shutter"), ((good, nan), b"shutter"), ((good, CM.SHUTTER, v, len(kinds) - 1), b"n_shapes"),
                       ((good, CM.SHUTTER, None, 0, 1), b"n_lights")):
        st, err = raw(*args)
        assert st == B.RM_ERR_INVALID_ARG and text in err and b"rm_render_progressive_camera" in err, err
    bad_v = np.array(v)
    bad_v[1, 0] = nan
    st, err = raw(good, CM.SHUTTER, bad_v, len(kinds))
    assert st == B.RM_ERR_INVALID_ARG and b"velocities[1]" in err
    assert tick() == 32                                                                    # ... the frame went on through all of them


def test_a_saturated_frame_stands_and_the_one_shot(pkg, ctx, Y, capsys):
    scene = Y.scene("demo")[0]
    GL.upload(ctx, scene)
    p = pkg.backend.make_params(workloads.FOV, 32., 32., 1)
    vel = (4., 0., -2.)
    n = 0
    first = True
    while n + 64 <= PR.MAX_SAMPLES:
        n = ctx.render_progressive_camera(p, vel, CM.SHUTTER, 0., 1., 64, restart=first)[1]
        first = False
    assert n == PR.MAX_SAMPLES
    host, again = np.zeros((32, 32, 3)), np.zeros((32, 32, 3))
    assert ctx.render_progressive_camera(p, vel, CM.SHUTTER, 0., 1., 1, host_rgb=host)[1] == PR.MAX_SAMPLES
    timing, total = ctx.render_progressive_camera(p, vel, CM.SHUTTER, 0., 1., 64, host_rgb=again)
    assert total == PR.MAX_SAMPLES and timing.kernel_ms == 0. and host.tobytes() == again.tobytes() and host.any()
    # the one-shot: 80 samples in slices of 64 and 16, the device call's frame
    r, fb = pkg.create_renderer(workloads.FOV, 32., 32.), pkg.create_frame_buffer(32, 32)
    r.max_depth = 3
    r.render_camera_blur(fb, scene, vel, CM.SHUTTER, 80, (0.2, 0.1, 0.))
    assert r.last_samples == 80
    c = pkg.backend.default_context(0)
    table, lights = c.lens_sequence(0, 80), np.zeros((80, Y.n_lights("demo"), 3))
    camera = c.camera_sequence(0, 80, vel, CM.SHUTTER, (0.2, 0.1, 0.))
    ref = run_camera(pkg, c, 32, 32, 3, 0., 1., table, camera, lights, None, (16,) * 5)[1]
    assert np.asarray(fb.buffer).reshape(32, 32, 3).tobytes() == ref.tobytes()
    capsys.readouterr()


def test_camera_calls_leave_the_render_state_and_the_counters_alone(pkg, Y):
    """A render, camera calls, the same render: the frames, the uploads and the launch counters of the renders do not know of them."""
    import torch
    scene = Y.scene("demo")[0]
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 3)
    small = pkg.backend.make_params(workloads.FOV, 32., 32., 3)

    def frames(with_calls):
        c = pkg.backend.Context(0)
        try:
            c.upload(scene.flatten())
            out = []
            total = torch.zeros((32, 32, 3), dtype=torch.float64, device="cuda:0")
            for k in range(3):
                a = np.zeros((64, 64, 3))
                c.render(p, a)
                out.append(a)
                if with_calls and k < 2:
                    before = (c.uploads(), c.launch_stats())
                    c.accumulate_camera_device(small, total, LR.APERTURE, LR.FOCUS, c.lens_sequence(2 * k, 2),
                                               c.camera_sequence(2 * k, 2, (4., 0., -2.), 1., (0.1, 0., 0.)), np.zeros((2, 2, 3)), None, 2 * k)
                    torch.cuda.synchronize()
                    host = np.zeros((32, 32, 3))
                    assert c.render_progressive_camera(small, (4., 0., -2.), 1., LR.APERTURE, LR.FOCUS, 4, (0.1, 0., 0.), host_rgb=host)[1] == 4 * (k + 1)
                    assert bool((total != 0.).any()) and host.any()
                    assert (c.uploads(), c.launch_stats()) == before
            return out
        finally:
            c.close()

    plain, mixed = frames(False), frames(True)
    for k, (a, b) in enumerate(zip(plain, mixed)):
        assert a.tobytes() == b.tobytes(), "frame %d differs once camera calls ran" % (k + 1)
