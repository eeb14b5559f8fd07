"""Moving spheres on the GPU (-m gpu): rm_accumulate_motion_device and rm_render_progressive_motion through the C ABI and the
Python bindings, against tests/motion_reference.py -- the lens rays in numpy, row s of every pixel cast by the CPU oracle's
cast_ray against the scene with its sphere centres and its lights moved by row s of the two offset tables, folded in table order
across passes (pinned on the CPU by tests/test_motion_abi.py) -- and against the frames of rm_accumulate_soft_device.

What the header calls byte for byte is demanded byte for byte; against the yardstick every channel of every pixel of the rows
a pass writes is demanded within TIGHT = 1e-9 of the mean (n TIGHT of a sum of n samples), no pixel left out.  Frames are
32 x 32 (32 x 40 and 64 x 32 where rows and patches matter) and a pass casts at most 16 rows."""
import ctypes as C

import numpy as np
import pytest

import lens_reference as LR
import motion_reference as MR
import progressive_reference as PR
import radiance_reference as RR
import soft_reference as SR
import test_gpu_lens as GL
import test_gpu_progressive as GP
import test_gpu_query as GQ
import test_gpu_soft as GS
import variant_matrix as VM
import workloads

pytestmark = pytest.mark.gpu

TIGHT = MR.TIGHT
NAN, BYTE = GP.NAN, GP.BYTE
# scene -> (depth, radii or None for point lights): depth 6 takes the kernels with STACK = 32; the 256 spheres carry a sphere
# hierarchy in the image -- the kernel walks flat, the device order is permuted --; the penumbra scene moves lights and sphere
SCENES = {"demo": (3, None), "penumbra": (3, SR.PENUMBRA_RADII), "synthetic256": (6, None)}
cells = pytest.mark.parametrize("cell", VM.CELLS, ids=VM.cell_id)


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_motion"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return MR.Yardstick(pkg, O, orc)


@pytest.fixture(scope="module")
def matrix(pkg, O, orc):
    return VM.Matrix(pkg, O, orc)


def run_motion(pkg, c, w, h, depth, aperture, focus, table, lights, shapes, sizes, want_mean=True, want_bytes=True):
    """Passes of the sizes `sizes` over consecutive slices of `table` and of both offset tables on torch's current stream, the
    first with n_before = 0, into buffers that held NaN (and BYTE) -> (sum, mean, bytes) as numpy, None for what was not asked."""
    import torch
    p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)
    total = torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda:0")
    mean = torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda:0") if want_mean else None
    rgb8 = torch.full((h, w, 3), BYTE, dtype=torch.uint8, device="cuda:0") if want_bytes else None
    torch.cuda.synchronize()
    done = 0
    assert sum(sizes) == len(table) == len(lights) == len(shapes) and max(sizes) <= 16
    for n in sizes:
        c.accumulate_motion_device(p, total, aperture, focus, np.ascontiguousarray(table[done:done + n]),
                                   np.ascontiguousarray(lights[done:done + n]), np.ascontiguousarray(shapes[done:done + n]), done,
                                   mean=mean, rgb8=rgb8)
        done += n
    torch.cuda.synchronize()
    return (total.cpu().numpy(), mean.cpu().numpy() if want_mean else None, rgb8.cpu().numpy() if want_bytes else None)


def tables(ctx, Y, name, first, n, radii):
    """Rows first .. first + n of the three sequences for the scene: the library's, and the test velocities."""
    lights = ctx.light_sequence(first, n, radii) if radii is not None else np.zeros((n, Y.n_lights(name), 3))
    v = MR.velocities(Y.kinds(name))
    shapes = ctx.motion_sequence(first, n, v, MR.SHUTTER)
    assert shapes.tobytes() == MR.motion_sequence(first, n, v, MR.SHUTTER).tobytes()
    return ctx.lens_sequence(first, n), lights, shapes


def held(got, ref_sum, ref_mean, n, what):
    """The parity demand: nothing NaN, every channel of every pixel within TIGHT (n TIGHT for the sum), bytes by to_bytes."""
    total, mean, rgb8 = got
    assert not np.isnan(mean).any() and not np.isnan(total).any(), what
    d_mean, d_sum = GL.worst(mean, ref_mean), GL.worst(total, ref_sum)
    print("%s: max |delta| mean %.3e, sum %.3e" % (what, d_mean, d_sum))
    assert d_mean < TIGHT and d_sum < n * TIGHT, what
    assert rgb8.tobytes() == PR.to_bytes(mean).tobytes(), what
    return d_mean


# ---------------------------------------------------------------- 1. parity with the yardstick
@pytest.mark.parametrize("name", sorted(SCENES))
def test_motion_frames_match_the_yardstick(pkg, ctx, Y, name):
    """16 rows of the library's sequences through a pinhole (the frames of the non-vacuity pins) and through a lens, and 5 rows
    of a table that is not the library's, with another offset for every row, sphere and light: a swapped sphere, a lane that
    reads another sample's row, or a normal about the stored centre is another picture."""
    depth, radii = SCENES[name]
    GL.upload(ctx, Y.scene(name)[0])
    for aperture in (0., LR.APERTURE):
        table, lights, shapes = tables(ctx, Y, name, 0, 16, radii)
        got = run_motion(pkg, ctx, 32, 32, depth, aperture, LR.FOCUS, table, lights, shapes, (16,))
        ref_sum, ref_mean = Y.motion(name, 32, 32, depth, aperture, LR.FOCUS, table, lights, shapes, (16,))
        held(got, ref_sum, ref_mean, 16, "%s depth %d, 16 rows, aperture %g" % (name, depth, aperture))
        still = Y.soft(name, 32, 32, depth, aperture, LR.FOCUS, table, lights, (16,))[1]
        moved = int((np.abs(ref_mean - still) > 0.05).any(axis=2).sum())
        print("    %d pixels differ from the still frame" % moved)
        assert moved > VM.SHARE * 32 * 32                             # the spheres did move: not the still frame again
        if aperture == 0. and radii is None:
            assert moved == MR.BLURRED[name][2]                       # the frame test_motion_abi.py pins
    rng = np.random.default_rng(20261931)
    table = LR.random_table(rng, 5)
    lights = SR.random_offsets(rng, 5, Y.n_lights(name))
    shapes = MR.random_offsets(rng, 5, Y.n_shapes(name))
    got = run_motion(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table, lights, shapes, (5,))
    ref_sum, ref_mean = Y.motion(name, 32, 32, depth, LR.APERTURE, LR.FOCUS, table, lights, shapes, (5,))
    held(got, ref_sum, ref_mean, 5, "%s depth %d, 5 random rows" % (name, depth))


@cells
def test_every_cell_of_the_variant_matrix(pkg, ctx, matrix, Y, cell):
    """Both powers, both stacks, a sphere hierarchy and a triangle hierarchy in the image: all walked flat."""
    bvh, generic, depth = cell
    pair = matrix.pair(bvh, generic)
    GL.upload(ctx, pair[0])
    name = VM.register(Y, matrix.name(bvh, generic), pair)
    n = MR.CELL_ROWS
    table, lights, shapes = tables(ctx, Y, name, 0, n, None)
    got = run_motion(pkg, ctx, VM.W, VM.H, depth, VM.APERTURE, VM.FOCUS, table, lights, shapes, (3, 5))
    ref_sum, ref_mean = Y.motion(name, VM.W, VM.H, depth, VM.APERTURE, VM.FOCUS, table, lights, shapes, (3, 5))
    held(got, ref_sum, ref_mean, n, "%s, 3 + 5 rows" % VM.cell_id(cell))
    still = Y.soft(name, VM.W, VM.H, depth, VM.APERTURE, VM.FOCUS, table, lights, (3, 5))[1]
    assert int((np.abs(ref_mean - still) > 0.05).any(axis=2).sum()) == MR.BLURRED_CELLS[VM.cell_id(cell)]
    # ... with area lights as well
    lights = ctx.light_sequence(0, n, VM.RADII)
    got = run_motion(pkg, ctx, VM.W, VM.H, depth, VM.APERTURE, VM.FOCUS, table, lights, shapes, (n,))
    ref_sum, ref_mean = Y.motion(name, VM.W, VM.H, depth, VM.APERTURE, VM.FOCUS, table, lights, shapes, (n,))
    held(got, ref_sum, ref_mean, n, "%s, radii %s" % (VM.cell_id(cell), VM.RADII))


def test_oriented_context(pkg, ctx, Y):
    depth, _ = SCENES["demo"]
    scene = Y.scene("demo")[0]
    GL.upload(ctx, scene)
    try:
        lo, hi = GQ.bounds_of(scene.flatten().desc())
        pos, _, _ = ctx.camera()
        eye = np.array([pos.x, pos.y, pos.z]) + np.array([0.12, 0.06, 0.]) * np.linalg.norm(hi - lo)
        ctx.look_at(tuple(eye), tuple((lo + hi) / 2.))
        pos, basis, on = ctx.camera()
        assert on
        view = ((pos.x, pos.y, pos.z), RR.basis_tuple(basis))
        focus = float(np.linalg.norm((lo + hi) / 2. - eye))
        table, lights, shapes = tables(ctx, Y, "demo", 0, 8, (1.5, 3.))
        got = run_motion(pkg, ctx, 32, 32, depth, LR.APERTURE, focus, table, lights, shapes, (4, 4))
        ref_sum, ref_mean = Y.motion("demo", 32, 32, depth, LR.APERTURE, focus, table, lights, shapes, (4, 4), view)
        held(got, ref_sum, ref_mean, 8, "demo from the side, 2 x 4 rows")
        fixed = Y.motion("demo", 32, 32, depth, LR.APERTURE, focus, table, lights, shapes, (4, 4))[1]
        assert GL.worst(ref_mean, fixed) > 0.05                        # ... and it is another picture than the fixed view's
    finally:
        ctx.orient(None)


# ---------------------------------------------------------------- 2. zero shape offsets are the soft frame
@pytest.mark.parametrize("name,depth", [("demo", 3), ("cornell", 3), ("matrix-spheres", 6)])
def test_zero_shape_offsets_are_the_soft_frame_byte_for_byte(pkg, ctx, matrix, Y, name, depth):
    """Two passes of 5 samples: 12 pixels a wave, four idle lanes.  +0. in the first pass, -0. in the second.  The hierarchy cell:
    the soft kernel walks the hierarchy, the motion kernel walks flat, and the bytes are the same."""
    if name == "matrix-spheres":
        pair = matrix.pair("spheres", False)
        name = VM.register(Y, matrix.name("spheres", False), pair)
        scene, aperture, focus = pair[0], VM.APERTURE, VM.FOCUS
    else:
        scene, (aperture, focus) = Y.scene(name)[0], GL.LENS[name]
    GL.upload(ctx, scene)
    table = ctx.lens_sequence(0, 10)
    lights = ctx.light_sequence(0, 10, (1.5,) * Y.n_lights(name))
    zeros = np.zeros((10, Y.n_shapes(name), 3))
    zeros[5:] = -0.
    soft = GS.run_soft(pkg, ctx, 32, 32, depth, aperture, focus, table, lights, (5, 5))
    motion = run_motion(pkg, ctx, 32, 32, depth, aperture, focus, table, lights, zeros, (5, 5))
    for a, b, what in zip(motion, soft, ("sum", "mean", "bytes")):
        assert not (what != "bytes" and np.isnan(a).any())
        assert a.tobytes() == b.tobytes(), "%s: %s differs in %d pixels" % (name, what, int((a != b).any(axis=2).sum()))
    assert soft[1].any()


# ---------------------------------------------------------------- 3. slicing
def test_passes_of_3_5_and_8_rows_are_one_pass_of_16_byte_for_byte(pkg, ctx, Y):
    depth, radii = SCENES["penumbra"]
    GL.upload(ctx, Y.scene("penumbra")[0])
    table, lights, shapes = tables(ctx, Y, "penumbra", 0, 16, radii)
    one = run_motion(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table, lights, shapes, (16,))
    three = run_motion(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table, lights, shapes, (3, 5, 8))
    for a, b, what in zip(three, one, ("sum", "mean", "bytes")):
        assert a.tobytes() == b.tobytes(), what
    assert not np.isnan(one[1]).any()
    # the optional outputs change nothing in the sum
    bare = run_motion(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table, lights, shapes, (3, 5, 8), want_mean=False, want_bytes=False)
    assert bare[0].tobytes() == one[0].tobytes()


# ---------------------------------------------------------------- 4. bookkeeping
def test_rows_below_the_last_patch_row_and_the_memory_behind_the_buffers_keep_their_bytes(pkg, ctx, Y):
    """32 x 40: rows = 32.  The three buffers, their eight last rows and a guard region behind each hold NaN / BYTE beforehand;
    both offset tables are read from allocations of exactly their size and from ones with NaN rows behind them.  The second
    pass continues the first: its mean divides by n_before + n."""
    import torch
    depth, radii = SCENES["penumbra"]
    GL.upload(ctx, Y.scene("penumbra")[0])
    p = pkg.backend.make_params(workloads.FOV, 40., 32., depth)
    n, guard = 40 * 32 * 3, 4096
    table, lights, shapes = tables(ctx, Y, "penumbra", 0, 12, radii)
    ref_sum, ref_mean = Y.motion("penumbra", 32, 40, depth, LR.APERTURE, LR.FOCUS, table, lights, shapes, (7, 5))

    def device(rows_of_table, k, guarded):
        exact = torch.from_numpy(np.ascontiguousarray(rows_of_table)).to("cuda:0")
        if guarded:
            wide = torch.full((k + 64,) + tuple(exact.shape[1:]), NAN, dtype=torch.float64, device="cuda:0")
            wide[:k] = exact
            exact = wide[:k]
        assert exact.is_contiguous()
        return exact

    def run(guarded):
        bufs = [torch.full((n + guard,), NAN, dtype=torch.float64, device="cuda:0"), torch.full((n + guard,), NAN, dtype=torch.float64, device="cuda:0"),
                torch.full((n + guard,), BYTE, dtype=torch.uint8, device="cuda:0")]
        before = [b.cpu().numpy().copy() for b in bufs]
        total, mean, rgb8 = (b[:n].view(40, 32, 3) for b in bufs)
        done = 0
        for k in (7, 5):
            ctx.accumulate_motion_device(p, total, LR.APERTURE, LR.FOCUS, table[done:done + k], device(lights[done:done + k], k, guarded),
                                         device(shapes[done:done + k], k, guarded), done, mean=mean, rgb8=rgb8)
            done += k
        torch.cuda.synchronize()
        after = [b.cpu().numpy() for b in bufs]
        for a, b in zip(after, before):
            assert a[32 * 32 * 3:].tobytes() == b[32 * 32 * 3:].tobytes()  # rows 32-39 and the guard, bit for bit
        return [a[:n].reshape(40, 32, 3)[:32] for a in after]

    got = run(False)
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()      # no pixel of [0, rows) left unwritten
    assert GL.worst(got[0], ref_sum[:32]) < 12 * TIGHT and GL.worst(got[1], ref_mean[:32]) < TIGHT
    assert got[2].tobytes() == PR.to_bytes(got[1]).tobytes()
    for a, b, what in zip(run(True), got, ("sum", "mean", "bytes")):
        assert a.tobytes() == b.tobytes(), "NaN rows behind the offset tables changed the %s" % what
    # the host path copies the rows [0, 32) only
    v = MR.velocities(Y.kinds("penumbra"))
    host, host8 = np.full((40, 32, 3), -3.5), np.full((40, 32, 3), 7, np.uint8)
    ctx.render_progressive_motion(p, v, MR.SHUTTER, LR.APERTURE, LR.FOCUS, 7, radii, restart=True, host_rgb=host, host_rgb8=host8)
    _, n_total = ctx.render_progressive_motion(p, v, MR.SHUTTER, LR.APERTURE, LR.FOCUS, 5, radii, host_rgb=host, host_rgb8=host8)
    assert n_total == 12
    assert host[:32].tobytes() == got[1].tobytes() and np.all(host[32:] == -3.5)
    assert host8[:32].tobytes() == got[2].tobytes() and np.all(host8[32:] == 7)


def test_motion_calls_leave_the_render_state_alone(pkg, Y):
    import torch
    demo = workloads.product_scene(pkg, "demo")
    v = MR.velocities(Y.kinds("demo"))
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 5)
    wide = pkg.backend.make_params(workloads.FOV, 32., 64., 5)           # 64 x 32: two patches a row

    def frames(with_motion):
        c = pkg.backend.Context(0)
        try:
            c.upload(demo.flatten())
            out = []
            if with_motion:
                total = torch.zeros((32, 64, 3), dtype=torch.float64, device="cuda:0")
                rgb8 = torch.zeros((32, 64, 3), dtype=torch.uint8, device="cuda:0")
            for k in range(3):
                f = np.zeros((64, 64, 3))
                c.render(p, f)
                out.append(f)
                if with_motion and k < 2:                            # before, between and after: motion calls behind frames 1 and 2
                    before = (c.uploads(), c.launch_stats())
                    c.accumulate_motion_device(wide, total, LR.APERTURE, LR.FOCUS, c.lens_sequence(2 * k, 2), np.zeros((2, 2, 3)),
                                               c.motion_sequence(2 * k, 2, v, MR.SHUTTER), 2 * k, rgb8=rgb8)
                    torch.cuda.synchronize()
                    host = np.zeros((32, 64, 3))
                    assert c.render_progressive_motion(wide, v, MR.SHUTTER, LR.APERTURE, LR.FOCUS, 4, host_rgb=host)[1] == 4 * (k + 1)
                    assert bool((total != 0.).any()) and bool((rgb8 != 0).any()) and host.any()
                    assert (c.uploads(), c.launch_stats()) == before
            return out
        finally:
            c.close()

    plain, ticked = frames(False), frames(True)
    for k, (a, b) in enumerate(zip(plain, ticked)):
        assert a.tobytes() == b.tobytes(), "frame %d differs once motion calls ran" % (k + 1)


# ---------------------------------------------------------------- 5. the tick
def test_the_tick_continues_begins_again_and_refuses(pkg, ctx, Y, capsys):
    L, B = pkg.lib(), pkg._lib
    depth = 3
    scene = Y.scene("demo")[0]
    GL.upload(ctx, scene)
    kinds = Y.kinds("demo")
    v = MR.velocities(kinds)
    radii = (1.5, 3.)
    table, lights, shapes = tables(ctx, Y, "demo", 0, 24, radii)
    _, device, device8 = run_motion(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table, lights, shapes, (8, 8, 8))
    ref_mean = Y.motion("demo", 32, 32, depth, LR.APERTURE, LR.FOCUS, table, lights, shapes, (8, 8, 8))[1]
    assert GL.worst(device, ref_mean) < TIGHT                         # rows [N, N + 8) of the three sequences, tick after tick
    p = pkg.backend.make_params(workloads.FOV, 32., 32., depth)
    host, host8 = np.full((32, 32, 3), -3.5), np.full((32, 32, 3), 7, np.uint8)

    def motion(vel=v, shutter=MR.SHUTTER, r=radii, restart=False, **kw):
        return ctx.render_progressive_motion(p, vel, shutter, LR.APERTURE, LR.FOCUS, 8, r, restart, **kw)[1]

    def soft(restart=False, **kw):
        return ctx.render_progressive_soft(p, radii, LR.APERTURE, LR.FOCUS, 8, restart, **kw)[1]

    # three ticks of 8 with the same arguments: the frame goes on, and is the device call's
    assert motion(restart=True) == 8 and motion() == 16
    timing, total = ctx.render_progressive_motion(p, v, MR.SHUTTER, LR.APERTURE, LR.FOCUS, 8, radii, host_rgb=host, host_rgb8=host8)
    assert total == 24 and host.tobytes() == device.tobytes() and host8.tobytes() == device8.tobytes()
    assert timing.kernel_ms > 0. and timing.total_ms >= timing.kernel_ms
    # what begins the frame again, one at a time (each followed by a tick that goes on: 16)
    faster = v * 1.5
    assert motion(vel=faster) == 8 and motion(vel=faster) == 16       # a changed velocity
    assert motion() == 8 and motion() == 16                           # ... and back
    assert motion(shutter=0.5) == 8 and motion(shutter=0.5) == 16     # a changed shutter
    assert motion() == 8 and motion() == 16
    assert soft() == 8 and soft() == 16                               # motion -> soft
    still = np.full((32, 32, 3), -3.5)
    assert soft(host_rgb=still) == 24
    assert still.tobytes() == GS.run_soft(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table, lights, (8, 8, 8))[1].tobytes()
    assert motion() == 8 and motion() == 16                           # soft -> motion
    assert ctx.render_progressive(p, LR.APERTURE, LR.FOCUS, 8)[1] == 8   # motion -> plain
    assert motion() == 8                                              # plain -> motion
    assert motion(r=None) == 8 and motion(r=None) == 16               # point lights are another frame than radii
    assert motion(vel=v * 0.) == 8                                    # velocities of zero are velocities: not the soft call's frame
    assert soft() == 8
    assert motion(restart=True) == 8 and motion() == 16               # restart
    again = np.full((32, 32, 3), -3.5)
    assert motion(host_rgb=again) == 24 and again.tobytes() == device.tobytes()
    # a refused call in between changes neither the count nor the key: a velocity on the floor, the shape named
    polygon = kinds.index(1)
    D = C.POINTER(C.c_double)
    lens, r64 = B.rm_lens(LR.APERTURE, LR.FOCUS, 8, 0), np.ascontiguousarray(radii, dtype=np.float64)
    for bad, n_shapes, word in ((None, len(v), "shape %d is not a sphere" % polygon), (v[:-1], len(v) - 1, "n_shapes"),
                                (np.where(np.arange(len(v))[:, None] == 0, NAN, v), len(v), "velocities[0]")):
        if bad is None:
            bad = v.copy()
            bad[polygon] = (0., 1e-300, 0.)
        bad = np.ascontiguousarray(bad)
        n_total, before = C.c_uint32(77), again.copy()
        st = L.rm_render_progressive_motion(ctx.ptr, C.byref(p), C.byref(lens), r64.ctypes.data_as(D), 2, bad.ctypes.data_as(C.POINTER(B.rm_vec3)),
                                            n_shapes, MR.SHUTTER, 0, again.ctypes.data_as(D), None, C.byref(n_total), None)
        assert st == B.RM_ERR_INVALID_ARG and n_total.value == 77 and again.tobytes() == before.tobytes()
        assert word in L.rm_last_error(ctx.ptr).decode(), L.rm_last_error(ctx.ptr)
    for shutter in (-1e-9, NAN, float("inf")):
        n_total = C.c_uint32(77)
        st = L.rm_render_progressive_motion(ctx.ptr, C.byref(p), C.byref(lens), r64.ctypes.data_as(D), 2, v.ctypes.data_as(C.POINTER(B.rm_vec3)),
                                            len(v), shutter, 0, again.ctypes.data_as(D), None, C.byref(n_total), None)
        assert st == B.RM_ERR_INVALID_ARG and n_total.value == 77 and b"shutter" in L.rm_last_error(ctx.ptr)
    with pytest.raises(B.BackendError, match="is not a sphere"):
        moving_floor = v.copy()
        moving_floor[polygon] = (1., 0., 0.)
        motion(vel=moving_floor)
    assert motion() == 32                                             # ... the frame went through all that untouched
    # -0. on a polygon is zero
    resting = v.copy()
    resting[polygon] = (-0., 0., -0.)
    assert motion(vel=resting, restart=True) == 8
    # Renderer.render_progressive_motion and render_motion_blur: the prints and the return value of render()
    r = pkg.create_renderer(workloads.FOV, 32., 32.)
    r.max_depth = depth
    fb = pkg.create_frame_buffer(32, 32)
    vel = [pkg.Vec3f(*e) if k == MR.ORC_SPHERE else None for e, k in zip(v, kinds)]
    capsys.readouterr()
    message = r.render_progressive_motion(fb, scene, vel, MR.SHUTTER, 8, radii, LR.APERTURE, LR.FOCUS, restart=True)
    out = capsys.readouterr().out
    assert message.startswith("Scene rendered in ") and message in out and "compute units used" in out
    assert r.last_samples == 8 and r.last_timing.kernel_ms > 0.
    r.render_progressive_motion(fb, scene, vel, MR.SHUTTER, 8, radii, LR.APERTURE, LR.FOCUS)
    r.render_progressive_motion(fb, scene, vel, MR.SHUTTER, 8, radii, LR.APERTURE, LR.FOCUS)
    assert r.last_samples == 24 and fb.buffer.tobytes() == device.tobytes()
    # the one-shot: 80 samples in slices of 64 and 16, through a pinhole, point lights
    r.render_motion_blur(fb, scene, vel, MR.SHUTTER, 80)
    assert r.last_samples == 80
    t80, l80, s80 = tables(ctx, Y, "demo", 0, 80, None)
    blur = run_motion(pkg, ctx, 32, 32, depth, 0., 1., t80, l80, s80, (16,) * 5)[1]      # (a left fold: however the passes are sliced)
    assert fb.buffer.tobytes() == blur.tobytes()


def test_a_saturated_frame_stands(pkg, ctx, Y):
    """1,024 ticks of 64 fill the frame to RM_PROGRESSIVE_MAX_SAMPLES; the next tick launches nothing and returns it as it stands."""
    GL.upload(ctx, Y.scene("demo")[0])
    v = MR.velocities(Y.kinds("demo"))
    p = pkg.backend.make_params(workloads.FOV, 32., 32., 3)
    assert ctx.render_progressive_motion(p, v, MR.SHUTTER, 0., LR.FOCUS, 64, restart=True)[1] == 64
    for k in range(2, 1024):
        total = ctx.render_progressive_motion(p, v, MR.SHUTTER, 0., LR.FOCUS, 64)[1]
    assert total == 65472
    before, before8 = np.full((32, 32, 3), NAN), np.full((32, 32, 3), BYTE, np.uint8)
    assert ctx.render_progressive_motion(p, v, MR.SHUTTER, 0., LR.FOCUS, 64, host_rgb=before, host_rgb8=before8)[1] == 65536 == MR.MAX_SAMPLES
    assert not np.isnan(before).any() and before8.tobytes() == PR.to_bytes(before).tobytes()
    for n in (64, 1):
        after, after8 = np.full((32, 32, 3), NAN), np.full((32, 32, 3), BYTE, np.uint8)
        timing, total = ctx.render_progressive_motion(p, v, MR.SHUTTER, 0., LR.FOCUS, n, host_rgb=after, host_rgb8=after8)
        assert total == 65536 and timing.kernel_ms == 0.
        assert after.tobytes() == before.tobytes() and after8.tobytes() == before8.tobytes()
    assert ctx.render_progressive_motion(p, v, MR.SHUTTER, 0., LR.FOCUS, 64, restart=True)[1] == 64


# ---------------------------------------------------------------- 6. refusals and the grid
def test_refusals_of_the_device_call_leave_the_buffers_alone(pkg, ctx, Y):
    import torch
    L, B = pkg.lib(), pkg._lib
    depth = 3
    GL.upload(ctx, Y.scene("demo")[0])
    n_shapes = Y.n_shapes("demo")
    p = pkg.backend.make_params(workloads.FOV, 64., 64., depth)
    total = torch.full((64, 64, 3), 7.25, dtype=torch.float64, device="cuda:0")
    mean = torch.full((64, 64, 3), 7.25, dtype=torch.float64, device="cuda:0")
    rgb8 = torch.full((64, 64, 3), 7, dtype=torch.uint8, device="cuda:0")
    table = torch.from_numpy(PR.lens_sequence(0, 4)).to("cuda:0")
    lights = torch.zeros((4, 2, 3), dtype=torch.float64, device="cuda:0")
    shapes = torch.from_numpy(MR.motion_sequence(0, 4, MR.velocities(Y.kinds("demo")), 1.)).to("cuda:0")
    good = B.rm_lens(LR.APERTURE, LR.FOCUS, 4, 0)

    def untouched():
        torch.cuda.synchronize()
        return bool((total == 7.25).all()) and bool((mean == 7.25).all()) and bool((rgb8 == 7).all())

    def device_call(lens=good, t=table, o=lights, n_lights=2, so=shapes, ns=n_shapes, s=total, m=mean, n_before=4, params=p):
        vp = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
        st = L.rm_accumulate_motion_device(ctx.ptr, C.byref(params), C.byref(lens), vp(t), vp(o), n_lights, vp(so), ns, n_before, vp(s), vp(m),
                                           vp(rgb8), None)
        msg = L.rm_last_error(ctx.ptr).decode()
        assert st != 0 and untouched(), msg
        return st, msg

    E = B.RM_ERR_INVALID_ARG
    # the moving spheres' own
    for ns in (0, n_shapes - 1, n_shapes + 1, 2 ** 32 - 1):
        st, msg = device_call(ns=ns)
        assert st == E and "n_shapes" in msg and "the resident scene has %d" % n_shapes in msg
    st, msg = device_call(so=None)
    assert st == E and "NULL shape offsets" in msg
    # the area lights' own
    for n_lights in (0, 1, 3, 2 ** 32 - 1):
        st, msg = device_call(n_lights=n_lights)
        assert st == E and "n_lights" in msg and "the resident scene has 2" in msg
    st, msg = device_call(o=None)
    assert st == E and "NULL light offsets" in msg
    # the progressive frames' own, through the new entry point
    st, msg = device_call(t=None)
    assert st == E and "table" in msg
    st, msg = device_call(s=None)
    assert st == E and "sum" in msg
    st, msg = device_call(m=total)
    assert st == E and "device_mean == device_sum" in msg
    for n_before, n in ((65533, 4), (65536, 1), (2 ** 32 - 1, 64)):
        st, msg = device_call(lens=B.rm_lens(LR.APERTURE, LR.FOCUS, n, 0), n_before=n_before)
        assert st == E and "n_before + n_samples" in msg, msg
    for lens, word in ((B.rm_lens(-1., LR.FOCUS, 4, 0), "aperture"), (B.rm_lens(LR.APERTURE, 0., 4, 0), "focus"), (B.rm_lens(LR.APERTURE, LR.FOCUS, 65, 0), "n_samples")):
        st, msg = device_call(lens=lens)
        assert st == E and word in msg
    odd = pkg.backend.make_params(workloads.FOV, 64., 100., depth)
    assert device_call(params=odd)[0] == B.RM_ERR_DIMENSIONS
    fresh = pkg.backend.Context(0)
    try:
        vp = lambda x: C.c_void_p(x.data_ptr())
        assert L.rm_accumulate_motion_device(fresh.ptr, C.byref(p), C.byref(good), vp(table), vp(lights), 2, vp(shapes), n_shapes, 0, vp(total),
                                             vp(mean), vp(rgb8), None) == B.RM_ERR_NO_SCENE
        n_total = C.c_uint32(77)
        v = np.zeros((n_shapes, 3))
        assert L.rm_render_progressive_motion(fresh.ptr, C.byref(p), C.byref(good), None, 0, v.ctypes.data_as(C.POINTER(B.rm_vec3)), n_shapes, 1., 0,
                                              None, None, C.byref(n_total), None) == B.RM_ERR_NO_SCENE and n_total.value == 77
    finally:
        fresh.close()
    assert untouched()
    # what is tolerated: a frame without a whole patch row; a scene without a sphere and a NULL shape table
    short = run_motion(pkg, ctx, 64, 31, depth, LR.APERTURE, LR.FOCUS, PR.lens_sequence(0, 4), np.zeros((4, 2, 3)), np.zeros((4, n_shapes, 3)), (4,))
    assert np.isnan(short[0]).all() and np.isnan(short[1]).all() and np.all(short[2] == BYTE)   # rows == 0: RM_OK, nothing done
    GL.upload(ctx, Y.scene("cornell")[0])
    nc, lc = Y.n_shapes("cornell"), Y.n_lights("cornell")
    small = pkg.backend.make_params(workloads.FOV, 32., 32., depth)
    aperture, focus = GL.LENS["cornell"]
    t4 = torch.from_numpy(PR.lens_sequence(0, 4)).to("cuda:0")
    l4 = torch.zeros((4, lc, 3), dtype=torch.float64, device="cuda:0")
    s32, m32 = (torch.full((32, 32, 3), NAN, dtype=torch.float64, device="cuda:0") for _ in range(2))
    lens = B.rm_lens(aperture, focus, 4, 0)
    assert L.rm_accumulate_motion_device(ctx.ptr, C.byref(small), C.byref(lens), C.c_void_p(t4.data_ptr()), C.c_void_p(l4.data_ptr()), lc, None, nc, 0,
                                         C.c_void_p(s32.data_ptr()), C.c_void_p(m32.data_ptr()), None, None) == 0
    torch.cuda.synchronize()
    soft = GS.run_soft(pkg, ctx, 32, 32, depth, aperture, focus, PR.lens_sequence(0, 4), np.zeros((4, lc, 3)), (4,))
    assert m32.cpu().numpy().tobytes() == soft[1].tobytes() and not np.isnan(soft[1]).any()


def test_a_capped_grid_changes_nothing(pkg, ctx, Y, monkeypatch):
    """RM_LENS_MAX_BLOCKS = 1 (read at rm_init: a context of its own) caps this kernel's grid too and drives its loop over the
    groups and its tail; 64 x 32: two patches a row."""
    depth, radii = SCENES["penumbra"]
    scene = Y.scene("penumbra")[0]
    GL.upload(ctx, scene)
    table, lights, shapes = tables(ctx, Y, "penumbra", 0, 24, radii)
    plans = ((1, 1), (5, 7), (16, 8))
    free = {s: run_motion(pkg, ctx, 64, 32, depth, LR.APERTURE, LR.FOCUS, table[:sum(s)], lights[:sum(s)], shapes[:sum(s)], s) for s in plans}
    monkeypatch.setenv("RM_LENS_MAX_BLOCKS", "1")
    c = pkg.backend.Context(0)
    try:
        c.upload(scene.flatten())
        for s in plans:
            got = run_motion(pkg, c, 64, 32, depth, LR.APERTURE, LR.FOCUS, table[:sum(s)], lights[:sum(s)], shapes[:sum(s)], s)
            for a, b, what in zip(got, free[s], ("sum", "mean", "bytes")):
                assert a.tobytes() == b.tobytes(), "1 workgroup, passes %s: %s" % (s, what)
    finally:
        c.close()
    assert not np.isnan(free[(16, 8)][1]).any()
