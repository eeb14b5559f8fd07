"""Moving shapes on the GPU (-m gpu): rm_accumulate_moving_device and rm_render_progressive_moving through the C ABI and the Python
bindings, against tests/moving_reference.py -- the lens rays in numpy, row s of every pixel cast by the CPU oracle's cast_ray
against the scene with its spheres, polygons, meshes and lights moved by row s of the two offset tables, folded in table order
across passes (pinned on the CPU by tests/test_moving_abi.py) -- and against the frames of rm_accumulate_motion_device.

What the header calls byte for byte is demanded byte for byte; against the yardstick every channel of every pixel of the rows a
pass writes is demanded within TIGHT = 1e-9 of the mean (n TIGHT of a sum of n samples), no pixel left out.  Frames are 32 x 32
(32 x 40 and 64 x 32 where rows and patches matter) and a pass casts at most 16 rows."""
import ctypes as C

import numpy as np
import pytest

import lens_reference as LR
import motion_reference as MR
import moving_reference as MV
import progressive_reference as PR
import radiance_reference as RR
import soft_reference as SR
import test_gpu_lens as GL
import test_gpu_motion as GM
import test_gpu_progressive as GP
import test_gpu_query as GQ
import variant_matrix as VM
import workloads

pytestmark = pytest.mark.gpu

TIGHT = MV.TIGHT
NAN, BYTE = GP.NAN, GP.BYTE
# scene -> (depth, radii or None for point lights, (aperture, focus) of the lens frames): the demo's floor and spheres move and
# the shadows on the moving floor change; every Obj of the Cornell box and the dodecahedron moves; the pool scene's pentagon and
# hexagon read their last vertices from the vertex pool; the 256 spheres carry a sphere hierarchy in the image, so the device
# order of the spheres is permuted, and depth 6 takes the kernels with STACK = 32
SCENES = {"demo": (3, None, (LR.APERTURE, LR.FOCUS)), "cornell": (3, None, GL.LENS["cornell"]), "dodecahedron": (3, None, GL.LENS["cornell"]),
          "pool": (3, SR.PENUMBRA_RADII, (LR.APERTURE, LR.FOCUS)), "synthetic256": (6, None, (LR.APERTURE, LR.FOCUS))}
cells = pytest.mark.parametrize("cell", VM.CELLS, ids=VM.cell_id)
held = GM.held


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_moving"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return MV.Yardstick(pkg, O, orc)


@pytest.fixture(scope="module")
def matrix(pkg, O, orc):
    return VM.Matrix(pkg, O, orc)


def run_moving(pkg, c, w, h, depth, aperture, focus, table, lights, shapes, sizes, want_mean=True, want_bytes=True, call="accumulate_moving_device"):
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
        getattr(c, call)(p, total, aperture, focus, np.ascontiguousarray(table[done:done + n]), np.ascontiguousarray(lights[done:done + n]),
                         np.ascontiguousarray(shapes[done:done + n]), done, mean=mean, rgb8=rgb8)
        done += n
    torch.cuda.synchronize()
    return (total.cpu().numpy(), mean.cpu().numpy() if want_mean else None, rgb8.cpu().numpy() if want_bytes else None)


def velocities_of(Y, name, only=None):
    return MV.velocities(Y.kinds(name), MV.SPEED.get(name, MV.CELL_SPEED), only)


def tables(ctx, Y, name, first, n, radii, only=None):
    """Rows first .. first + n of the three sequences for the scene: the library's, and the test velocities."""
    lights = ctx.light_sequence(first, n, radii) if radii is not None else np.zeros((n, Y.n_lights(name), 3))
    v = velocities_of(Y, name, only)
    shapes = ctx.motion_sequence(first, n, v, MV.SHUTTER)
    assert shapes.tobytes() == MR.motion_sequence(first, n, v, MV.SHUTTER).tobytes()
    return ctx.lens_sequence(first, n), lights, shapes


def same(a, b, what):
    for x, y, part in zip(a, b, ("sum", "mean", "bytes")):
        assert not (part != "bytes" and np.isnan(x).any()), "%s: %s" % (what, part)
        assert x.tobytes() == y.tobytes(), "%s: %s differs in %d pixels" % (what, part, int((x != y).any(axis=2).sum()))


# ---------------------------------------------------------------- 1. parity with the yardstick
@pytest.mark.parametrize("name", sorted(SCENES))
def test_moving_frames_match_the_yardstick(pkg, ctx, Y, name):
    """16 rows of the library's sequences through a pinhole (the frames of the non-vacuity pins) and through a lens, and 5 rows
    of a table that is not the library's, with another offset for every row, shape and light: a polygon moved by another
    shape's row, a vertex left where it was, a numerator from the stored plane point or a lane that reads another sample's row
    is another picture."""
    depth, radii, (aperture, focus) = SCENES[name]
    GL.upload(ctx, Y.scene(name)[0])
    kinds = Y.kinds(name)
    for a in (0., aperture):
        table, lights, shapes = tables(ctx, Y, name, 0, 16, radii)
        got = run_moving(pkg, ctx, 32, 32, depth, a, focus, table, lights, shapes, (16,))
        ref_sum, ref_mean = Y.moving(name, 32, 32, depth, a, focus, table, lights, shapes, (16,))
        held(got, ref_sum, ref_mean, 16, "%s depth %d, 16 rows, aperture %g" % (name, depth, a))
        if a == 0. and radii is None:
            spheres = Y.motion(name, 32, 32, depth, 0., focus, table, lights, MV.spheres_only(shapes, kinds), (16,))[1]
            moved = int((np.abs(ref_mean - spheres) > 0.05).any(axis=2).sum())
            print("    %d pixels differ from the frame with only the spheres moving" % moved)
            assert moved == MV.BLURRED[name][2] > VM.SHARE * 32 * 32   # the frame test_moving_abi.py pins (a pinhole has no focus)
    rng = np.random.default_rng(20261951)
    table = LR.random_table(rng, 5)
    lights = SR.random_offsets(rng, 5, Y.n_lights(name))
    shapes = MV.random_offsets(rng, 5, kinds, MV.SPEED[name] / 3.)
    got = run_moving(pkg, ctx, 32, 32, depth, aperture, focus, table, lights, shapes, (5,))
    ref_sum, ref_mean = Y.moving(name, 32, 32, depth, aperture, focus, table, lights, shapes, (5,))
    held(got, ref_sum, ref_mean, 5, "%s depth %d, 5 random rows" % (name, depth))


def test_one_mesh_of_the_cornell_box_moves_and_the_others_stand_still(pkg, ctx, Y):
    """Triangles of different shapes read different rows: the mover's alone are not zero."""
    depth, _, (aperture, focus) = SCENES["cornell"]
    GL.upload(ctx, Y.scene("cornell")[0])
    for a, f in ((0., LR.FOCUS), (aperture, focus)):
        table, lights, shapes = tables(ctx, Y, "cornell", 0, 16, None, MV.CORNELL_MOVER)
        assert list(np.flatnonzero((shapes != 0.).any(axis=(0, 2)))) == [MV.CORNELL_MOVER]
        got = run_moving(pkg, ctx, 32, 32, depth, a, f, table, lights, shapes, (16,))
        ref_sum, ref_mean = Y.moving("cornell", 32, 32, depth, a, f, table, lights, shapes, (16,))
        held(got, ref_sum, ref_mean, 16, "cornell, Obj %d moves, aperture %g" % (MV.CORNELL_MOVER, a))
        if a == 0.:
            still = Y.motion("cornell", 32, 32, depth, a, f, table, lights, np.zeros_like(shapes), (16,))[1]
            assert int((np.abs(ref_mean - still) > 0.05).any(axis=2).sum()) == MV.BLURRED["cornell-one"][2]


@cells
def test_every_cell_of_the_variant_matrix(pkg, ctx, matrix, Y, cell):
    """Both powers, both stacks, a sphere hierarchy and a triangle hierarchy in the image, all walked flat: the glass panes move,
    so refracted and reflected children go through moved quads; the mesh cell's triangles are permuted by its hierarchy."""
    bvh, generic, depth = cell
    pair = matrix.pair(bvh, generic)
    GL.upload(ctx, pair[0])
    name = VM.register(Y, matrix.name(bvh, generic), pair)
    n = MV.CELL_ROWS
    table, lights, shapes = tables(ctx, Y, name, 0, n, None)
    got = run_moving(pkg, ctx, VM.W, VM.H, depth, VM.APERTURE, VM.FOCUS, table, lights, shapes, (3, 5))
    ref_sum, ref_mean = Y.moving(name, VM.W, VM.H, depth, VM.APERTURE, VM.FOCUS, table, lights, shapes, (3, 5))
    held(got, ref_sum, ref_mean, n, "%s, 3 + 5 rows" % VM.cell_id(cell))
    spheres = Y.motion(name, VM.W, VM.H, depth, VM.APERTURE, VM.FOCUS, table, lights, MV.spheres_only(shapes, Y.kinds(name)), (3, 5))[1]
    assert int((np.abs(ref_mean - spheres) > 0.05).any(axis=2).sum()) == MV.BLURRED_CELLS[VM.cell_id(cell)]
    # ... with area lights as well
    lights = ctx.light_sequence(0, n, VM.RADII)
    got = run_moving(pkg, ctx, VM.W, VM.H, depth, VM.APERTURE, VM.FOCUS, table, lights, shapes, (n,))
    ref_sum, ref_mean = Y.moving(name, VM.W, VM.H, depth, VM.APERTURE, VM.FOCUS, table, lights, shapes, (n,))
    held(got, ref_sum, ref_mean, n, "%s, radii %s" % (VM.cell_id(cell), VM.RADII))


def test_oriented_context(pkg, ctx, Y):
    depth = SCENES["demo"][0]
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
        got = run_moving(pkg, ctx, 32, 32, depth, LR.APERTURE, focus, table, lights, shapes, (4, 4))
        ref_sum, ref_mean = Y.moving("demo", 32, 32, depth, LR.APERTURE, focus, table, lights, shapes, (4, 4), view)
        held(got, ref_sum, ref_mean, 8, "demo from the side, 2 x 4 rows")
        fixed = Y.moving("demo", 32, 32, depth, LR.APERTURE, focus, table, lights, shapes, (4, 4))[1]
        assert GL.worst(ref_mean, fixed) > 0.05                        # ... and it is another picture than the fixed view's
    finally:
        ctx.orient(None)


# ---------------------------------------------------------------- 2. what the header calls byte for byte
@pytest.mark.parametrize("name,depth", [("demo", 3), ("cornell", 3), ("matrix-mesh", 5), ("matrix-spheres", 6)])
def test_zero_rows_are_the_moving_spheres_pass_byte_for_byte(pkg, ctx, matrix, Y, name, depth):
    """Two passes of 5 samples: 12 pixels a wave, four idle lanes.  (a) every offset zero, +0. in the first pass and -0. in the
    second, against rm_accumulate_motion_device with the same zeros; (b) the test velocities' rows for the spheres and zero rows
    for every other shape, against the moving spheres' pass with those rows."""
    if name.startswith("matrix-"):
        bvh = name.split("-")[1]
        pair = matrix.pair(bvh, False)
        name = VM.register(Y, matrix.name(bvh, False), pair)
        scene, aperture, focus = pair[0], VM.APERTURE, VM.FOCUS
    else:
        scene, (aperture, focus) = Y.scene(name)[0], SCENES[name][2]
    GL.upload(ctx, scene)
    kinds = Y.kinds(name)
    table = ctx.lens_sequence(0, 10)
    lights = ctx.light_sequence(0, 10, (1.5,) * Y.n_lights(name))
    zeros = np.zeros((10, len(kinds), 3))
    zeros[5:] = -0.
    only = MV.spheres_only(ctx.motion_sequence(0, 10, velocities_of(Y, name), MV.SHUTTER), kinds)
    for shapes, what in ((zeros, "zero offsets"), (only, "zero rows but the spheres'")):
        motion = GM.run_motion(pkg, ctx, 32, 32, depth, aperture, focus, table, lights, shapes, (5, 5))
        moving = run_moving(pkg, ctx, 32, 32, depth, aperture, focus, table, lights, shapes, (5, 5))
        same(moving, motion, "%s, %s" % (name, what))
        assert motion[1].any()
    if MV.ORC_SPHERE in kinds:
        assert (only != 0.).any()


# ---------------------------------------------------------------- 3. slicing
def test_passes_of_3_5_and_8_rows_are_one_pass_of_16_byte_for_byte(pkg, ctx, Y):
    depth, radii, (aperture, focus) = SCENES["pool"]
    GL.upload(ctx, Y.scene("pool")[0])
    table, lights, shapes = tables(ctx, Y, "pool", 0, 16, radii)
    one = run_moving(pkg, ctx, 32, 32, depth, aperture, focus, table, lights, shapes, (16,))
    three = run_moving(pkg, ctx, 32, 32, depth, aperture, focus, table, lights, shapes, (3, 5, 8))
    same(three, one, "3 + 5 + 8")
    bare = run_moving(pkg, ctx, 32, 32, depth, aperture, focus, table, lights, shapes, (3, 5, 8), want_mean=False, want_bytes=False)
    assert bare[0].tobytes() == one[0].tobytes()                      # the optional outputs change nothing in the sum


# ---------------------------------------------------------------- 4. bookkeeping
def test_rows_below_the_last_patch_row_and_the_memory_behind_the_buffers_keep_their_bytes(pkg, ctx, Y):
    """32 x 40: rows = 32.  The three buffers, their eight last rows and a guard region behind each hold NaN / BYTE beforehand;
    both offset tables are read from allocations of exactly their size and from ones with NaN rows behind them.  The second
    pass continues the first: its mean divides by n_before + n."""
    import torch
    depth, radii, (aperture, focus) = SCENES["pool"]
    GL.upload(ctx, Y.scene("pool")[0])
    p = pkg.backend.make_params(workloads.FOV, 40., 32., depth)
    n, guard = 40 * 32 * 3, 4096
    table, lights, shapes = tables(ctx, Y, "pool", 0, 12, radii)
    ref_sum, ref_mean = Y.moving("pool", 32, 40, depth, aperture, focus, table, lights, shapes, (7, 5))

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
            ctx.accumulate_moving_device(p, total, aperture, focus, table[done:done + k], device(lights[done:done + k], k, guarded),
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
    v = velocities_of(Y, "pool")
    host, host8 = np.full((40, 32, 3), -3.5), np.full((40, 32, 3), 7, np.uint8)
    ctx.render_progressive_moving(p, v, MV.SHUTTER, aperture, focus, 7, radii, restart=True, host_rgb=host, host_rgb8=host8)
    _, n_total = ctx.render_progressive_moving(p, v, MV.SHUTTER, aperture, focus, 5, radii, host_rgb=host, host_rgb8=host8)
    assert n_total == 12
    assert host[:32].tobytes() == got[1].tobytes() and np.all(host[32:] == -3.5)
    assert host8[:32].tobytes() == got[2].tobytes() and np.all(host8[32:] == 7)


def test_moving_calls_leave_the_render_state_alone(pkg, Y):
    import torch
    demo = workloads.product_scene(pkg, "demo")
    v = velocities_of(Y, "demo")
    p = pkg.backend.make_params(workloads.FOV, 64., 64., 5)
    wide = pkg.backend.make_params(workloads.FOV, 32., 64., 5)           # 64 x 32: two patches a row

    def frames(with_moving):
        c = pkg.backend.Context(0)
        try:
            c.upload(demo.flatten())
            out = []
            if with_moving:
                total = torch.zeros((32, 64, 3), dtype=torch.float64, device="cuda:0")
                rgb8 = torch.zeros((32, 64, 3), dtype=torch.uint8, device="cuda:0")
            for k in range(3):
                f = np.zeros((64, 64, 3))
                c.render(p, f)
                out.append(f)
                if with_moving and k < 2:                            # before, between and after: moving calls behind frames 1 and 2
                    before = (c.uploads(), c.launch_stats())
                    c.accumulate_moving_device(wide, total, LR.APERTURE, LR.FOCUS, c.lens_sequence(2 * k, 2), np.zeros((2, 2, 3)),
                                               c.motion_sequence(2 * k, 2, v, MV.SHUTTER), 2 * k, rgb8=rgb8)
                    torch.cuda.synchronize()
                    host = np.zeros((32, 64, 3))
                    assert c.render_progressive_moving(wide, v, MV.SHUTTER, LR.APERTURE, LR.FOCUS, 4, host_rgb=host)[1] == 4 * (k + 1)
                    assert bool((total != 0.).any()) and bool((rgb8 != 0).any()) and host.any()
                    assert (c.uploads(), c.launch_stats()) == before
            return out
        finally:
            c.close()

    plain, ticked = frames(False), frames(True)
    for k, (a, b) in enumerate(zip(plain, ticked)):
        assert a.tobytes() == b.tobytes(), "frame %d differs once moving calls ran" % (k + 1)


# ---------------------------------------------------------------- 5. the tick
def test_the_tick_continues_begins_again_and_refuses(pkg, ctx, Y, capsys):
    L, B = pkg.lib(), pkg._lib
    depth = 3
    scene = Y.scene("demo")[0]
    GL.upload(ctx, scene)
    kinds = Y.kinds("demo")
    v = velocities_of(Y, "demo")
    polygon = kinds.index(MV.ORC_POLYGON)
    radii = (1.5, 3.)
    table, lights, shapes = tables(ctx, Y, "demo", 0, 24, radii)
    _, device, device8 = run_moving(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table, lights, shapes, (8, 8, 8))
    ref_mean = Y.moving("demo", 32, 32, depth, LR.APERTURE, LR.FOCUS, table, lights, shapes, (8, 8, 8))[1]
    assert GL.worst(device, ref_mean) < TIGHT                         # rows [N, N + 8) of the three sequences, tick after tick
    p = pkg.backend.make_params(workloads.FOV, 32., 32., depth)
    host, host8 = np.full((32, 32, 3), -3.5), np.full((32, 32, 3), 7, np.uint8)

    def moving(vel=v, shutter=MV.SHUTTER, r=radii, restart=False, c=ctx, **kw):
        return c.render_progressive_moving(p, vel, shutter, LR.APERTURE, LR.FOCUS, 8, r, restart, **kw)[1]

    def motion(vel, r=radii, restart=False, c=ctx, **kw):
        return c.render_progressive_motion(p, vel, MV.SHUTTER, LR.APERTURE, LR.FOCUS, 8, r, restart, **kw)[1]

    # three ticks of 8 with the same arguments: the frame goes on, and is the device call's
    assert moving(restart=True) == 8 and moving() == 16
    timing, total = ctx.render_progressive_moving(p, v, MV.SHUTTER, LR.APERTURE, LR.FOCUS, 8, radii, host_rgb=host, host_rgb8=host8)
    assert total == 24 and host.tobytes() == device.tobytes() and host8.tobytes() == device8.tobytes()
    assert timing.kernel_ms > 0. and timing.total_ms >= timing.kernel_ms
    # what begins the frame again, one at a time (each followed by a tick that goes on: 16)
    pushed = v.copy()
    pushed[polygon] = v[polygon] * 1.5
    assert moving(vel=pushed) == 8 and moving(vel=pushed) == 16       # a changed polygon velocity
    assert moving() == 8 and moving() == 16                           # ... and back
    assert moving(shutter=0.5) == 8 and moving(shutter=0.5) == 16     # a changed shutter
    assert moving() == 8 and moving() == 16
    # a switch to and from render_progressive_motion with the same sphere-only velocities
    only = MR.velocities(kinds)
    assert moving(vel=only) == 8 and moving(vel=only) == 16
    assert motion(only) == 8 and motion(only) == 16                   # moving -> motion
    assert moving(vel=only) == 8 and moving(vel=only) == 16           # motion -> moving
    assert ctx.render_progressive(p, LR.APERTURE, LR.FOCUS, 8)[1] == 8   # moving -> plain
    assert moving() == 8                                              # plain -> moving
    assert ctx.render_progressive_soft(p, radii, LR.APERTURE, LR.FOCUS, 8)[1] == 8
    assert moving(r=None) == 8 and moving(r=None) == 16               # point lights are another frame than radii
    assert moving(restart=True) == 8 and moving() == 16               # restart
    again = np.full((32, 32, 3), -3.5)
    assert moving(host_rgb=again) == 24 and again.tobytes() == device.tobytes()
    # refused calls in between change neither the count nor the key
    D = C.POINTER(C.c_double)
    lens, r64 = B.rm_lens(LR.APERTURE, LR.FOCUS, 8, 0), np.ascontiguousarray(radii, dtype=np.float64)
    for bad, n_shapes, word in ((v[:-1], len(v) - 1, "n_shapes"), (np.where(np.arange(len(v))[:, None] == polygon, NAN, v), len(v), "velocities[%d]" % polygon)):
        bad = np.ascontiguousarray(bad)
        n_total, before = C.c_uint32(77), again.copy()
        st = L.rm_render_progressive_moving(ctx.ptr, C.byref(p), C.byref(lens), r64.ctypes.data_as(D), 2, bad.ctypes.data_as(C.POINTER(B.rm_vec3)),
                                            n_shapes, MV.SHUTTER, 0, again.ctypes.data_as(D), None, C.byref(n_total), None)
        assert st == B.RM_ERR_INVALID_ARG and n_total.value == 77 and again.tobytes() == before.tobytes()
        assert word in L.rm_last_error(ctx.ptr).decode(), L.rm_last_error(ctx.ptr)
    for shutter in (-1e-9, NAN, float("inf")):
        n_total = C.c_uint32(77)
        st = L.rm_render_progressive_moving(ctx.ptr, C.byref(p), C.byref(lens), r64.ctypes.data_as(D), 2, v.ctypes.data_as(C.POINTER(B.rm_vec3)),
                                            len(v), shutter, 0, again.ctypes.data_as(D), None, C.byref(n_total), None)
        assert st == B.RM_ERR_INVALID_ARG and n_total.value == 77 and b"shutter" in L.rm_last_error(ctx.ptr)
    with pytest.raises(B.BackendError, match="is not a sphere"):       # the moving spheres' tick keeps refusing, and leaves this frame alone
        motion(v)
    assert moving() == 32                                             # ... the frame went through all that untouched
    # the two ticks alternating on one context equal contexts that make one kind of call
    a, b = pkg.backend.Context(0), pkg.backend.Context(0)
    try:
        a.upload(scene.flatten())
        b.upload(scene.flatten())
        alt_moving, alt_motion, one_moving, one_motion = (np.full((32, 32, 3), -3.5) for _ in range(4))
        for k in range(2):
            assert moving(restart=True, host_rgb=alt_moving) == 8 and motion(only, restart=True, host_rgb=alt_motion) == 8
        assert moving(restart=True, c=a, host_rgb=one_moving) == 8 and motion(only, restart=True, c=b, host_rgb=one_motion) == 8
        assert alt_moving.tobytes() == one_moving.tobytes() and alt_motion.tobytes() == one_motion.tobytes()
        assert alt_moving.tobytes() != alt_motion.tobytes()
    finally:
        a.close()
        b.close()
    # Renderer.render_progressive_moving and render_moving_shapes: the prints and the return value of render()
    r = pkg.create_renderer(workloads.FOV, 32., 32.)
    r.max_depth = depth
    fb = pkg.create_frame_buffer(32, 32)
    vel = [pkg.Vec3f(*e) for e in v]
    capsys.readouterr()
    message = r.render_progressive_moving(fb, scene, vel, MV.SHUTTER, 8, radii, LR.APERTURE, LR.FOCUS, restart=True)
    out = capsys.readouterr().out
    assert message.startswith("Scene rendered in ") and message in out and "compute units used" in out
    assert r.last_samples == 8 and r.last_timing.kernel_ms > 0.
    r.render_progressive_moving(fb, scene, vel, MV.SHUTTER, 8, radii, LR.APERTURE, LR.FOCUS)
    r.render_progressive_moving(fb, scene, vel, MV.SHUTTER, 8, radii, LR.APERTURE, LR.FOCUS)
    assert r.last_samples == 24 and fb.buffer.tobytes() == device.tobytes()
    # the one-shot: 80 samples in slices of 64 and 16, through a pinhole, point lights
    r.render_moving_shapes(fb, scene, vel, MV.SHUTTER, 80)
    assert r.last_samples == 80
    t80, l80, s80 = tables(ctx, Y, "demo", 0, 80, None)
    blur = run_moving(pkg, ctx, 32, 32, depth, 0., 1., t80, l80, s80, (16,) * 5)[1]      # (a left fold: however the passes are sliced)
    assert fb.buffer.tobytes() == blur.tobytes()


def test_a_saturated_frame_stands(pkg, ctx, Y):
    """1,024 ticks of 64 fill the frame to RM_PROGRESSIVE_MAX_SAMPLES; the next tick launches nothing and returns it as it stands."""
    GL.upload(ctx, Y.scene("pool")[0])
    v = velocities_of(Y, "pool")
    p = pkg.backend.make_params(workloads.FOV, 32., 32., 1)
    assert ctx.render_progressive_moving(p, v, MV.SHUTTER, 0., LR.FOCUS, 64, restart=True)[1] == 64
    for k in range(2, 1024):
        total = ctx.render_progressive_moving(p, v, MV.SHUTTER, 0., LR.FOCUS, 64)[1]
    assert total == 65472
    before, before8 = np.full((32, 32, 3), NAN), np.full((32, 32, 3), BYTE, np.uint8)
    assert ctx.render_progressive_moving(p, v, MV.SHUTTER, 0., LR.FOCUS, 64, host_rgb=before, host_rgb8=before8)[1] == 65536 == MR.MAX_SAMPLES
    assert not np.isnan(before).any() and before8.tobytes() == PR.to_bytes(before).tobytes()
    for n in (64, 1):
        after, after8 = np.full((32, 32, 3), NAN), np.full((32, 32, 3), BYTE, np.uint8)
        timing, total = ctx.render_progressive_moving(p, v, MV.SHUTTER, 0., LR.FOCUS, n, host_rgb=after, host_rgb8=after8)
        assert total == 65536 and timing.kernel_ms == 0.
        assert after.tobytes() == before.tobytes() and after8.tobytes() == before8.tobytes()
    assert ctx.render_progressive_moving(p, v, MV.SHUTTER, 0., LR.FOCUS, 64, restart=True)[1] == 64


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
    shapes = torch.from_numpy(MR.motion_sequence(0, 4, velocities_of(Y, "demo"), 1.)).to("cuda:0")
    good = B.rm_lens(LR.APERTURE, LR.FOCUS, 4, 0)
    vp = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None

    def untouched():
        torch.cuda.synchronize()
        return bool((total == 7.25).all()) and bool((mean == 7.25).all()) and bool((rgb8 == 7).all())

    def device_call(lens=good, t=table, o=lights, n_lights=2, so=shapes, ns=n_shapes, s=total, m=mean, n_before=4, params=p):
        st = L.rm_accumulate_moving_device(ctx.ptr, C.byref(params), C.byref(lens), vp(t), vp(o), n_lights, vp(so), ns, n_before, vp(s), vp(m),
                                           vp(rgb8), None)
        msg = L.rm_last_error(ctx.ptr).decode()
        assert st != 0 and untouched(), msg
        assert msg.startswith("rm_accumulate_moving_device") or st != B.RM_ERR_INVALID_ARG, msg
        return st, msg

    E = B.RM_ERR_INVALID_ARG
    for ns in (0, n_shapes - 1, n_shapes + 1, 2 ** 32 - 1):
        st, msg = device_call(ns=ns)
        assert st == E and "n_shapes" in msg and "the resident scene has %d" % n_shapes in msg
    st, msg = device_call(so=None)
    assert st == E and "NULL shape offsets" in msg
    for n_lights in (0, 1, 3, 2 ** 32 - 1):
        st, msg = device_call(n_lights=n_lights)
        assert st == E and "n_lights" in msg and "the resident scene has 2" in msg
    st, msg = device_call(o=None)
    assert st == E and "NULL light offsets" in msg
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
        assert L.rm_accumulate_moving_device(fresh.ptr, C.byref(p), C.byref(good), vp(table), vp(lights), 2, vp(shapes), n_shapes, 0, vp(total),
                                             vp(mean), vp(rgb8), None) == B.RM_ERR_NO_SCENE
        n_total = C.c_uint32(77)
        v = np.zeros((n_shapes, 3))
        assert L.rm_render_progressive_moving(fresh.ptr, C.byref(p), C.byref(good), None, 0, v.ctypes.data_as(C.POINTER(B.rm_vec3)), n_shapes, 1., 0,
                                              None, None, C.byref(n_total), None) == B.RM_ERR_NO_SCENE and n_total.value == 77
    finally:
        fresh.close()
    assert untouched()
    # a scene without a sphere still needs its table here (the moving spheres' call takes NULL for it)
    GL.upload(ctx, Y.scene("cornell")[0])
    nc, lc = Y.n_shapes("cornell"), Y.n_lights("cornell")
    small = pkg.backend.make_params(workloads.FOV, 32., 32., depth)
    l4 = torch.zeros((4, lc, 3), dtype=torch.float64, device="cuda:0")
    st = L.rm_accumulate_moving_device(ctx.ptr, C.byref(small), C.byref(good), vp(table), vp(l4), lc, None, nc, 0, vp(total), vp(mean), vp(rgb8), None)
    assert st == E and "NULL shape offsets" in L.rm_last_error(ctx.ptr).decode() and untouched()
    # what is tolerated: a frame without a whole patch row
    GL.upload(ctx, Y.scene("demo")[0])
    short = run_moving(pkg, ctx, 64, 31, depth, LR.APERTURE, LR.FOCUS, PR.lens_sequence(0, 4), np.zeros((4, 2, 3)), np.zeros((4, n_shapes, 3)), (4,))
    assert np.isnan(short[0]).all() and np.isnan(short[1]).all() and np.all(short[2] == BYTE)   # rows == 0: RM_OK, nothing done


def test_a_scene_with_no_shape_at_all_takes_a_null_table(pkg, ctx):
    """Lights and a camera alone: every ray leaves the scene, and neither the device call nor the tick asks for shape offsets."""
    import torch
    L, B = pkg.lib(), pkg._lib
    empty = pkg.Scene.new()
    empty.lights.append(pkg.create_light(pkg.Vec3f(0., 5., 0.), pkg.Vec3f(1., 1., 1.), 1.))
    GL.upload(ctx, empty)
    p = pkg.backend.make_params(workloads.FOV, 32., 32., 3)
    lens = B.rm_lens(LR.APERTURE, LR.FOCUS, 4, 0)
    table = torch.from_numpy(PR.lens_sequence(0, 4)).to("cuda:0")
    lights = torch.zeros((4, 1, 3), dtype=torch.float64, device="cuda:0")
    total, mean = (torch.full((32, 32, 3), NAN, dtype=torch.float64, device="cuda:0") for _ in range(2))
    vp = lambda x: C.c_void_p(x.data_ptr())
    assert L.rm_accumulate_moving_device(ctx.ptr, C.byref(p), C.byref(lens), vp(table), vp(lights), 1, None, 0, 0, vp(total), vp(mean), None, None) == 0, \
        L.rm_last_error(ctx.ptr)
    torch.cuda.synchronize()
    got = mean.cpu().numpy()
    assert not np.isnan(got).any() and (got == got[0, 0]).all()       # the background, everywhere
    host, n_total = np.full((32, 32, 3), NAN), C.c_uint32(0)
    assert L.rm_render_progressive_moving(ctx.ptr, C.byref(p), C.byref(lens), None, 0, None, 0, 1., 1, host.ctypes.data_as(C.POINTER(C.c_double)), None,
                                          C.byref(n_total), None) == 0, L.rm_last_error(ctx.ptr)
    assert n_total.value == 4 and host.tobytes() == got.tobytes()


def test_a_capped_grid_changes_nothing(pkg, ctx, Y, monkeypatch):
    """RM_LENS_MAX_BLOCKS = 1 (read at rm_init: a context of its own) caps this kernel's grid too and drives its loop over the
    groups and its tail; 64 x 32: two patches a row."""
    depth, radii, (aperture, focus) = SCENES["pool"]
    scene = Y.scene("pool")[0]
    GL.upload(ctx, scene)
    table, lights, shapes = tables(ctx, Y, "pool", 0, 24, radii)
    plans = ((1, 1), (5, 7), (16, 8))
    free = {s: run_moving(pkg, ctx, 64, 32, depth, aperture, focus, table[:sum(s)], lights[:sum(s)], shapes[:sum(s)], s) for s in plans}
    monkeypatch.setenv("RM_LENS_MAX_BLOCKS", "1")
    c = pkg.backend.Context(0)
    try:
        c.upload(scene.flatten())
        for s in plans:
            got = run_moving(pkg, c, 64, 32, depth, aperture, focus, table[:sum(s)], lights[:sum(s)], shapes[:sum(s)], s)
            same(got, free[s], "1 workgroup, passes %s" % (s,))
    finally:
        c.close()
    assert not np.isnan(free[(16, 8)][1]).any()
