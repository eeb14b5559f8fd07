"""Swept hierarchies on the GPU (-m gpu): rm_swept_build, rm_accumulate_swept_device and the moving shapes' ticks through the C
ABI and the Python bindings, against the flat passes of rm_accumulate_moving_device -- byte for byte, as the header says -- and
against tests/moving_reference.py within TIGHT = 1e-9 on every channel of every pixel (n TIGHT of a sum of n samples).

Frames are 32 x 32 (64 x 64 for the chain scenes, whose trees are deep), a pass casts 5 to 8 rows, depth 3 to 6."""
import numpy as np
import pytest

import hierarchy_reference as HR
import lens_reference as LR
import moving_reference as MV
import radiance_reference as RR
import swept_reference as SW
import test_gpu_lens as GL
import test_gpu_motion as GM
import test_gpu_moving as GMV
import test_gpu_progressive as GP
import variant_matrix as VM
import workloads

pytestmark = pytest.mark.gpu

NAN, BYTE = GP.NAN, GP.BYTE
same = GMV.same
# scene -> (frame side, fov, aperture, focus)
CHAIN_VIEW = (HR.CHAIN_W, HR.CHAIN_FOV, HR.CHAIN_APERTURE, HR.CHAIN_FOCUS)
VIEW = {"chain-spheres": CHAIN_VIEW, "chain-mesh": CHAIN_VIEW, "pinhole": (32, workloads.FOV, 0., VM.FOCUS)}
DEFAULT_VIEW = (32, workloads.FOV, VM.APERTURE, VM.FOCUS)
# (scene, generic exponents -- the matrix's alone --, depth): depth <= 5 takes STACK = 4, 6 takes 32
CASES = [(name, False, depth) for name in SW.SCENES for depth in (5, 6)] + [("matrix-spheres", True, 5), ("matrix-mesh", True, 6)]


def case_id(case):
    return "%s%s-%d" % (case[0], "-generic" if case[1] else "", case[2])


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_swept"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return MV.Yardstick(pkg, O, orc)


def scene_of(Y, name, generic=False):
    """The scene as one of the yardstick's, made once -> (its name there, the product scene)."""
    key = name + ("-generic" if generic else "")
    if key not in Y._scene:
        if name.startswith("matrix-"):
            pair = VM.scene_pair(Y.pkg, Y.O, name[len("matrix-"):], generic)
        else:
            pair = SW.scene_pair(Y.pkg, Y.O, name)
        VM.register(Y, key, pair)
    return key, Y.scene(key)[0]


def tables(ctx, Y, key, name, n, only=None):
    """Rows 0 .. n of the library's three sequences for the scene and the test velocities (point lights)."""
    v = MV.velocities(Y.kinds(key), MV.SPEED.get(name, MV.CELL_SPEED), only)
    return ctx.lens_sequence(0, n), np.zeros((n, Y.n_lights(key), 3)), ctx.motion_sequence(0, n, v, MV.SHUTTER), v


def run(pkg, c, name, depth, table, lights, shapes, sizes, call, **kw):
    """GMV.run_moving with the scene's own frame and view, and `kw` (swept=) handed to the call."""
    import torch
    side, fov, aperture, focus = VIEW.get(name, DEFAULT_VIEW)
    p = pkg.backend.make_params(fov, float(side), float(side), depth)
    total = torch.full((side, side, 3), NAN, dtype=torch.float64, device="cuda:0")
    mean = torch.full((side, side, 3), NAN, dtype=torch.float64, device="cuda:0")
    rgb8 = torch.full((side, side, 3), BYTE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    done = 0
    assert sum(sizes) == len(table) == len(lights) == len(shapes)
    for n in sizes:
        getattr(c, call)(p, total, aperture, focus, np.ascontiguousarray(table[done:done + n]), np.ascontiguousarray(lights[done:done + n]),
                         np.ascontiguousarray(shapes[done:done + n]), done, mean=mean, rgb8=rgb8, **kw)
        done += n
    torch.cuda.synchronize()
    return total.cpu().numpy(), mean.cpu().numpy(), rgb8.cpu().numpy()


FLAT, SWEPT = "accumulate_moving_device", "accumulate_swept_device"


# ---------------------------------------------------------------- 1. the flat pass's bytes
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_a_swept_pass_leaves_the_flat_passs_bytes(pkg, ctx, Y, case):
    """Every scene, both stacks and, on the matrix's scenes, both powers: 3 + 5 rows of the library's tables with the test
    velocities.  The handle is the binding's own, from the table's extents."""
    name, generic, depth = case
    key, scene = scene_of(Y, name, generic)
    GL.upload(ctx, scene)
    table, lights, shapes, _ = tables(ctx, Y, key, name, 8)
    assert (shapes != 0.).any()
    flat = run(pkg, ctx, name, depth, table, lights, shapes, (3, 5), FLAT)
    swept = run(pkg, ctx, name, depth, table, lights, shapes, (3, 5), SWEPT)
    same(swept, flat, case_id(case))
    assert flat[1].any() and len(np.unique(flat[2])) > 4                # a picture, not a background


# ---------------------------------------------------------------- 2. parity with the yardstick
@pytest.mark.parametrize("name,depth", [("matrix-spheres", 5), ("matrix-mesh", 5), ("cornell", 3)])
def test_swept_frames_match_the_yardstick(pkg, ctx, Y, name, depth):
    key, scene = scene_of(Y, name)
    GL.upload(ctx, scene)
    table, lights, shapes, _ = tables(ctx, Y, key, name, 8)
    got = run(pkg, ctx, name, depth, table, lights, shapes, (8,), SWEPT)
    _, _, aperture, focus = DEFAULT_VIEW
    ref_sum, ref_mean = Y.moving(key, 32, 32, depth, aperture, focus, table, lights, shapes, (8,))
    GM.held(got, ref_sum, ref_mean, 8, "%s depth %d, 8 rows through a swept hierarchy" % (name, depth))


# ---------------------------------------------------------------- 3. handles of the caller's own
def test_one_mesh_of_the_cornell_box_moves_and_wider_extents_change_no_byte(pkg, ctx, Y):
    """Only Obj CORNELL_MOVER moves: the others get extents of zero.  Then the handle from the documented extents of the
    velocities (every row of the sequence, not these eight), and one four times wider than needed."""
    key, scene = scene_of(Y, "cornell")
    GL.upload(ctx, scene)
    table, lights, shapes, v = tables(ctx, Y, key, "cornell", 8, MV.CORNELL_MOVER)
    lo, hi = pkg.backend.swept_extents(shapes)
    assert list(np.flatnonzero((lo != 0.).any(axis=1) | (hi != 0.).any(axis=1))) == [MV.CORNELL_MOVER]
    flat = run(pkg, ctx, "cornell", 3, table, lights, shapes, (8,), FLAT)
    for what, (l, h) in (("the table's extents", (lo, hi)), ("the velocities' extents", pkg.backend.swept_motion_extents(v, MV.SHUTTER)),
                         ("four times wider", (4. * lo - 1., 4. * hi + 1.))):
        handle = ctx.swept(l, h)
        try:
            same(run(pkg, ctx, "cornell", 3, table, lights, shapes, (8,), SWEPT, swept=handle), flat, "cornell, " + what)
        finally:
            handle.close()
    still = run(pkg, ctx, "cornell", 3, table, lights, np.zeros_like(shapes), (8,), FLAT)
    assert int((np.abs(flat[1] - still[1]) > 0.05).any(axis=2).sum()) > 32    # the mover's blur is in the picture


def test_passes_of_3_5_and_8_rows_are_one_pass_of_16(pkg, ctx, Y):
    key, scene = scene_of(Y, "matrix-spheres")
    GL.upload(ctx, scene)
    table, lights, shapes, v = tables(ctx, Y, key, "matrix-spheres", 16)
    handle = ctx.swept(*pkg.backend.swept_motion_extents(v, MV.SHUTTER))
    try:
        one = run(pkg, ctx, "matrix-spheres", 5, table, lights, shapes, (16,), SWEPT, swept=handle)
        three = run(pkg, ctx, "matrix-spheres", 5, table, lights, shapes, (3, 5, 8), SWEPT, swept=handle)
    finally:
        handle.close()
    same(three, one, "3 + 5 + 8")
    same(one, run(pkg, ctx, "matrix-spheres", 5, table, lights, shapes, (16,), FLAT), "16 rows against the flat pass")


# ---------------------------------------------------------------- 4. images without a hierarchy
def test_a_context_without_hierarchies_walks_flat(pkg, ctx, Y, monkeypatch):
    """RM_DISABLE_BVH=1: the image of matrix-spheres holds no hierarchy; the build succeeds and the pass is the flat one (the
    demo, whose image never holds one, is among the cases above)."""
    key, scene = scene_of(Y, "matrix-spheres")
    table, lights, shapes, _ = tables(ctx, Y, key, "matrix-spheres", 5)
    GL.upload(ctx, scene)
    with_bvh = run(pkg, ctx, "matrix-spheres", 5, table, lights, shapes, (5,), SWEPT)
    monkeypatch.setenv("RM_DISABLE_BVH", "1")
    c = pkg.backend.Context(0)
    try:
        GL.upload(c, scene)
        flat = run(pkg, c, "matrix-spheres", 5, table, lights, shapes, (5,), FLAT)
        same(run(pkg, c, "matrix-spheres", 5, table, lights, shapes, (5,), SWEPT), flat, "RM_DISABLE_BVH=1")
    finally:
        c.close()
    same(with_bvh, flat, "with and without the image's hierarchy")


# ---------------------------------------------------------------- 5. the boxes are consulted
def test_a_row_outside_the_extents_is_missed(pkg, ctx, Y, orc):
    """A handle with extents of zero and a table that moves one small sphere of matrix-spheres by several times its radius
    across the view: the flat pass shows it where the row puts it, the swept pass looks for it in boxes about where it was.
    The input breaks the header's precondition and is safe by its contract: no offset or box forms an address.  Without this
    test a build that quietly walks flat passes every other one.

    Which sphere: the first whose moved self is the closest hit of 8 or more pixel-centre rays the image's own boxes never
    lead to, by tests/hierarchy_reference.py's walk model on the CPU."""
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
    n = 5
    table, lights = ctx.lens_sequence(0, n), np.zeros((n, Y.n_lights(key), 3))
    shapes = np.tile(row, (n, 1, 1))
    flat = run(pkg, ctx, "pinhole", 3, table, lights, shapes, (n,), FLAT)
    handle = ctx.swept(np.zeros((n_shapes, 3)), np.zeros((n_shapes, 3)))
    try:
        zero = run(pkg, ctx, "pinhole", 3, table, lights, shapes, (n,), SWEPT, swept=handle)
        # (the same handle with rows it does hold is the flat pass: what differs below is the boxes' doing)
        same(run(pkg, ctx, "pinhole", 3, table, lights, np.zeros_like(shapes), (n,), SWEPT, swept=handle),
             run(pkg, ctx, "pinhole", 3, table, lights, np.zeros_like(shapes), (n,), FLAT), "zero rows, zero extents")
    finally:
        handle.close()
    differ = int((zero[1] != flat[1]).any(axis=2).sum())
    print("shape %d moved out of its boxes: %d pixel centres lose it in the model, %d pixels differ on the GPU" % (k, lost, differ))
    assert not np.isnan(zero[1]).any() and differ >= 1
    same(run(pkg, ctx, "pinhole", 3, table, lights, shapes, (n,), SWEPT), flat, "the same rows under a handle that holds them")


# ---------------------------------------------------------------- 6. refusals
def test_a_stale_handle_is_refused_and_the_buffers_keep_their_bytes(pkg, ctx, Y):
    import torch
    key, scene = scene_of(Y, "matrix-mesh")
    other_key, other = scene_of(Y, "thirteen")
    GL.upload(ctx, scene)
    n_shapes = Y.n_shapes(key)
    handle = ctx.swept(np.zeros((n_shapes, 3)), np.zeros((n_shapes, 3)))
    p = pkg.backend.make_params(workloads.FOV, 32., 32., 3)
    n, guard = 32 * 32 * 3, 4096
    bufs = [torch.full((n + guard,), NAN, dtype=torch.float64, device="cuda:0"), torch.full((n + guard,), NAN, dtype=torch.float64, device="cuda:0"),
            torch.full((n + guard,), BYTE, dtype=torch.uint8, device="cuda:0")]
    before = [b.cpu().numpy().copy() for b in bufs]
    total, mean, rgb8 = (b[:n].view(32, 32, 3) for b in bufs)

    def call(key_, swept):
        table, lights = ctx.lens_sequence(0, 5), np.zeros((5, Y.n_lights(key_), 3))
        ctx.accumulate_swept_device(p, total, 0., 1., table, lights, np.zeros((5, Y.n_shapes(key_), 3)), 0, mean=mean, rgb8=rgb8, swept=swept)

    def untouched():
        torch.cuda.synchronize()
        return all(b.cpu().numpy().tobytes() == a.tobytes() for b, a in zip(bufs, before))

    try:
        GL.upload(ctx, other)
        with pytest.raises(pkg._lib.BackendError, match="rm_accumulate_swept_device: swept was built before the scene last changed"):
            call(other_key, handle)
        assert untouched()
        # ... also once the first scene is back: another image epoch, another handle
        GL.upload(ctx, scene)
        with pytest.raises(pkg._lib.BackendError, match="before the scene last changed"):
            call(key, handle)
        assert untouched()
    finally:
        handle.close()
    with pytest.raises(ValueError, match="open Swept handle"):
        call(key, handle)                                               # closed: the binding's own refusal
    with pytest.raises(pkg._lib.BackendError, match="n_shapes %d, the resident scene has %d" % (n_shapes + 1, n_shapes)):
        ctx.swept(np.zeros((n_shapes + 1, 3)), np.zeros((n_shapes + 1, 3)))
    bad = np.zeros((n_shapes, 3))
    bad[2, 0] = np.inf
    with pytest.raises(pkg._lib.BackendError, match="rm_swept_build: the extents of shape 2"):
        ctx.swept(np.zeros((n_shapes, 3)), bad)
    assert untouched()
    call(key, None)                                                    # ... and the context still serves
    assert not untouched()


# ---------------------------------------------------------------- 7. the ticks
@pytest.mark.parametrize("name", ["matrix-mesh", "matrix-spheres"])
def test_the_ticks_walk_the_hierarchy_to_the_flat_ticks_bytes(pkg, Y, name, monkeypatch):
    """Two contexts, the default and RM_SWEPT_BVH=0 (flat, as the ticks always were): three ticks of 5 samples of
    render_progressive_moving and of render_converging_moving return equal means and bytes; a changed velocity begins the
    frame again (the count says so) and still matches."""
    key, scene = scene_of(Y, name)
    v = MV.velocities(Y.kinds(key), MV.CELL_SPEED)
    faster = 1.5 * np.asarray(v)
    p = pkg.backend.make_params(workloads.FOV, 32., 32., 5)

    def ticks(c):
        GL.upload(c, scene)
        out = []
        for vel, restart in ((v, True), (v, False), (faster, False), (faster, False)):
            rgb, rgb8 = np.full((32, 32, 3), NAN), np.full((32, 32, 3), BYTE, np.uint8)
            _, total = c.render_progressive_moving(p, vel, MV.SHUTTER, VM.APERTURE, VM.FOCUS, 5, restart=restart, host_rgb=rgb, host_rgb8=rgb8)
            out.append((total, rgb.tobytes(), rgb8.tobytes()))
        for vel, restart in ((v, True), (v, False), (faster, False), (faster, False)):
            rgb, rgb8 = np.full((32, 32, 3), NAN), np.full((32, 32, 3), BYTE, np.uint8)
            _, rep = c.render_converging_moving(p, vel, MV.SHUTTER, VM.APERTURE, VM.FOCUS, 5, 0.01, 10, 20, restart=restart, host_rgb=rgb,
                                                host_rgb8=rgb8)
            assert not np.isnan(rgb).any()
            out.append(((rep.listed, rep.passes, rep.max_count, rep.samples_cast), rgb.tobytes(), rgb8.tobytes()))
        return out

    c = pkg.backend.Context(0)
    try:
        swept = ticks(c)
    finally:
        c.close()
    monkeypatch.setenv("RM_SWEPT_BVH", "0")
    c = pkg.backend.Context(0)
    try:
        flat = ticks(c)
    finally:
        c.close()
    assert [t[0] for t in swept[:4]] == [5, 10, 5, 10]                  # the changed velocity began the frame again
    assert [t[0][1] for t in swept[4:]] == [1, 2, 1, 2]
    for k, (a, b) in enumerate(zip(swept, flat)):
        assert a == b, "%s: tick %d differs between the swept and the flat walk" % (name, k)
    assert swept[1][1] != swept[3][1]                                   # ... and the faster shapes are another picture
