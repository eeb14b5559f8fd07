"""Converging frames with a moving camera over a swept hierarchy on the GPU (-m gpu):
rm_accumulate_converging_camera_swept_device through the C ABI and the Python bindings, against
rm_accumulate_converging_camera_device given the same four tables pass for pass -- sums, stats, counts, means, bytes, masks, lists
and their lengths, byte for byte -- and against the plain run of rm_accumulate_camera_swept_device.  The context is oriented, the
camera translates and turns.  Frames are 32 x 32, passes of 4 or 5 samples, depth 5 (4 parked rays a lane) and 6 (32)."""
import numpy as np
import pytest

import camera_motion_reference as CM
import moving_reference as MV
import radiance_reference as RR
import test_gpu_camera_swept as GCS
import test_gpu_converge as GC
import test_gpu_converge_moving as GCM
import test_gpu_lens as GL
import test_gpu_progressive as GP
import test_gpu_swept as GSW
import variant_matrix as VM
import workloads

pytestmark = pytest.mark.gpu

NAN, BYTE = GP.NAN, GP.BYTE
Frame = GC.Frame
FLAT, SWEPT = "accumulate_converging_camera_device", "accumulate_converging_camera_swept_device"
KEYS = ("sum", "stats", "count", "mean", "rgb8", "mask", "list")
NS, TOL, LO, HI = 4, 0.02, 8, 24                                       # samples a pass, tolerance, min_samples, max_samples


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_converge_camera_swept"))


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return CM.Yardstick(pkg, O, orc)


def device_tables(ctx, Y, key, name, rows):
    """(lens, camera, lights, shapes) on the device: rows 0 .. rows of the library's four sequences, the camera's from the
    context's basis."""
    table, lights, shapes, _ = GSW.tables(ctx, Y, key, name, rows)
    assert (shapes != 0.).any()
    return GCM.on_device(table, GCS.camera_of(ctx, name, rows), lights, shapes)


def one_pass(pkg, c, f, depth, ns, tol, lo, hi, tables, fresh, call, **kw):
    p = pkg.backend.make_params(workloads.FOV, float(f.h), float(f.w), depth)
    table, camera, lights, shapes = tables
    getattr(c, call)(p, f.sum, f.stats, f.count, VM.APERTURE, VM.FOCUS, ns, table, camera, lights, shapes, tol, lo, hi, fresh, mean=f.mean,
                     rgb8=f.rgb8, mask=f.mask, workspace=f.ws[:f.ws_words], **kw)


def three_passes(pkg, c, depth, tables, call):
    f, out = Frame(pkg, 32, 32), []
    for k in range(3):
        one_pass(pkg, c, f, depth, NS, TOL, LO, HI, tables, k == 0, call)
        out.append(f.snapshot())
    return out


# ---------------------------------------------------------------- 1. the flat pass's bytes, pass for pass, both stacks
@pytest.mark.parametrize("depth", [5, 6])
@pytest.mark.parametrize("name", ["matrix-spheres", "matrix-mesh"])
def test_swept_camera_passes_are_the_flat_camera_passes_byte_for_byte(pkg, ctx, Y, name, depth):
    key, scene = GSW.scene_of(Y, name)
    try:
        GCS.oriented(pkg, ctx, scene)
        tables = device_tables(ctx, Y, key, name, HI)
        flat = three_passes(pkg, ctx, depth, tables, FLAT)
        swept = three_passes(pkg, ctx, depth, tables, SWEPT)
    finally:
        ctx.orient(None)
    for k, (a, b) in enumerate(zip(swept, flat)):
        # (the workspace's head, and behind it the list)
        assert a["listed"] == b["listed"], "%s pass %d: %d listed, the flat pass lists %d" % (name, k, a["listed"], b["listed"])
        for part in KEYS:
            assert a[part].tobytes() == b[part].tobytes(), "%s depth %d pass %d: %s differs" % (name, depth, k, part)
    last = flat[-1]
    print("%s depth %d: listed %s, counts %d .. %d" % (name, depth, [s["listed"] for s in flat], last["count"].min(), last["count"].max()))
    assert not np.isnan(last["mean"]).any() and last["mean"].any()
    assert flat[0]["listed"] == flat[1]["listed"] == 1024               # (two passes to min_samples, then the rule decides)
    assert 0 < last["listed"] < 1024                                    # some pixels settle at min_samples, some do not


# ---------------------------------------------------------------- 2. tolerance < 0 is the plain swept camera frame
@pytest.mark.parametrize("depth", [5, 6])
def test_a_negative_tolerance_is_the_plain_swept_camera_frame(pkg, ctx, Y, depth):
    import torch
    key, scene = GSW.scene_of(Y, "matrix-mesh")
    try:
        GCS.oriented(pkg, ctx, scene)
        tables = device_tables(ctx, Y, key, "matrix-mesh", 15)
        handle = ctx.swept(*pkg.backend.swept_extents(tables[3].cpu().numpy()))
        try:
            p = pkg.backend.make_params(workloads.FOV, 32., 32., depth)
            total = torch.full((32, 32, 3), NAN, dtype=torch.float64, device="cuda:0")
            mean = torch.full((32, 32, 3), NAN, dtype=torch.float64, device="cuda:0")
            rgb8 = torch.full((32, 32, 3), BYTE, dtype=torch.uint8, device="cuda:0")
            f = Frame(pkg, 32, 32)
            for k in range(3):
                rows = slice(5 * k, 5 * (k + 1))
                ctx.accumulate_camera_swept_device(p, total, VM.APERTURE, VM.FOCUS, *(t[rows].contiguous() for t in tables), 5 * k, mean=mean,
                                                   rgb8=rgb8, swept=handle)
                one_pass(pkg, ctx, f, depth, 5, -1., 15, 15, tables, k == 0, SWEPT, swept=handle)
                got = f.snapshot()
                n = 5 * (k + 1)
                assert got["listed"] == 1024 and np.all(got["count"] == n) and np.all(got["mask"] == 1)
                for part, ref in zip(("sum", "mean", "rgb8"), (total, mean, rgb8)):
                    assert got[part].tobytes() == ref.cpu().numpy().tobytes(), "depth %d, %d samples: %s differs" % (depth, n, part)
            assert got["mean"].any()
        finally:
            handle.close()
    finally:
        ctx.orient(None)


# ---------------------------------------------------------------- 3. refusals
def test_refusals_name_the_offender_and_the_buffers_keep_their_bytes(pkg, ctx, Y):
    """tests/test_gpu_camera_swept.py's refusals through the converging call, by the C ABI itself: another context's handle, a NULL
    shape table (refused among the tables, in front of the handle's checks), no handle, a stale handle and a freed one.  Every
    buffer of the frame and the guard behind it keep their bytes, and the context still serves."""
    import ctypes as C

    import torch
    L, B = pkg.lib(), pkg._lib
    key, scene = GSW.scene_of(Y, "matrix-mesh")
    other_key, other = GSW.scene_of(Y, "thirteen")
    GL.upload(ctx, scene)
    n_shapes, n_lights = Y.n_shapes(key), Y.n_lights(key)
    p = pkg.backend.make_params(workloads.FOV, 32., 32., 3)
    lens, conv = B.rm_lens(0., 1., 4, 0), B.rm_converge(0.02, 8, 8)
    f = Frame(pkg, 32, 32, guard=4096)
    vp = lambda t: C.c_void_p(t.data_ptr())
    frame = B.rm_converge_frame(vp(f.sum), vp(f.stats), vp(f.count), vp(f.ws), vp(f.mean), vp(f.rgb8), vp(f.mask))

    def state():
        torch.cuda.synchronize()
        return [f.raw[k].cpu().numpy().tobytes() for k in sorted(f.raw)] + [f.ws.cpu().numpy().tobytes()]

    before = state()

    def raw(swept, shapes_of, lights_of, with_shapes=True):
        table, camera = GCM.on_device(ctx.lens_sequence(0, 8), CM.standing_rows(8))
        lights, shapes = GCM.on_device(np.zeros((8, lights_of, 3)), np.zeros((8, shapes_of, 3)))
        st = L.rm_accumulate_converging_camera_swept_device(ctx.ptr, C.byref(p), C.byref(lens), C.byref(conv), vp(table), 8, vp(camera), vp(lights),
                                                            lights_of, vp(shapes) if with_shapes else None, shapes_of, swept, 1, C.byref(frame), None)
        torch.cuda.synchronize()
        return st, L.rm_last_error(ctx.ptr)

    who = b"rm_accumulate_converging_camera_swept_device: "
    handle = ctx.swept(np.zeros((n_shapes, 3)), np.zeros((n_shapes, 3)))
    c2 = pkg.backend.Context(0)
    try:
        GL.upload(c2, scene)
        foreign = c2.swept(np.zeros((n_shapes, 3)), np.zeros((n_shapes, 3)))
        st, err = raw(foreign.ptr, n_shapes, n_lights)
        assert st == B.RM_ERR_INVALID_ARG and err == who + b"swept is not a handle of this context", err
        st, err = raw(handle.ptr, n_shapes, n_lights, with_shapes=False)
        assert st == B.RM_ERR_INVALID_ARG and err == who + b"NULL shape offsets", err
        st, err = raw(None, n_shapes, n_lights, with_shapes=False)       # (the tables are looked at first)
        assert st == B.RM_ERR_INVALID_ARG and err == who + b"NULL shape offsets", err
        st, err = raw(None, n_shapes, n_lights)
        assert st == B.RM_ERR_INVALID_ARG and err == who + b"NULL swept", err
        st, err = raw(handle.ptr, n_shapes + 1, n_lights)
        assert st == B.RM_ERR_INVALID_ARG and b"n_shapes %d, the resident scene has %d" % (n_shapes + 1, n_shapes) in err, err
        GL.upload(ctx, other)                                            # stale: the scene changed
        st, err = raw(handle.ptr, Y.n_shapes(other_key), Y.n_lights(other_key))
        assert st == B.RM_ERR_INVALID_ARG and err.startswith(who + b"swept was built before the scene last changed"), err
        GL.upload(ctx, scene)
        freed = C.c_void_p(handle.ptr.value)
        handle.close()                                                   # freed: looked up, not looked into
        st, err = raw(freed, n_shapes, n_lights)
        assert st == B.RM_ERR_INVALID_ARG and err == who + b"swept is not a handle of this context", err
        assert state() == before
        fresh = ctx.swept(np.zeros((n_shapes, 3)), np.zeros((n_shapes, 3)))
        try:
            st, err = raw(fresh.ptr, n_shapes, n_lights)                 # ... and the context still serves
            assert st == 0, err
        finally:
            fresh.close()
        got = f.snapshot()
        assert got["listed"] == 1024 and np.all(got["count"] == 4) and not np.isnan(got["mean"]).any()
    finally:
        handle.close()
        c2.close()
