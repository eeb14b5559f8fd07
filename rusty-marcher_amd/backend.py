"""rm_ctx ownership for the Python host mirror: one context per GPU, created on first
use.  Raises (never falls back) when no MI355X is visible."""
import collections
import ctypes as C

import numpy as np

from . import _lib

# numpy mirror of rm_hit (72 bytes): what Context.intersect returns, one record per ray
HIT_DTYPE = np.dtype([("t", "<f8"), ("point", "<f8", (3,)), ("normal", "<f8", (3,)), ("shape", "<u4"),
                      ("element", "<u4"), ("hit", "<i4"), ("_pad", "<u4")])
assert HIT_DTYPE.itemsize == C.sizeof(_lib.rm_hit)

# The device answers as views of one buffer of rm_hit records, nothing copied: t (N,), point and normal (N, 3) float64;
# shape, element and hit (N,) int32 (torch has no uint32 arithmetic; shape indices stay below 2^31); raw: the records,
# (N, 9) float64 -- or [H][W] of them for primary_hits_device.
DeviceHits = collections.namedtuple("DeviceHits", "t point normal shape element hit raw")


def _rays(origins, directions):
    o = np.ascontiguousarray(origins, dtype=np.float64)
    d = np.ascontiguousarray(directions, dtype=np.float64)
    if o.ndim != 2 or o.shape[1] != 3 or o.shape != d.shape:
        raise ValueError("origins and directions must be two float64 arrays of shape (N, 3), got %s and %s" % (o.shape, d.shape))
    return o, d


def _ranges(ranges, n):
    """(n, 2) float64 [t_min, t_max] rows from an (n, 2) array or one (t_min, t_max) pair for every ray."""
    r = np.asarray(ranges, dtype=np.float64)
    if r.shape == (2,):
        r = np.broadcast_to(r, (n, 2))
    if r.shape != (n, 2):
        raise ValueError("ranges must be one (t_min, t_max) pair or a float64 array of shape (%d, 2), got %s" % (n, r.shape))
    return np.ascontiguousarray(r)


def _pairs(a, b, names):
    """Two (N, 3) float64 arrays of one shape: segment endpoints, or points and normals."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape != b.shape:
        raise ValueError("%s and %s must be two float64 arrays of shape (N, 3), got %s and %s" % (names[0], names[1], a.shape, b.shape))
    return a, b


def _samples(xy):
    """(N, 2) float64 sample positions (sx = column, sy = row), C-contiguous."""
    a = np.ascontiguousarray(xy, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("xy must be a float64 array of shape (N, 2), got %s" % (a.shape,))
    return a


def _shading(max_depth, background):
    """rm_shading of a ray-list radiance call."""
    if int(max_depth) != max_depth or max_depth < 0:
        raise ValueError("max_depth must be a non-negative integer, got %r" % (max_depth,))
    return _lib.rm_shading(_lib.vec3(background), int(max_depth), 0)


def _refine(n, threshold):
    """rm_refine of an adaptive anti-aliasing call: n an integer in 1..8, threshold any number but NaN."""
    if isinstance(n, bool) or int(n) != n or not 1 <= n <= 8:
        raise ValueError("n must be an integer in 1..8, got %r" % (n,))
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("threshold must not be NaN")
    return _lib.rm_refine(int(n), 0, threshold)


def _lens(aperture, focus, n_samples):
    """rm_lens of a depth-of-field call: aperture finite and >= 0, focus finite and > 0, n_samples an integer in 1..64."""
    if isinstance(n_samples, bool) or int(n_samples) != n_samples or not 1 <= n_samples <= 64:
        raise ValueError("n_samples must be an integer in 1..64, got %r" % (n_samples,))
    aperture, focus = float(aperture), float(focus)
    if not (np.isfinite(aperture) and aperture >= 0.):
        raise ValueError("aperture must be a finite number >= 0, got %r" % (aperture,))
    if not (np.isfinite(focus) and focus > 0.):
        raise ValueError("focus must be a finite number > 0, got %r" % (focus,))
    return _lib.rm_lens(aperture, focus, int(n_samples), 0)


PROGRESSIVE_MAX_SAMPLES = 65536            # RM_PROGRESSIVE_MAX_SAMPLES: samples a pixel a progressive frame can hold


def _lens_rows(table, n_samples):
    """(n_samples, 4) float64 rows (dx, dy, u, v), C-contiguous, with the conditions rm_render_lens checks."""
    t = np.ascontiguousarray(table, dtype=np.float64)
    if t.shape != (n_samples, 4):
        raise ValueError("table must be a float64 array of shape (%d, 4), got %s" % (n_samples, t.shape))
    ok = np.isfinite(t).all() and (t[:, :2] >= 0.).all() and (t[:, :2] < 1.).all() and (t[:, 2] * t[:, 2] + t[:, 3] * t[:, 3] <= 1. + 1e-12).all()
    if not ok:
        raise ValueError("table rows must be finite (dx, dy, u, v) with 0 <= dx, dy < 1 and u*u + v*v <= 1")
    return t


def _radii(radii, n_lights=None):
    """The radii of a scene's area lights as a C-contiguous float64 vector: one finite number >= 0 a light (n_lights of them
    where that is known)."""
    if isinstance(radii, (str, bytes)) or np.ndim(radii) != 1:
        raise ValueError("light radii must be a sequence of numbers, one a light, got %r" % (radii,))
    try:
        r = np.ascontiguousarray(radii, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("light radii must be numbers, got %r" % (radii,))
    if not (np.isfinite(r).all() and (r >= 0.).all()):
        raise ValueError("every light radius must be a finite number >= 0, got %r" % (list(radii),))
    if n_lights is not None and r.shape[0] != n_lights:
        raise ValueError("one radius a light: the scene has %d lights, got %d radii" % (n_lights, r.shape[0]))
    return r


def _velocities(velocities, n_shapes=None):
    """The velocities of a scene's shapes as a C-contiguous float64 array (n_shapes, 3): one finite vector a shape, None for a
    shape that stands still (n_shapes of them where that is known)."""
    if isinstance(velocities, (str, bytes)) or not hasattr(velocities, "__len__"):
        raise ValueError("velocities must be a sequence of vectors, one a shape, got %r" % (velocities,))
    v = np.zeros((len(velocities), 3), dtype=np.float64)
    for k, e in enumerate(velocities):
        if e is None:
            continue
        try:
            v[k] = (e.x, e.y, e.z) if hasattr(e, "x") else tuple(float(c) for c in e)
        except (TypeError, ValueError):
            raise ValueError("velocities[%d] must be a vector of three numbers or None, got %r" % (k, e))
    if not np.isfinite(v).all():
        raise ValueError("every velocity must be finite, got %r" % (v.tolist(),))
    if n_shapes is not None and v.shape[0] != n_shapes:
        raise ValueError("one velocity a shape: the scene has %d shapes, got %d velocities" % (n_shapes, v.shape[0]))
    return v


def _shutter(shutter):
    """The time the shutter stands open: a finite number >= 0."""
    if isinstance(shutter, bool) or not isinstance(shutter, (int, float, np.floating, np.integer)) or not np.isfinite(shutter) or shutter < 0.:
        raise ValueError("shutter must be a finite number >= 0, got %r" % (shutter,))
    return float(shutter)


def _camera_motion(velocity, turn):
    """rm_camera_motion of a camera's velocity (three finite numbers) and its yaw, pitch and roll rates (three more)."""
    try:
        v = (velocity.x, velocity.y, velocity.z) if hasattr(velocity, "x") else tuple(float(c) for c in velocity)
        t = tuple(float(c) for c in turn)
    except (TypeError, ValueError):
        raise ValueError("camera velocity and turn must be vectors of three numbers, got %r and %r" % (velocity, turn))
    if len(v) != 3 or len(t) != 3 or not np.isfinite(v + t).all():
        raise ValueError("camera velocity and turn must be three finite numbers each, got %r and %r" % (velocity, turn))
    return _lib.rm_camera_motion(_lib.rm_vec3(*(float(c) for c in v)), *t)


def _camera_rows_tensor(rows, n_rows, device):
    """A camera table as a contiguous float64 tensor (n_rows, 12) on `device`: a tensor is checked, an array is checked (finite)
    and copied over."""
    torch = _torch()
    if isinstance(rows, torch.Tensor):
        if rows.dtype != torch.float64 or rows.dim() != 2 or rows.shape[0] != n_rows or rows.shape[1] != 12 or not rows.is_contiguous():
            raise ValueError("camera_rows must be a contiguous float64 torch tensor of shape (%d, 12)" % n_rows)
        if rows.device != device:
            raise ValueError("camera_rows must live on %s, not %s" % (device, rows.device))
        return rows
    r = np.ascontiguousarray(rows, dtype=np.float64)
    if r.ndim != 2 or r.shape[0] != n_rows or r.shape[1] != 12 or not np.isfinite(r).all():
        raise ValueError("camera_rows must be a finite float64 array of shape (%d, 12), got %s" % (n_rows, r.shape))
    return torch.from_numpy(r).to(device)


def _sequence_rows(first, count):
    """first and count of a sequence call: non-negative integers with first + count <= RM_PROGRESSIVE_MAX_SAMPLES."""
    for name, v in (("first", first), ("count", count)):
        if isinstance(v, bool) or int(v) != v or v < 0:
            raise ValueError("%s must be a non-negative integer, got %r" % (name, v))
    if first + count > PROGRESSIVE_MAX_SAMPLES:
        raise ValueError("first + count must be at most %d, got %d + %d" % (PROGRESSIVE_MAX_SAMPLES, first, count))
    return int(first), int(count)


def _host_outputs(params, host_rgb, host_rgb8):
    """The two optional host outputs of a tick, each a C-contiguous array that holds the frame's whole patch rows
    -> their pointers (None where not given)."""
    need = (params.frame_height - params.frame_height % 32) * params.frame_width * 3
    out = []
    for name, a, dtype, ctype in (("host_rgb", host_rgb, np.float64, C.c_double), ("host_rgb8", host_rgb8, np.uint8, C.c_uint8)):
        if a is not None and (not isinstance(a, np.ndarray) or a.dtype != dtype or not a.flags.c_contiguous or a.size < need):
            raise ValueError("%s must be a C-contiguous %s array that holds the frame's whole patch rows" % (name, np.dtype(dtype).name))
        out.append(a.ctypes.data_as(C.POINTER(ctype)) if a is not None else None)
    return out


def _extents(lo, hi):
    """The per-shape offset extents of a swept hierarchy as two C-contiguous float64 arrays (n_shapes, 3); their numbers are the
    library's to check (it names the shape)."""
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    if lo.ndim != 2 or lo.shape[1] != 3 or hi.shape != lo.shape:
        raise ValueError("lo and hi must both have the shape (n_shapes, 3), got %s and %s" % (lo.shape, hi.shape))
    return lo, hi


def _offset_tensor(offsets, name, what, n_samples, device):
    """A light or shape offset table as a contiguous float64 tensor (n_samples, n, 3) on `device`: a tensor is checked, an array is
    checked (finite) and copied over."""
    torch = _torch()
    if isinstance(offsets, torch.Tensor):
        if offsets.dtype != torch.float64 or offsets.dim() != 3 or offsets.shape[0] != n_samples or offsets.shape[2] != 3 \
                or not offsets.is_contiguous():
            raise ValueError("%s must be a contiguous float64 torch tensor of shape (%d, %s, 3)" % (name, n_samples, what))
        if offsets.device != device:
            raise ValueError("%s must live on %s, not %s" % (name, device, offsets.device))
        return offsets
    off = np.ascontiguousarray(offsets, dtype=np.float64)
    if off.ndim != 3 or off.shape[0] != n_samples or off.shape[2] != 3 or not np.isfinite(off).all():
        raise ValueError("%s must be a finite float64 array of shape (%d, %s, 3), got %s" % (name, n_samples, what, off.shape))
    return torch.from_numpy(off).to(device)


def _strength(strength):
    """The strength of a diffuse bounce: a finite number >= 0."""
    strength = float(strength)
    if not np.isfinite(strength) or not strength >= 0.:
        raise ValueError("strength must be a finite number >= 0, got %r" % strength)
    return strength


def _bounce_tensor(bounce, n_rows, device):
    """A bounce table as a contiguous float64 tensor (n_rows, 2) on `device`: a tensor is checked, an array is checked (finite)
    and copied over."""
    torch = _torch()
    if isinstance(bounce, torch.Tensor):
        if bounce.dtype != torch.float64 or tuple(bounce.shape) != (n_rows, 2) or not bounce.is_contiguous():
            raise ValueError("bounce must be a contiguous float64 torch tensor of shape (%d, 2)" % n_rows)
        if bounce.device != device:
            raise ValueError("bounce must live on %s, not %s" % (device, bounce.device))
        return bounce
    rows = np.ascontiguousarray(bounce, dtype=np.float64)
    if rows.shape != (n_rows, 2) or not np.isfinite(rows).all():
        raise ValueError("bounce must be a finite float64 array of shape (%d, 2), got %s" % (n_rows, rows.shape))
    return torch.from_numpy(rows).to(device)


def _converge(tolerance, min_samples, max_samples, n_samples, table_rows=PROGRESSIVE_MAX_SAMPLES):
    """rm_converge of a converging frame: tolerance any number but NaN, min_samples an integer >= 0, max_samples an integer in
    n_samples..min(table_rows, RM_PROGRESSIVE_MAX_SAMPLES)."""
    tolerance = float(tolerance)
    if tolerance != tolerance:
        raise ValueError("tolerance must not be NaN")
    for name, v in (("min_samples", min_samples), ("max_samples", max_samples)):
        if isinstance(v, bool) or int(v) != v or not 0 <= v < 2 ** 32:
            raise ValueError("%s must be a non-negative integer, got %r" % (name, v))
    most = min(int(table_rows), PROGRESSIVE_MAX_SAMPLES)
    if not n_samples <= max_samples <= most:
        raise ValueError("max_samples must lie in n_samples..min(table rows, %d) = %d..%d, got %r" % (PROGRESSIVE_MAX_SAMPLES, n_samples, most, max_samples))
    return _lib.rm_converge(tolerance, int(min_samples), int(max_samples))


def _denoise(sigma_l, sigma_z, epsilon, fallback_variance, iterations, normal_squarings):
    """rm_denoise of a filter call: sigma_l and fallback_variance finite and >= 0, sigma_z and epsilon finite and > 0, iterations
    an integer in 0..5, normal_squarings one in 0..8."""
    numbers = []
    for name, v, positive in (("sigma_l", sigma_l, False), ("sigma_z", sigma_z, True), ("epsilon", epsilon, True),
                              ("fallback_variance", fallback_variance, False)):
        v = float(v)
        if not np.isfinite(v) or not (v > 0. if positive else v >= 0.):
            raise ValueError("%s must be a finite number %s 0, got %r" % (name, ">" if positive else ">=", v))
        numbers.append(v)
    for name, v, most in (("iterations", iterations, 5), ("normal_squarings", normal_squarings, 8)):
        if isinstance(v, bool) or int(v) != v or not 0 <= v <= most:
            raise ValueError("%s must be an integer in 0..%d, got %r" % (name, most, v))
    return _lib.rm_denoise(*numbers, int(iterations), int(normal_squarings))


def _reproject(sigma_z, min_normal_dot, max_history):
    """rm_reproject of a reprojection: sigma_z finite and > 0, min_normal_dot in [-1, 1), max_history an integer in
    1..PROGRESSIVE_MAX_SAMPLES."""
    sigma_z, min_normal_dot = float(sigma_z), float(min_normal_dot)
    if not np.isfinite(sigma_z) or not sigma_z > 0.:
        raise ValueError("sigma_z must be a finite number > 0, got %r" % sigma_z)
    if not -1. <= min_normal_dot < 1.:
        raise ValueError("min_normal_dot must lie in [-1, 1), got %r" % min_normal_dot)
    if isinstance(max_history, bool) or int(max_history) != max_history or not 1 <= max_history <= PROGRESSIVE_MAX_SAMPLES:
        raise ValueError("max_history must be an integer in 1..%d, got %r" % (PROGRESSIVE_MAX_SAMPLES, max_history))
    return _lib.rm_reproject(sigma_z, min_normal_dot, int(max_history), 0)


def _view(view):
    """rm_view of a camera: an rm_view, or (position, basis[, oriented]) as Context.camera() returns it."""
    if isinstance(view, _lib.rm_view):
        return view
    position, basis = view[0], view[1]
    position = position if isinstance(position, _lib.rm_vec3) else _lib.vec3(position)
    basis = basis if isinstance(basis, _lib.rm_camera_basis) else _lib.camera_basis(basis)
    return _lib.rm_view(position, basis)


def _converging_args(ctx, params, sum, stats, count, aperture, focus, n_samples, table, tolerance, min_samples, max_samples, mean, rgb8, mask,
                     workspace):
    """What Context.accumulate_converging_device and accumulate_converging_motion_device check of their common arguments (ctx: the
    context)
    -> (rm_lens, rm_converge, the table's tensor, the workspace)."""
    torch = _torch()
    h, w = params.frame_height, params.frame_width
    for name, t, dtype, shape in (("sum", sum, torch.float64, (h, w, 3)), ("stats", stats, torch.float64, (h, w, 2)),
                                  ("count", count, torch.int32, (h, w)), ("mean", mean, torch.float64, (h, w, 3)),
                                  ("rgb8", rgb8, torch.uint8, (h, w, 3)), ("mask", mask, torch.uint8, (h, w))):
        if t is None and name in ("mean", "rgb8", "mask"):
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s torch tensor of shape %s" % (name, dtype, shape))
        if t.device.type != "cuda" or t.device.index != ctx.device:
            raise ValueError("%s must live on cuda:%d (the context's device), not %s" % (name, ctx.device, t.device))
    if mean is not None and mean.data_ptr() == sum.data_ptr():
        raise ValueError("mean must not be the sum's own tensor")
    lens = _lens(aperture, focus, n_samples)
    if isinstance(table, torch.Tensor):
        if table.dtype != torch.float64 or table.dim() != 2 or table.shape[1] != 4 or not table.is_contiguous():
            raise ValueError("table must be a contiguous float64 torch tensor of shape (rows, 4)")
        if table.device != sum.device:
            raise ValueError("table must live on %s, not %s" % (sum.device, table.device))
    else:
        rows = np.asarray(table)
        table = torch.from_numpy(_lens_rows(rows, rows.shape[0] if rows.ndim == 2 else 0)).to(sum.device)
    conv = _converge(tolerance, min_samples, max_samples, lens.n_samples, table.shape[0])
    need = Context.converge_workspace(ctx, params) // 4
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.int32, device=sum.device)
    elif not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.int32 or workspace.dim() != 1 or workspace.shape[0] < need \
            or not workspace.is_contiguous() or workspace.device != sum.device:
        raise ValueError("workspace must be a contiguous int32 torch tensor of at least %d words on %s" % (need, sum.device))
    return lens, conv, table, workspace


def _accumulate_args(device, params, sum, aperture, focus, table, n_before, mean, rgb8):
    """What accumulate_lens_device and accumulate_soft_device check of their common arguments -> (rm_lens, the table's tensor)."""
    torch = _torch()
    h, w = params.frame_height, params.frame_width
    for name, t, dtype in (("sum", sum, torch.float64), ("mean", mean, torch.float64), ("rgb8", rgb8, torch.uint8)):
        if t is None and name != "sum":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (h, w, 3) or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s torch tensor of shape %s" % (name, dtype, (h, w, 3)))
        if t.device.type != "cuda" or t.device.index != device:
            raise ValueError("%s must live on cuda:%d (the context's device), not %s" % (name, device, t.device))
    if mean is not None and mean.data_ptr() == sum.data_ptr():
        raise ValueError("mean must not be the sum's own tensor")
    if isinstance(n_before, bool) or int(n_before) != n_before or n_before < 0:
        raise ValueError("n_before must be a non-negative integer, got %r" % (n_before,))
    if isinstance(table, torch.Tensor):
        if table.dtype != torch.float64 or table.dim() != 2 or table.shape[1] != 4 or not table.is_contiguous():
            raise ValueError("table must be a contiguous float64 torch tensor of shape (n_samples, 4)")
        if table.device != sum.device:
            raise ValueError("table must live on %s, not %s" % (sum.device, table.device))
        lens = _lens(aperture, focus, table.shape[0])
    else:
        rows = np.asarray(table)
        lens = _lens(aperture, focus, rows.shape[0] if rows.ndim == 2 else 0)
        table = torch.from_numpy(_lens_rows(rows, lens.n_samples)).to(sum.device)
    if n_before + lens.n_samples > PROGRESSIVE_MAX_SAMPLES:
        raise ValueError("n_before + n_samples must be at most %d, got %d + %d" % (PROGRESSIVE_MAX_SAMPLES, n_before, lens.n_samples))
    return lens, table


def _device_hits(raw):
    """DeviceHits over a float64 tensor whose last dimension is one rm_hit (9 words)."""
    ints = raw.view(_torch().int32)                       # 18 int32 a record: shape, element, hit are 14, 15, 16
    return DeviceHits(raw[..., 0], raw[..., 1:4], raw[..., 4:7], ints[..., 14], ints[..., 15], ints[..., 16], raw)


def _torch():
    import torch
    return torch


class Swept:
    """A swept hierarchy of a context's uploaded scene (Context.swept).  close() releases it (waits for the device)."""

    def __init__(self, ctx, ptr):
        self.ctx, self.ptr = ctx, ptr

    def close(self):
        if self.ptr is not None and self.ctx.ptr is not None:
            self.ctx.L.rm_swept_free(self.ctx.ptr, self.ptr)
        self.ptr = None


class Context:
    def __init__(self, device=0):
        self.L = _lib.lib()
        p = C.c_void_p()
        _lib.check(self.L.rm_init(int(device), C.byref(p)))
        self.ptr = p
        self.device = int(device)
        self._uploaded = None   # keeps the SceneHandle of the uploaded scene alive

    def close(self):
        if self.ptr:
            self.L.rm_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, desc_or_handle):
        desc = desc_or_handle.desc() if hasattr(desc_or_handle, "desc") else desc_or_handle
        _lib.check(self.L.rm_scene_upload(self.ptr, C.byref(desc)), self.ptr)
        self._uploaded = desc_or_handle

    def uploads(self):
        """(calls of rm_scene_upload, copies it had to make)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        _lib.check(self.L.rm_scene_uploads(self.ptr, C.byref(a), C.byref(b)), self.ptr)
        return a.value, b.value

    def set_camera(self, cam):
        _lib.check(self.L.rm_camera_update(self.ptr, _lib.vec3(cam)), self.ptr)

    # ---- the oriented camera (include/rusty_marcher_amd.h, "the oriented camera") ----
    def orient(self, basis=None):
        """View direction of every later render and pixel query: an rm_camera_basis or (right, up, forward); None resets to
        the reference's fixed view (down -z, +y up)."""
        b = None if basis is None else C.byref(_lib.camera_basis(basis))
        _lib.check(self.L.rm_camera_orient(self.ptr, b), self.ptr)

    def look_at(self, eye, target, up=(0., 1., 0.)):
        """Camera at `eye`, looking at `target`."""
        _lib.check(self.L.rm_camera_look_at(self.ptr, _lib.vec3(eye), _lib.vec3(target), _lib.vec3(up)), self.ptr)

    def camera(self):
        """(position, basis, oriented) the context renders with."""
        pos, b, on = _lib.rm_vec3(), _lib.rm_camera_basis(), C.c_int(0)
        _lib.check(self.L.rm_camera_get(self.ptr, C.byref(pos), C.byref(b), C.byref(on)), self.ptr)
        return pos, b, bool(on.value)

    def render(self, params, host_array=None):
        t = _lib.rm_timing()
        ptr = host_array.ctypes.data_as(C.POINTER(C.c_double)) if host_array is not None else None
        _lib.check(self.L.rm_render(self.ptr, C.byref(params), ptr, C.byref(t)), self.ptr)
        return t

    @staticmethod
    def row_pointers(rows):
        """double *const * for rm_render_rows / rm_fetch_rows: one pointer per row, each row a
        float64 array of its own (the reference's Vec<Vec<Vec3f>>, framebuffer.rs:6-22); None for
        rows the call must not touch."""
        arr = (C.POINTER(C.c_double) * len(rows))()
        for i, r in enumerate(rows):
            if r is not None:
                arr[i] = r.ctypes.data_as(C.POINTER(C.c_double))
        return arr

    def render_rows(self, params, rows):
        """Renderer::render into rows of rows (rm_render_rows)."""
        t = _lib.rm_timing()
        _lib.check(self.L.rm_render_rows(self.ptr, C.byref(params), self.row_pointers(rows), C.byref(t)), self.ptr)
        return t

    def render_display(self, params, host_u8):
        """Renderer::render with the f64 frame left on the device: only fb.to_vec() comes back."""
        t = _lib.rm_timing()
        _lib.check(self.L.rm_render_display(self.ptr, C.byref(params), host_u8.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            C.byref(t)), self.ptr)
        return t

    def fetch_rows(self, rows, patch_row_begin=0, patch_row_end=0, width=None):
        """`rows`: the FrameBuffer's rows, all of them (None for rows not to be touched): their count is its height,
        a row's length / 3 its width (`width` where every row is None)."""
        w = width if width is not None else next((r.size // 3 for r in rows if r is not None), 0)
        for r in rows:
            if r is not None and r.size != w * 3:
                raise ValueError("fetch_rows: a row of %d doubles in a FrameBuffer %d wide" % (r.size, w))
        _lib.check(self.L.rm_fetch_rows(self.ptr, self.row_pointers(rows), w, len(rows), patch_row_begin, patch_row_end), self.ptr)

    def tile_stats(self, stream=None):
        """(tiles of the last render launch, tiles the classification listed for rendering)"""
        a, b = C.c_uint32(0), C.c_uint32(0)
        _lib.check(self.L.rm_tile_stats(self.ptr, C.c_void_p(stream) if stream else None, C.byref(a), C.byref(b)), self.ptr)
        return a.value, b.value

    def launch_stats(self):
        """(workgroups of the last render launch, patches handed to its sky tail)"""
        a, b = C.c_uint32(0), C.c_uint32(0)
        _lib.check(self.L.rm_launch_stats(self.ptr, C.byref(a), C.byref(b)), self.ptr)
        return a.value, b.value

    def hostio_stats(self):
        """What the last host-bound call moved: bytes over the link, patches, patches sent, threads."""
        b, p, s, t = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        _lib.check(self.L.rm_hostio_stats(self.ptr, C.byref(b), C.byref(p), C.byref(s), C.byref(t)), self.ptr)
        return {"bytes_copied": b.value, "patches": p.value, "patches_sent": s.value, "threads": t.value}

    def render_device(self, params, device_ptr, stream=None):
        _lib.check(self.L.rm_render_device(self.ptr, C.byref(params), C.c_void_p(device_ptr),
                                           C.c_void_p(stream) if stream else None), self.ptr)

    def render_device_u8(self, params, device_ptr, device_ptr8, stream=None):
        _lib.check(self.L.rm_render_device_u8(self.ptr, C.byref(params), C.c_void_p(device_ptr),
                                              C.c_void_p(device_ptr8), C.c_void_p(stream) if stream else None),
                   self.ptr)

    # ---- ray queries (include/rusty_marcher_amd.h, "ray queries") ----
    def intersect(self, origins, directions, ranges=None):
        """find_closest_intersect (shapes.rs:110-143) of N rays of the caller's own: (N, 3) float64 origins and unit
        directions -> a structured array of N rm_hit records (HIT_DTYPE), written by the library in place.
        ranges: an (N, 2) array of [t_min, t_max], or one pair for every ray: only hits in the range count
        (rm_intersect_rays_ranged)."""
        o, d = _rays(origins, directions)
        out = np.zeros(o.shape[0], dtype=HIT_DTYPE)
        V = C.POINTER(_lib.rm_vec3)
        if ranges is not None:
            r = _ranges(ranges, o.shape[0])
            _lib.check(self.L.rm_intersect_rays_ranged(self.ptr, o.ctypes.data_as(V), d.ctypes.data_as(V),
                                                       r.ctypes.data_as(C.POINTER(_lib.rm_range)), o.shape[0],
                                                       out.ctypes.data_as(C.POINTER(_lib.rm_hit))), self.ptr)
            return out
        _lib.check(self.L.rm_intersect_rays(self.ptr, o.ctypes.data_as(V), d.ctypes.data_as(V), o.shape[0],
                                            out.ctypes.data_as(C.POINTER(_lib.rm_hit))), self.ptr)
        return out

    def occluded(self, origins, directions, ranges=None):
        """intersect_shape_set (shapes.rs:92-108) of N rays: a bool array, True where anything lies along the ray
        (no maximum distance, as in the reference) -- or, with `ranges` (as for intersect), within the ray's range."""
        o, d = _rays(origins, directions)
        out = np.zeros(o.shape[0], dtype=np.uint8)
        V = C.POINTER(_lib.rm_vec3)
        if ranges is not None:
            r = _ranges(ranges, o.shape[0])
            _lib.check(self.L.rm_occluded_rays_ranged(self.ptr, o.ctypes.data_as(V), d.ctypes.data_as(V),
                                                      r.ctypes.data_as(C.POINTER(_lib.rm_range)), o.shape[0],
                                                      out.ctypes.data_as(C.POINTER(C.c_uint8))), self.ptr)
            return out.view(np.bool_)
        _lib.check(self.L.rm_occluded_rays(self.ptr, o.ctypes.data_as(V), d.ctypes.data_as(V), o.shape[0],
                                           out.ctypes.data_as(C.POINTER(C.c_uint8))), self.ptr)
        return out.view(np.bool_)

    def _device_rays(self, origins, directions, names=("origins", "directions")):
        torch = _torch()
        for name, t in zip(names, (origins, directions)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != 3:
                raise ValueError("%s must be a float64 torch tensor of shape (N, 3)" % name)
            if t.device.type != "cuda" or t.device.index != self.device:
                raise ValueError("%s must live on cuda:%d (the context's device), not %s" % (name, self.device, t.device))
            if not t.is_contiguous():
                raise ValueError("%s must be contiguous" % name)
        if origins.shape != directions.shape:
            raise ValueError("%s %s and %s %s differ in shape" % (names[0], tuple(origins.shape), names[1], tuple(directions.shape)))
        return origins.shape[0]

    def _device_ranges(self, ranges, like):
        """A contiguous (N, 2) float64 tensor next to `like` from one, or from one (t_min, t_max) pair."""
        torch = _torch()
        n = like.shape[0]
        if not isinstance(ranges, torch.Tensor):
            r = np.asarray(ranges, dtype=np.float64)
            if r.shape != (2,):
                raise ValueError("ranges must be one (t_min, t_max) pair or a float64 torch tensor of shape (%d, 2)" % n)
            return torch.from_numpy(np.ascontiguousarray(np.broadcast_to(r, (n, 2)))).to(like.device)
        if ranges.dtype != torch.float64 or tuple(ranges.shape) != (n, 2) or not ranges.is_contiguous():
            raise ValueError("ranges must be a contiguous float64 torch tensor of shape (%d, 2), got %s" % (n, tuple(ranges.shape)))
        if ranges.device != like.device:
            raise ValueError("ranges must live on %s, not %s" % (like.device, ranges.device))
        return ranges

    def _stream(self, stream):
        """The HIP stream of a call: `stream` (a torch stream or a raw handle), else torch's current stream."""
        torch = _torch()
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)

    def intersect_device(self, origins, directions, stream=None, ranges=None):
        """intersect() on torch tensors of the context's device, asynchronous on `stream` (torch's current one by
        default): DeviceHits, no copy to the host.  ranges: an (N, 2) tensor there, or one pair."""
        torch = _torch()
        n = self._device_rays(origins, directions)
        raw = torch.empty((n, 9), dtype=torch.float64, device=origins.device)
        if ranges is not None:
            r = self._device_ranges(ranges, origins)
            _lib.check(self.L.rm_intersect_rays_ranged_device(self.ptr, C.c_void_p(origins.data_ptr()), C.c_void_p(directions.data_ptr()),
                                                              C.c_void_p(r.data_ptr()), n, C.c_void_p(raw.data_ptr()),
                                                              C.c_void_p(self._stream(stream))), self.ptr)
            return _device_hits(raw)
        _lib.check(self.L.rm_intersect_rays_device(self.ptr, C.c_void_p(origins.data_ptr()), C.c_void_p(directions.data_ptr()),
                                                   n, C.c_void_p(raw.data_ptr()), C.c_void_p(self._stream(stream))), self.ptr)
        return _device_hits(raw)

    def occluded_device(self, origins, directions, stream=None, ranges=None):
        """occluded() on torch tensors of the context's device: a bool tensor there, asynchronous on `stream`."""
        torch = _torch()
        n = self._device_rays(origins, directions)
        out = torch.empty((n,), dtype=torch.uint8, device=origins.device)
        if ranges is not None:
            r = self._device_ranges(ranges, origins)
            _lib.check(self.L.rm_occluded_rays_ranged_device(self.ptr, C.c_void_p(origins.data_ptr()), C.c_void_p(directions.data_ptr()),
                                                             C.c_void_p(r.data_ptr()), n, C.c_void_p(out.data_ptr()),
                                                             C.c_void_p(self._stream(stream))), self.ptr)
            return out.view(torch.bool)
        _lib.check(self.L.rm_occluded_rays_device(self.ptr, C.c_void_p(origins.data_ptr()), C.c_void_p(directions.data_ptr()),
                                                  n, C.c_void_p(out.data_ptr()), C.c_void_p(self._stream(stream))), self.ptr)
        return out.view(torch.bool)

    def visible(self, a, b, skin=0.):
        """rm_visible_segments: can a[i] see b[i]?  (N, 3) float64 endpoints -> a bool array, True where nothing lies on the
        segment between `skin` and its length less `skin` (the guard against the surfaces the endpoints lie on)."""
        a, b = _pairs(a, b, ("a", "b"))
        out = np.zeros(a.shape[0], dtype=np.uint8)
        V = C.POINTER(_lib.rm_vec3)
        _lib.check(self.L.rm_visible_segments(self.ptr, a.ctypes.data_as(V), b.ctypes.data_as(V), a.shape[0], float(skin),
                                              out.ctypes.data_as(C.POINTER(C.c_uint8))), self.ptr)
        return out.view(np.bool_)

    def visible_device(self, a, b, skin=0., stream=None):
        """visible() on torch tensors of the context's device: a bool tensor there, asynchronous on `stream`."""
        torch = _torch()
        n = self._device_rays(a, b, ("a", "b"))
        out = torch.empty((n,), dtype=torch.uint8, device=a.device)
        _lib.check(self.L.rm_visible_segments_device(self.ptr, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), n, float(skin),
                                                     C.c_void_p(out.data_ptr()), C.c_void_p(self._stream(stream))), self.ptr)
        return out.view(torch.bool)

    def n_lights(self):
        """Lights of the uploaded scene (what sizes lights_visible's answer)."""
        if self._uploaded is None:
            raise _lib.BackendError(_lib.RM_ERR_NO_SCENE, "no scene uploaded")
        d = self._uploaded.desc() if hasattr(self._uploaded, "desc") else self._uploaded
        return int(d.n_lights)

    def lights_visible(self, points, normals, clipped=False):
        """rm_lights_visible: which lights reach each surface point -- an (N, n_lights) bool array.  clipped=False: the
        decision direct_lighting takes (renderer.rs:166-174), a shape behind the light shadows; True: the shadow ray ends
        at the light."""
        p, nrm = _pairs(points, normals, ("points", "normals"))
        nl = self.n_lights()
        out = np.zeros((p.shape[0], nl), dtype=np.uint8)
        V = C.POINTER(_lib.rm_vec3)
        _lib.check(self.L.rm_lights_visible(self.ptr, p.ctypes.data_as(V), nrm.ctypes.data_as(V), p.shape[0], nl,
                                            _lib.RM_LIGHTS_CLIPPED if clipped else _lib.RM_LIGHTS_AS_RENDERED,
                                            out.ctypes.data_as(C.POINTER(C.c_uint8))), self.ptr)
        return out.view(np.bool_)

    def lights_visible_device(self, points, normals, clipped=False, stream=None):
        """lights_visible() on torch tensors of the context's device: an (N, n_lights) bool tensor there."""
        torch = _torch()
        n = self._device_rays(points, normals, ("points", "normals"))
        nl = self.n_lights()
        out = torch.empty((n, nl), dtype=torch.uint8, device=points.device)
        _lib.check(self.L.rm_lights_visible_device(self.ptr, C.c_void_p(points.data_ptr()), C.c_void_p(normals.data_ptr()), n, nl,
                                                   _lib.RM_LIGHTS_CLIPPED if clipped else _lib.RM_LIGHTS_AS_RENDERED,
                                                   C.c_void_p(out.data_ptr()), C.c_void_p(self._stream(stream))), self.ptr)
        return out.view(torch.bool)

    # ---- radiance queries (include/rusty_marcher_amd.h, "radiance queries") ----
    def radiance(self, origins, directions, max_depth=3, background=(.1, .1, .1)):
        """rm_radiance_rays: cast_ray (renderer.rs:254-309) along N rays of the caller's own, (N, 3) float64 origins and
        unit directions -> (N, 3) float64 radiance.  A ray that leaves the scene returns exactly zero."""
        o, d = _rays(origins, directions)
        sh = _shading(max_depth, background)
        out = np.zeros((o.shape[0], 3), dtype=np.float64)
        V = C.POINTER(_lib.rm_vec3)
        _lib.check(self.L.rm_radiance_rays(self.ptr, o.ctypes.data_as(V), d.ctypes.data_as(V), o.shape[0], C.byref(sh),
                                           out.ctypes.data_as(V)), self.ptr)
        return out

    def radiance_device(self, origins, directions, max_depth=3, background=(.1, .1, .1), stream=None):
        """radiance() on torch tensors of the context's device, asynchronous on `stream` (torch's current one by
        default): an (N, 3) float64 tensor there."""
        torch = _torch()
        n = self._device_rays(origins, directions)
        sh = _shading(max_depth, background)
        out = torch.empty((n, 3), dtype=torch.float64, device=origins.device)
        _lib.check(self.L.rm_radiance_rays_device(self.ptr, C.c_void_p(origins.data_ptr()), C.c_void_p(directions.data_ptr()), n,
                                                  C.byref(sh), C.c_void_p(out.data_ptr()), C.c_void_p(self._stream(stream))), self.ptr)
        return out

    def radiance_samples(self, params, xy):
        """rm_radiance_samples: the radiance at N real-valued positions (sx = column, sy = row) of the frame `params`
        describes, from the context's camera; depth cap and background are params'.  (N, 2) float64 -> (N, 3) float64."""
        a = _samples(xy)
        out = np.zeros((a.shape[0], 3), dtype=np.float64)
        _lib.check(self.L.rm_radiance_samples(self.ptr, C.byref(params), a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[0],
                                              out.ctypes.data_as(C.POINTER(_lib.rm_vec3))), self.ptr)
        return out

    def radiance_samples_device(self, params, xy, stream=None):
        """radiance_samples() on a contiguous (N, 2) float64 torch tensor of the context's device, asynchronous on
        `stream`: an (N, 3) float64 tensor there."""
        torch = _torch()
        if not isinstance(xy, torch.Tensor) or xy.dtype != torch.float64 or xy.dim() != 2 or xy.shape[1] != 2:
            raise ValueError("xy must be a float64 torch tensor of shape (N, 2)")
        if xy.device.type != "cuda" or xy.device.index != self.device:
            raise ValueError("xy must live on cuda:%d (the context's device), not %s" % (self.device, xy.device))
        if not xy.is_contiguous():
            raise ValueError("xy must be contiguous")
        n = xy.shape[0]
        out = torch.empty((n, 3), dtype=torch.float64, device=xy.device)
        _lib.check(self.L.rm_radiance_samples_device(self.ptr, C.byref(params), C.c_void_p(xy.data_ptr()), n,
                                                     C.c_void_p(out.data_ptr()), C.c_void_p(self._stream(stream))), self.ptr)
        return out

    # ---- adaptive anti-aliasing (include/rusty_marcher_amd.h, "adaptive anti-aliasing") ----
    def refine_workspace(self, params):
        """rm_refine_workspace: bytes of device memory refine_device needs for `params`."""
        b = C.c_size_t(0)
        _lib.check(self.L.rm_refine_workspace(C.byref(params), C.byref(b)), None)
        return b.value

    def refine_device(self, params, frame_tensor, n, threshold, mask=None, stream=None):
        """rm_refine_device: refines in place the frame render_device wrote into `frame_tensor` -- a contiguous float64
        tensor of shape (frame_height, frame_width, 3) on the context's device -- with n x n samples for every pixel whose
        contrast is > threshold; asynchronous on `stream` (torch's current one by default).  mask: optionally a contiguous
        uint8 tensor (frame_height, frame_width) there, which gets 1 / 0 per pixel of the whole patch rows.  -> the workspace,
        an int32 tensor: ws[0] is the number of refined pixels, ws[1:1 + ws[0]] their indices y * frame_width + x."""
        torch = _torch()
        r = _refine(n, threshold)
        h, w = params.frame_height, params.frame_width
        for name, t, dtype, shape in (("frame_tensor", frame_tensor, torch.float64, (h, w, 3)), ("mask", mask, torch.uint8, (h, w))):
            if t is None and name == "mask":
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("%s must be a contiguous %s torch tensor of shape %s" % (name, dtype, shape))
            if t.device.type != "cuda" or t.device.index != self.device:
                raise ValueError("%s must live on cuda:%d (the context's device), not %s" % (name, self.device, t.device))
        ws = torch.empty((self.refine_workspace(params) // 4,), dtype=torch.int32, device=frame_tensor.device)
        _lib.check(self.L.rm_refine_device(self.ptr, C.byref(params), C.byref(r), C.c_void_p(frame_tensor.data_ptr()),
                                           C.c_void_p(ws.data_ptr()), C.c_void_p(mask.data_ptr()) if mask is not None else None,
                                           C.c_void_p(self._stream(stream))), self.ptr)
        return ws

    def render_antialiased(self, params, host_array, n, threshold):
        """rm_render_antialiased: render(), then n x n samples for every pixel whose contrast is > threshold, then the copy
        into host_array.  -> (rm_timing, number of refined pixels)."""
        r = _refine(n, threshold)
        t, count = _lib.rm_timing(), C.c_uint32(0)
        ptr = host_array.ctypes.data_as(C.POINTER(C.c_double)) if host_array is not None else None
        _lib.check(self.L.rm_render_antialiased(self.ptr, C.byref(params), C.byref(r), ptr, C.byref(count), C.byref(t)), self.ptr)
        return t, count.value

    # ---- thin-lens camera (include/rusty_marcher_amd.h, "thin-lens camera") ----
    def lens_table(self, n_samples):
        """rm_lens_table: the library's sample table for n_samples rays a pixel, (n_samples, 4) float64 rows (dx, dy, u, v).
        Host arithmetic: needs neither a context nor a GPU."""
        if isinstance(n_samples, bool) or int(n_samples) != n_samples or not 1 <= n_samples <= 64:
            raise ValueError("n_samples must be an integer in 1..64, got %r" % (n_samples,))
        t = np.zeros((int(n_samples), 4), dtype=np.float64)
        _lib.check(self.L.rm_lens_table(int(n_samples), t.ctypes.data_as(C.POINTER(C.c_double))), None)
        return t

    def render_lens_device(self, params, frame_tensor, aperture, focus, table, stream=None):
        """rm_render_lens_device: a depth-of-field frame into `frame_tensor` -- a contiguous float64 tensor of shape
        (frame_height, frame_width, 3) on the context's device --, table.shape[0] rays a pixel through a lens of radius
        `aperture` that is sharp at the distance `focus`; asynchronous on `stream` (torch's current one by default).  table:
        a contiguous float64 tensor (n_samples, 4) there, or an array, which is checked and copied over.  -> the table's tensor."""
        torch = _torch()
        h, w = params.frame_height, params.frame_width
        if not isinstance(frame_tensor, torch.Tensor) or frame_tensor.dtype != torch.float64 or tuple(frame_tensor.shape) != (h, w, 3) \
                or not frame_tensor.is_contiguous():
            raise ValueError("frame_tensor must be a contiguous float64 torch tensor of shape %s" % ((h, w, 3),))
        if frame_tensor.device.type != "cuda" or frame_tensor.device.index != self.device:
            raise ValueError("frame_tensor must live on cuda:%d (the context's device), not %s" % (self.device, frame_tensor.device))
        if isinstance(table, torch.Tensor):
            if table.dtype != torch.float64 or table.dim() != 2 or table.shape[1] != 4 or not table.is_contiguous():
                raise ValueError("table must be a contiguous float64 torch tensor of shape (n_samples, 4)")
            if table.device != frame_tensor.device:
                raise ValueError("table must live on %s, not %s" % (frame_tensor.device, table.device))
            lens = _lens(aperture, focus, table.shape[0])
        else:
            rows = np.asarray(table)
            lens = _lens(aperture, focus, rows.shape[0] if rows.ndim == 2 else 0)
            table = torch.from_numpy(_lens_rows(rows, lens.n_samples)).to(frame_tensor.device)
        _lib.check(self.L.rm_render_lens_device(self.ptr, C.byref(params), C.byref(lens), C.c_void_p(table.data_ptr()),
                                                C.c_void_p(frame_tensor.data_ptr()), C.c_void_p(self._stream(stream))), self.ptr)
        return table

    def render_lens(self, params, host_array, aperture, focus, table):
        """rm_render_lens: the depth-of-field frame of render_lens_device with a host table, (n_samples, 4) float64, copied
        into host_array (the whole patch rows).  -> rm_timing."""
        rows = np.asarray(table)
        lens = _lens(aperture, focus, rows.shape[0] if rows.ndim == 2 else 0)
        t = _lens_rows(rows, lens.n_samples)
        if not isinstance(host_array, np.ndarray) or host_array.dtype != np.float64 or not host_array.flags.c_contiguous \
                or host_array.size < (params.frame_height - params.frame_height % 32) * params.frame_width * 3:
            raise ValueError("host_array must be a C-contiguous float64 array that holds the frame's whole patch rows")
        timing = _lib.rm_timing()
        _lib.check(self.L.rm_render_lens(self.ptr, C.byref(params), C.byref(lens), t.ctypes.data_as(C.POINTER(C.c_double)),
                                         host_array.ctypes.data_as(C.POINTER(C.c_double)), C.byref(timing)), self.ptr)
        return timing

    # ---- progressive frames (include/rusty_marcher_amd.h, "progressive frames") ----
    def lens_sequence(self, first, count):
        """rm_lens_sequence: rows first .. first + count - 1 of the library's unbounded sample sequence, (count, 4) float64 rows
        (dx, dy, u, v); every prefix is well spread.  Host arithmetic: needs neither a context nor a GPU."""
        first, count = _sequence_rows(first, count)
        t = np.zeros((int(count), 4), dtype=np.float64)
        _lib.check(self.L.rm_lens_sequence(int(first), int(count), t.ctypes.data_as(C.POINTER(C.c_double))), None)
        return t

    def accumulate_lens_device(self, params, sum, aperture, focus, table, n_before, mean=None, rgb8=None, stream=None):
        """rm_accumulate_lens_device: table.shape[0] more lens samples a pixel added to `sum`, which holds n_before a pixel
        already (0: it is not read) -- a contiguous float64 tensor of shape (frame_height, frame_width, 3) on the context's
        device.  mean: optionally a float64 tensor of that shape for sum / (n_before + n_samples); rgb8: optionally a uint8
        tensor of that shape for the mean's display bytes.  Asynchronous on `stream` (torch's current one by default).
        table: as render_lens_device's.  -> the table's tensor."""
        lens, table = _accumulate_args(self.device, params, sum, aperture, focus, table, n_before, mean, rgb8)
        _lib.check(self.L.rm_accumulate_lens_device(self.ptr, C.byref(params), C.byref(lens), C.c_void_p(table.data_ptr()), int(n_before),
                                                    C.c_void_p(sum.data_ptr()), C.c_void_p(mean.data_ptr()) if mean is not None else None,
                                                    C.c_void_p(rgb8.data_ptr()) if rgb8 is not None else None,
                                                    C.c_void_p(self._stream(stream))), self.ptr)
        return table

    def render_progressive(self, params, aperture, focus, n_samples, restart=False, host_rgb=None, host_rgb8=None):
        """rm_render_progressive: n_samples more samples a pixel of the library's sequence into the frame the context keeps
        for the standing view -- begun again when `restart` is set or the view, the lens or the scene changed --, its mean
        copied into host_rgb (float64) and its display bytes into host_rgb8 (uint8) where given: C-contiguous arrays that hold
        the frame's whole patch rows.  -> (rm_timing, samples a pixel in the frame now)."""
        lens = _lens(aperture, focus, n_samples)
        host = _host_outputs(params, host_rgb, host_rgb8)
        timing, total = _lib.rm_timing(), C.c_uint32(0)
        _lib.check(self.L.rm_render_progressive(self.ptr, C.byref(params), C.byref(lens), 1 if restart else 0,
                                                *host, C.byref(total), C.byref(timing)), self.ptr)
        return timing, total.value

    # ---- area lights (include/rusty_marcher_amd.h, "area lights") ----
    def light_sequence(self, first, count, radii):
        """rm_light_sequence: rows first .. first + count - 1 of the library's light offset sequence for lights of the radii
        `radii`, (count, len(radii), 3) float64: row s moves light l to a point of the sphere of radius radii[l] about its
        position.  Host arithmetic: needs neither a context nor a GPU."""
        first, count = _sequence_rows(first, count)
        r = _radii(radii)
        off = np.zeros((int(count), r.shape[0], 3), dtype=np.float64)
        _lib.check(self.L.rm_light_sequence(int(first), int(count), r.ctypes.data_as(C.POINTER(C.c_double)), r.shape[0],
                                            off.ctypes.data_as(C.POINTER(C.c_double))), None)
        return off

    def accumulate_soft_device(self, params, sum, aperture, focus, table, offsets, n_before, mean=None, rgb8=None, stream=None):
        """rm_accumulate_soft_device: accumulate_lens_device with a light offset table -- sample row s sees light l at its
        position + offsets[s][l].  offsets: a contiguous float64 tensor (n_samples, n_lights, 3) on the context's device, or
        an array, which is checked (finite) and copied over; n_lights must be the uploaded scene's.
        -> (the table's tensor, the offsets' tensor)."""
        lens, table = _accumulate_args(self.device, params, sum, aperture, focus, table, n_before, mean, rgb8)
        offsets = _offset_tensor(offsets, "offsets", "n_lights", lens.n_samples, sum.device)
        n_lights = int(offsets.shape[1])
        _lib.check(self.L.rm_accumulate_soft_device(self.ptr, C.byref(params), C.byref(lens), C.c_void_p(table.data_ptr()),
                                                    C.c_void_p(offsets.data_ptr()) if n_lights > 0 else None, n_lights, int(n_before),
                                                    C.c_void_p(sum.data_ptr()), C.c_void_p(mean.data_ptr()) if mean is not None else None,
                                                    C.c_void_p(rgb8.data_ptr()) if rgb8 is not None else None,
                                                    C.c_void_p(self._stream(stream))), self.ptr)
        return table, offsets

    def render_progressive_soft(self, params, radii, aperture, focus, n_samples, restart=False, host_rgb=None, host_rgb8=None):
        """rm_render_progressive_soft: render_progressive with area lights -- light l is sampled on the sphere of radius radii[l]
        about its position, one radius for every light of the uploaded scene.  The frame begins again when a radius changes or
        the caller switches between this call and render_progressive, and on everything that begins it again there.
        -> (rm_timing, samples a pixel in the frame now)."""
        lens = _lens(aperture, focus, n_samples)
        r = _radii(radii)
        host = _host_outputs(params, host_rgb, host_rgb8)
        timing, total = _lib.rm_timing(), C.c_uint32(0)
        _lib.check(self.L.rm_render_progressive_soft(self.ptr, C.byref(params), C.byref(lens), r.ctypes.data_as(C.POINTER(C.c_double)),
                                                     r.shape[0], 1 if restart else 0,
                                                     *host, C.byref(total), C.byref(timing)), self.ptr)
        return timing, total.value

    # ---- moving spheres (include/rusty_marcher_amd.h, "moving spheres") ----
    def motion_sequence(self, first, count, velocities, shutter):
        """rm_motion_sequence: rows first .. first + count - 1 of the library's shape offset sequence for shapes of the velocities
        `velocities` and a shutter open for `shutter`, (count, len(velocities), 3) float64: row s moves shape k by velocities[k]
        times the row's time within the shutter.  Host arithmetic: needs neither a context nor a GPU."""
        first, count = _sequence_rows(first, count)
        v, shutter = _velocities(velocities), _shutter(shutter)
        off = np.zeros((int(count), v.shape[0], 3), dtype=np.float64)
        _lib.check(self.L.rm_motion_sequence(int(first), int(count), v.ctypes.data_as(C.POINTER(_lib.rm_vec3)), v.shape[0], shutter,
                                             off.ctypes.data_as(C.POINTER(C.c_double))), None)
        return off

    def accumulate_motion_device(self, params, sum, aperture, focus, table, light_offsets, shape_offsets, n_before, mean=None, rgb8=None,
                                 stream=None):
        """rm_accumulate_motion_device: accumulate_soft_device with a shape offset table as well -- sample row s sees the sphere
        that is shape k of the scene at its centre + shape_offsets[s][k], in every hit test, shadow test and normal.
        light_offsets: (n_samples, n_lights, 3), zeros for point lights; shape_offsets: (n_samples, n_shapes, 3), rows of shapes
        that are not spheres are not read.  Each a contiguous float64 tensor on the context's device, or an array, which is
        checked (finite) and copied over; n_lights and n_shapes must be the uploaded scene's.
        -> (the table's tensor, the light offsets' tensor, the shape offsets' tensor)."""
        lens, table = _accumulate_args(self.device, params, sum, aperture, focus, table, n_before, mean, rgb8)
        light_offsets = _offset_tensor(light_offsets, "light_offsets", "n_lights", lens.n_samples, sum.device)
        shape_offsets = _offset_tensor(shape_offsets, "shape_offsets", "n_shapes", lens.n_samples, sum.device)
        n_lights, n_shapes = int(light_offsets.shape[1]), int(shape_offsets.shape[1])
        _lib.check(self.L.rm_accumulate_motion_device(self.ptr, C.byref(params), C.byref(lens), C.c_void_p(table.data_ptr()),
                                                      C.c_void_p(light_offsets.data_ptr()) if n_lights > 0 else None, n_lights,
                                                      C.c_void_p(shape_offsets.data_ptr()) if n_shapes > 0 else None, n_shapes, int(n_before),
                                                      C.c_void_p(sum.data_ptr()), C.c_void_p(mean.data_ptr()) if mean is not None else None,
                                                      C.c_void_p(rgb8.data_ptr()) if rgb8 is not None else None,
                                                      C.c_void_p(self._stream(stream))), self.ptr)
        return table, light_offsets, shape_offsets

    def render_progressive_motion(self, params, velocities, shutter, aperture, focus, n_samples, radii=None, restart=False, host_rgb=None,
                                  host_rgb8=None):
        """rm_render_progressive_motion: render_progressive_soft with moving spheres -- the sphere that is shape k of the uploaded
        scene moves by velocities[k] while the shutter stands open, and every sample sees it at a time of its own.  velocities:
        one vector (or None) for every shape, zero for what is not a sphere; radii: one radius a light, None for point lights.
        The frame begins again when a velocity or the shutter changes or the caller switches between this call and the other two
        ticks, and on everything that begins it again there.  -> (rm_timing, samples a pixel in the frame now)."""
        lens = _lens(aperture, focus, n_samples)
        v, shutter = _velocities(velocities), _shutter(shutter)
        r = _radii(radii) if radii is not None else None
        host = _host_outputs(params, host_rgb, host_rgb8)
        timing, total = _lib.rm_timing(), C.c_uint32(0)
        _lib.check(self.L.rm_render_progressive_motion(self.ptr, C.byref(params), C.byref(lens),
                                                       r.ctypes.data_as(C.POINTER(C.c_double)) if r is not None else None,
                                                       r.shape[0] if r is not None else 0,
                                                       v.ctypes.data_as(C.POINTER(_lib.rm_vec3)), v.shape[0], shutter, 1 if restart else 0,
                                                       *host, C.byref(total), C.byref(timing)), self.ptr)
        return timing, total.value

    # ---- moving shapes (include/rusty_marcher_amd.h, "moving shapes") ----
    def accumulate_moving_device(self, params, sum, aperture, focus, table, light_offsets, shape_offsets, n_before, mean=None, rgb8=None,
                                 stream=None):
        """rm_accumulate_moving_device: accumulate_motion_device in which every shape moves -- sample row s sees shape k of the
        scene, sphere, polygon or mesh, moved by shape_offsets[s][k]: a polygon's plane point and vertices, every triangle's
        centre and vertices of a mesh, the normals as uploaded.  The rows of every shape are read.  Arguments and result as
        accumulate_motion_device's."""
        lens, table = _accumulate_args(self.device, params, sum, aperture, focus, table, n_before, mean, rgb8)
        light_offsets = _offset_tensor(light_offsets, "light_offsets", "n_lights", lens.n_samples, sum.device)
        shape_offsets = _offset_tensor(shape_offsets, "shape_offsets", "n_shapes", lens.n_samples, sum.device)
        n_lights, n_shapes = int(light_offsets.shape[1]), int(shape_offsets.shape[1])
        _lib.check(self.L.rm_accumulate_moving_device(self.ptr, C.byref(params), C.byref(lens), C.c_void_p(table.data_ptr()),
                                                      C.c_void_p(light_offsets.data_ptr()) if n_lights > 0 else None, n_lights,
                                                      C.c_void_p(shape_offsets.data_ptr()) if n_shapes > 0 else None, n_shapes, int(n_before),
                                                      C.c_void_p(sum.data_ptr()), C.c_void_p(mean.data_ptr()) if mean is not None else None,
                                                      C.c_void_p(rgb8.data_ptr()) if rgb8 is not None else None,
                                                      C.c_void_p(self._stream(stream))), self.ptr)
        return table, light_offsets, shape_offsets

    def render_progressive_moving(self, params, velocities, shutter, aperture, focus, n_samples, radii=None, restart=False, host_rgb=None,
                                  host_rgb8=None):
        """rm_render_progressive_moving: render_progressive_motion in which a velocity on any shape is obeyed -- spheres,
        polygons and meshes move by velocities[k] while the shutter stands open.  Its frames are its own: a switch between this
        call and render_progressive_motion begins the frame again.  -> (rm_timing, samples a pixel in the frame now)."""
        lens = _lens(aperture, focus, n_samples)
        v, shutter = _velocities(velocities), _shutter(shutter)
        r = _radii(radii) if radii is not None else None
        host = _host_outputs(params, host_rgb, host_rgb8)
        timing, total = _lib.rm_timing(), C.c_uint32(0)
        _lib.check(self.L.rm_render_progressive_moving(self.ptr, C.byref(params), C.byref(lens),
                                                       r.ctypes.data_as(C.POINTER(C.c_double)) if r is not None else None,
                                                       r.shape[0] if r is not None else 0,
                                                       v.ctypes.data_as(C.POINTER(_lib.rm_vec3)), v.shape[0], shutter, 1 if restart else 0,
                                                       *host, C.byref(total), C.byref(timing)), self.ptr)
        return timing, total.value

    # ---- swept hierarchies (include/rusty_marcher_amd.h, "swept hierarchies") ----
    def swept(self, lo, hi):
        """rm_swept_build: a swept hierarchy of the uploaded scene -- its hierarchies' boxes refitted to bound every primitive at
        every offset within lo[k] .. hi[k] of its shape k.  lo, hi: (n_shapes, 3), finite, lo <= hi.  -> a Swept handle, stale
        once another scene is uploaded; close() it, or leave it to the context."""
        lo, hi = _extents(lo, hi)
        h = C.c_void_p()
        _lib.check(self.L.rm_swept_build(self.ptr, lo.ctypes.data_as(C.POINTER(C.c_double)), hi.ctypes.data_as(C.POINTER(C.c_double)),
                                         lo.shape[0], C.byref(h)), self.ptr)
        return Swept(self, h)

    def _swept_for(self, swept, shape_offsets):
        """The handle a swept pass walks: the caller's, or one built from the table's own extents (amin / amax over its rows, on
        the device)."""
        if swept is not None:
            if not isinstance(swept, Swept) or swept.ctx is not self or swept.ptr is None:
                raise ValueError("swept must be an open Swept handle of this context")
            return swept
        if shape_offsets.shape[1] == 0:
            return self.swept(np.zeros((0, 3)), np.zeros((0, 3)))
        return self.swept(shape_offsets.amin(dim=0).cpu().numpy(), shape_offsets.amax(dim=0).cpu().numpy())

    def accumulate_swept_device(self, params, sum, aperture, focus, table, light_offsets, shape_offsets, n_before, mean=None, rgb8=None,
                                stream=None, swept=None):
        """rm_accumulate_swept_device: accumulate_moving_device through a swept hierarchy -- the same bytes, with the scene's
        hierarchies walked where it has any.  swept: a handle of Context.swept whose extents hold every row of shape_offsets;
        None builds one from the table itself.  Arguments and result as accumulate_moving_device's."""
        lens, table = _accumulate_args(self.device, params, sum, aperture, focus, table, n_before, mean, rgb8)
        light_offsets = _offset_tensor(light_offsets, "light_offsets", "n_lights", lens.n_samples, sum.device)
        shape_offsets = _offset_tensor(shape_offsets, "shape_offsets", "n_shapes", lens.n_samples, sum.device)
        n_lights, n_shapes = int(light_offsets.shape[1]), int(shape_offsets.shape[1])
        handle = self._swept_for(swept, shape_offsets)
        try:
            _lib.check(self.L.rm_accumulate_swept_device(self.ptr, C.byref(params), C.byref(lens), C.c_void_p(table.data_ptr()),
                                                         C.c_void_p(light_offsets.data_ptr()) if n_lights > 0 else None, n_lights,
                                                         C.c_void_p(shape_offsets.data_ptr()) if n_shapes > 0 else None, n_shapes, handle.ptr,
                                                         int(n_before), C.c_void_p(sum.data_ptr()),
                                                         C.c_void_p(mean.data_ptr()) if mean is not None else None,
                                                         C.c_void_p(rgb8.data_ptr()) if rgb8 is not None else None,
                                                         C.c_void_p(self._stream(stream))), self.ptr)
        finally:
            if swept is None:
                handle.close()                                  # (waits for the device: the pass is through)
        return table, light_offsets, shape_offsets

    def accumulate_converging_swept_device(self, params, sum, stats, count, aperture, focus, n_samples, table, light_offsets, shape_offsets,
                                           tolerance, min_samples, max_samples, fresh, mean=None, rgb8=None, mask=None, workspace=None,
                                           stream=None, swept=None):
        """rm_accumulate_converging_swept_device: accumulate_converging_moving_device through a swept hierarchy -- the same
        bytes, lists and counts.  swept: as accumulate_swept_device's.  Arguments and result as
        accumulate_converging_moving_device's."""
        lens, conv, table, workspace = _converging_args(self, params, sum, stats, count, aperture, focus, n_samples, table, tolerance, min_samples,
                                                        max_samples, mean, rgb8, mask, workspace)
        rows = int(table.shape[0])
        light_offsets = _offset_tensor(light_offsets, "light_offsets", "n_lights", rows, sum.device)
        shape_offsets = _offset_tensor(shape_offsets, "shape_offsets", "n_shapes", rows, sum.device)
        n_lights, n_shapes = int(light_offsets.shape[1]), int(shape_offsets.shape[1])
        vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        frame = _lib.rm_converge_frame(vp(sum), vp(stats), vp(count), vp(workspace), vp(mean), vp(rgb8), vp(mask))
        handle = self._swept_for(swept, shape_offsets)
        try:
            _lib.check(self.L.rm_accumulate_converging_swept_device(self.ptr, C.byref(params), C.byref(lens), C.byref(conv), vp(table), rows,
                                                                    vp(light_offsets) if n_lights > 0 else None, n_lights,
                                                                    vp(shape_offsets) if n_shapes > 0 else None, n_shapes, handle.ptr,
                                                                    1 if fresh else 0, C.byref(frame), C.c_void_p(self._stream(stream))), self.ptr)
        finally:
            if swept is None:
                handle.close()
        return workspace

    # ---- converging frames (include/rusty_marcher_amd.h, "converging frames") ----
    def converge_workspace(self, params):
        """rm_converge_workspace: bytes of device memory the list of accumulate_converging_device needs for `params`."""
        b = C.c_size_t(0)
        _lib.check(self.L.rm_converge_workspace(C.byref(params), C.byref(b)), None)
        return b.value

    def accumulate_converging_device(self, params, sum, stats, count, aperture, focus, n_samples, table, tolerance, min_samples, max_samples,
                                     fresh, offsets=None, mean=None, rgb8=None, mask=None, workspace=None, stream=None):
        """rm_accumulate_converging_device: one pass of a converging frame -- the pixels still noisy by (tolerance, min_samples,
        max_samples), and their neighbours, are listed on the device and n_samples (1..64) more samples are cast for the listed
        pixels alone, each from the row of `table` its own count says.  sum (h, w, 3) and stats (h, w, 2) are contiguous float64
        tensors and count (h, w) an int32 one on the context's device; with `fresh` they are not read and every count is 0.
        table: the first rows of lens_sequence, at least max_samples of them, a float64 tensor (rows, 4) there or an array,
        which is checked and copied over; offsets: optionally as many rows of light_sequence, (rows, n_lights, 3).  mean, rgb8
        (h, w, 3) and mask (h, w, uint8) are optional outputs.  Asynchronous on `stream` (torch's current one by default).
        -> the workspace, an int32 tensor: ws[0] is the number of listed pixels, ws[1:1 + ws[0]] their indices y * w + x."""
        lens, conv, table, workspace = _converging_args(self, params, sum, stats, count, aperture, focus, n_samples, table, tolerance, min_samples,
                                                        max_samples, mean, rgb8, mask, workspace)
        n_lights = 0
        if offsets is not None:
            offsets = _offset_tensor(offsets, "offsets", "n_lights", int(table.shape[0]), sum.device)
            n_lights = int(offsets.shape[1])
        vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        frame = _lib.rm_converge_frame(vp(sum), vp(stats), vp(count), vp(workspace), vp(mean), vp(rgb8), vp(mask))
        _lib.check(self.L.rm_accumulate_converging_device(self.ptr, C.byref(params), C.byref(lens), C.byref(conv), vp(table), int(table.shape[0]),
                                                          vp(offsets) if n_lights > 0 else None, n_lights, 1 if fresh else 0, C.byref(frame),
                                                          C.c_void_p(self._stream(stream))), self.ptr)
        return workspace

    def render_converging(self, params, aperture, focus, n_samples, tolerance, min_samples, max_samples, radii=None, restart=False,
                          host_rgb=None, host_rgb8=None):
        """rm_render_converging: a tick of a converging frame the context keeps for the standing view, apart from
        render_progressive's -- n_samples more samples of the library's sequences for the pixels still noisy and their
        neighbours; radii: one radius a light for area lights, None for point lights.  Begun again as render_progressive_soft's
        frame is; tolerance, min_samples, max_samples and n_samples may change while it goes on.  Once a tick lists nothing the
        picture is finished and further ticks launch nothing.  -> (rm_timing, rm_converge_report)."""
        lens = _lens(aperture, focus, n_samples)
        conv = _converge(tolerance, min_samples, max_samples, lens.n_samples)
        r = _radii(radii) if radii is not None else None
        host = _host_outputs(params, host_rgb, host_rgb8)
        timing, report = _lib.rm_timing(), _lib.rm_converge_report()
        _lib.check(self.L.rm_render_converging(self.ptr, C.byref(params), C.byref(lens), C.byref(conv),
                                               r.ctypes.data_as(C.POINTER(C.c_double)) if r is not None else None,
                                               r.shape[0] if r is not None else 0, 1 if restart else 0,
                                               *host, C.byref(report), C.byref(timing)), self.ptr)
        return timing, report

    # ---- diffuse bounce (include/rusty_marcher_amd.h, "diffuse bounce") ----
    def bounce_sequence(self, first, count):
        """backend.bounce_sequence."""
        return bounce_sequence(first, count)

    def accumulate_bounce_device(self, params, sum, aperture, focus, table, offsets, bounce, strength, n_before, mean=None, rgb8=None,
                                 stream=None):
        """rm_accumulate_bounce_device: accumulate_soft_device with one bounce of indirect light -- where sample row s first hits
        a surface that is not glass, a ray leaves it in the direction row s of `bounce` gives (shifted for every pixel), and what
        comes back, times `strength`, the surface's diffusion and its diffuse colour, is added to the sample.  bounce: a
        contiguous float64 tensor (n_samples, 2) of points in [0, 1) on the context's device, or an array, which is checked
        (finite) and copied over; strength: a finite number >= 0, 0 is accumulate_soft_device's frame byte for byte.
        -> (the table's tensor, the offsets' tensor, the bounce table's tensor)."""
        strength = _strength(strength)
        lens, table = _accumulate_args(self.device, params, sum, aperture, focus, table, n_before, mean, rgb8)
        offsets = _offset_tensor(offsets, "offsets", "n_lights", lens.n_samples, sum.device)
        bounce = _bounce_tensor(bounce, lens.n_samples, sum.device)
        n_lights = int(offsets.shape[1])
        _lib.check(self.L.rm_accumulate_bounce_device(self.ptr, C.byref(params), C.byref(lens), C.c_void_p(table.data_ptr()),
                                                      C.c_void_p(offsets.data_ptr()) if n_lights > 0 else None, n_lights,
                                                      C.c_void_p(bounce.data_ptr()), strength, int(n_before),
                                                      C.c_void_p(sum.data_ptr()), C.c_void_p(mean.data_ptr()) if mean is not None else None,
                                                      C.c_void_p(rgb8.data_ptr()) if rgb8 is not None else None,
                                                      C.c_void_p(self._stream(stream))), self.ptr)
        return table, offsets, bounce

    def render_progressive_bounce(self, params, aperture, focus, n_samples, strength=1., radii=None, restart=False, host_rgb=None,
                                  host_rgb8=None):
        """rm_render_progressive_bounce: render_progressive_soft with a diffuse bounce of the library's sequence; radii: one radius
        a light for area lights, None for point lights.  The frame begins again when the strength changes or the caller switches
        between this call and another tick, and on everything that begins it again there.
        -> (rm_timing, samples a pixel in the frame now)."""
        lens = _lens(aperture, focus, n_samples)
        strength = _strength(strength)
        r = _radii(radii) if radii is not None else None
        host = _host_outputs(params, host_rgb, host_rgb8)
        timing, total = _lib.rm_timing(), C.c_uint32(0)
        _lib.check(self.L.rm_render_progressive_bounce(self.ptr, C.byref(params), C.byref(lens),
                                                       r.ctypes.data_as(C.POINTER(C.c_double)) if r is not None else None,
                                                       r.shape[0] if r is not None else 0, strength, 1 if restart else 0,
                                                       *host, C.byref(total), C.byref(timing)), self.ptr)
        return timing, total.value

    def accumulate_converging_bounce_device(self, params, sum, stats, count, aperture, focus, n_samples, table, bounce, strength, tolerance,
                                            min_samples, max_samples, fresh, offsets=None, mean=None, rgb8=None, mask=None, workspace=None,
                                            stream=None):
        """rm_accumulate_converging_bounce_device: accumulate_converging_device with a diffuse bounce -- the sample that is row r
        of the tables takes row r of `bounce`, (rows, 2) with the table's rows, a float64 tensor on the context's device or an
        array.  strength: a finite number >= 0, 0 is accumulate_converging_device's pass byte for byte.
        -> the workspace, as accumulate_converging_device."""
        strength = _strength(strength)
        lens, conv, table, workspace = _converging_args(self, params, sum, stats, count, aperture, focus, n_samples, table, tolerance, min_samples,
                                                        max_samples, mean, rgb8, mask, workspace)
        rows = int(table.shape[0])
        bounce = _bounce_tensor(bounce, rows, sum.device)
        n_lights = 0
        if offsets is not None:
            offsets = _offset_tensor(offsets, "offsets", "n_lights", rows, sum.device)
            n_lights = int(offsets.shape[1])
        vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        frame = _lib.rm_converge_frame(vp(sum), vp(stats), vp(count), vp(workspace), vp(mean), vp(rgb8), vp(mask))
        _lib.check(self.L.rm_accumulate_converging_bounce_device(self.ptr, C.byref(params), C.byref(lens), C.byref(conv), vp(table), rows,
                                                                 vp(offsets) if n_lights > 0 else None, n_lights, vp(bounce),
                                                                 strength, 1 if fresh else 0, C.byref(frame),
                                                                 C.c_void_p(self._stream(stream))), self.ptr)
        return workspace

    def render_converging_bounce(self, params, aperture, focus, n_samples, tolerance, min_samples, max_samples, strength=1., radii=None,
                                 restart=False, host_rgb=None, host_rgb8=None):
        """rm_render_converging_bounce: render_converging with a diffuse bounce of the library's sequence.  The frame is
        render_converging's own: beyond what begins it again there, a changed strength does, a switch between the calls does, and
        so does every camera move (history does not reach it).  -> (rm_timing, rm_converge_report)."""
        lens = _lens(aperture, focus, n_samples)
        conv = _converge(tolerance, min_samples, max_samples, lens.n_samples)
        strength = _strength(strength)
        r = _radii(radii) if radii is not None else None
        host = _host_outputs(params, host_rgb, host_rgb8)
        timing, report = _lib.rm_timing(), _lib.rm_converge_report()
        _lib.check(self.L.rm_render_converging_bounce(self.ptr, C.byref(params), C.byref(lens), C.byref(conv),
                                                      r.ctypes.data_as(C.POINTER(C.c_double)) if r is not None else None,
                                                      r.shape[0] if r is not None else 0, strength, 1 if restart else 0,
                                                      *host, C.byref(report), C.byref(timing)), self.ptr)
        return timing, report

    # ---- converging frames with moving spheres (include/rusty_marcher_amd.h, "converging frames with moving spheres") ----
    def accumulate_converging_motion_device(self, params, sum, stats, count, aperture, focus, n_samples, table, light_offsets, shape_offsets,
                                            tolerance, min_samples, max_samples, fresh, mean=None, rgb8=None, mask=None, workspace=None,
                                            stream=None):
        """rm_accumulate_converging_motion_device: accumulate_converging_device with a shape offset table as well -- the sample
        that is row r of the tables sees the sphere that is shape k of the scene at its centre + shape_offsets[r][k], in every
        hit test, shadow test and normal.  light_offsets: (rows, n_lights, 3), zeros for point lights; shape_offsets:
        (rows, n_shapes, 3), rows of shapes that are not spheres are not read; `rows` is the table's, at least max_samples.
        Each a contiguous float64 tensor on the context's device, or an array, which is checked (finite) and copied over;
        n_lights and n_shapes must be the uploaded scene's.  -> the workspace, as accumulate_converging_device."""
        lens, conv, table, workspace = _converging_args(self, params, sum, stats, count, aperture, focus, n_samples, table, tolerance, min_samples,
                                                        max_samples, mean, rgb8, mask, workspace)
        rows = int(table.shape[0])
        light_offsets = _offset_tensor(light_offsets, "light_offsets", "n_lights", rows, sum.device)
        shape_offsets = _offset_tensor(shape_offsets, "shape_offsets", "n_shapes", rows, sum.device)
        n_lights, n_shapes = int(light_offsets.shape[1]), int(shape_offsets.shape[1])
        vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        frame = _lib.rm_converge_frame(vp(sum), vp(stats), vp(count), vp(workspace), vp(mean), vp(rgb8), vp(mask))
        _lib.check(self.L.rm_accumulate_converging_motion_device(self.ptr, C.byref(params), C.byref(lens), C.byref(conv), vp(table), rows,
                                                                 vp(light_offsets) if n_lights > 0 else None, n_lights,
                                                                 vp(shape_offsets) if n_shapes > 0 else None, n_shapes, 1 if fresh else 0,
                                                                 C.byref(frame), C.c_void_p(self._stream(stream))), self.ptr)
        return workspace

    def render_converging_motion(self, params, velocities, shutter, aperture, focus, n_samples, tolerance, min_samples, max_samples, radii=None,
                                 restart=False, host_rgb=None, host_rgb8=None):
        """rm_render_converging_motion: render_converging with moving spheres -- the sphere that is shape k of the uploaded scene
        moves by velocities[k] while the shutter stands open, and every sample sees it at a time of its own.  velocities: one
        vector (or None) for every shape, zero for what is not a sphere; radii: one radius a light, None for point lights.  The
        frame is render_converging's own: it begins again when a velocity or the shutter changes or the caller switches between
        the two ticks, and on everything that begins it again there.  -> (rm_timing, rm_converge_report)."""
        lens = _lens(aperture, focus, n_samples)
        conv = _converge(tolerance, min_samples, max_samples, lens.n_samples)
        v, shutter = _velocities(velocities), _shutter(shutter)
        r = _radii(radii) if radii is not None else None
        host = _host_outputs(params, host_rgb, host_rgb8)
        timing, report = _lib.rm_timing(), _lib.rm_converge_report()
        _lib.check(self.L.rm_render_converging_motion(self.ptr, C.byref(params), C.byref(lens), C.byref(conv),
                                                      r.ctypes.data_as(C.POINTER(C.c_double)) if r is not None else None,
                                                      r.shape[0] if r is not None else 0,
                                                      v.ctypes.data_as(C.POINTER(_lib.rm_vec3)), v.shape[0], shutter, 1 if restart else 0,
                                                      *host, C.byref(report), C.byref(timing)), self.ptr)
        return timing, report

    # ---- converging frames with moving shapes (include/rusty_marcher_amd.h, "converging frames with moving shapes") ----
    def accumulate_converging_moving_device(self, params, sum, stats, count, aperture, focus, n_samples, table, light_offsets, shape_offsets,
                                            tolerance, min_samples, max_samples, fresh, mean=None, rgb8=None, mask=None, workspace=None,
                                            stream=None):
        """rm_accumulate_converging_moving_device: accumulate_converging_motion_device in which every shape moves -- the sample
        that is row r of the tables sees shape k of the scene, sphere, polygon or mesh, moved by shape_offsets[r][k]: a polygon's
        plane point and vertices, every triangle's centre and vertices of a mesh, the normals as uploaded.  The rows of every
        shape are read.  Arguments and result as accumulate_converging_motion_device's."""
        lens, conv, table, workspace = _converging_args(self, params, sum, stats, count, aperture, focus, n_samples, table, tolerance, min_samples,
                                                        max_samples, mean, rgb8, mask, workspace)
        rows = int(table.shape[0])
        light_offsets = _offset_tensor(light_offsets, "light_offsets", "n_lights", rows, sum.device)
        shape_offsets = _offset_tensor(shape_offsets, "shape_offsets", "n_shapes", rows, sum.device)
        n_lights, n_shapes = int(light_offsets.shape[1]), int(shape_offsets.shape[1])
        vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        frame = _lib.rm_converge_frame(vp(sum), vp(stats), vp(count), vp(workspace), vp(mean), vp(rgb8), vp(mask))
        _lib.check(self.L.rm_accumulate_converging_moving_device(self.ptr, C.byref(params), C.byref(lens), C.byref(conv), vp(table), rows,
                                                                 vp(light_offsets) if n_lights > 0 else None, n_lights,
                                                                 vp(shape_offsets) if n_shapes > 0 else None, n_shapes, 1 if fresh else 0,
                                                                 C.byref(frame), C.c_void_p(self._stream(stream))), self.ptr)
        return workspace

    def render_converging_moving(self, params, velocities, shutter, aperture, focus, n_samples, tolerance, min_samples, max_samples, radii=None,
                                 restart=False, host_rgb=None, host_rgb8=None):
        """rm_render_converging_moving: render_converging_motion in which a velocity on any shape is obeyed -- spheres, polygons
        and meshes move by velocities[k] while the shutter stands open.  Its frames are its own: a switch between this call and
        render_converging_motion or render_converging begins the frame again.  -> (rm_timing, rm_converge_report)."""
        lens = _lens(aperture, focus, n_samples)
        conv = _converge(tolerance, min_samples, max_samples, lens.n_samples)
        v, shutter = _velocities(velocities), _shutter(shutter)
        r = _radii(radii) if radii is not None else None
        host = _host_outputs(params, host_rgb, host_rgb8)
        timing, report = _lib.rm_timing(), _lib.rm_converge_report()
        _lib.check(self.L.rm_render_converging_moving(self.ptr, C.byref(params), C.byref(lens), C.byref(conv),
                                                      r.ctypes.data_as(C.POINTER(C.c_double)) if r is not None else None,
                                                      r.shape[0] if r is not None else 0,
                                                      v.ctypes.data_as(C.POINTER(_lib.rm_vec3)), v.shape[0], shutter, 1 if restart else 0,
                                                      *host, C.byref(report), C.byref(timing)), self.ptr)
        return timing, report

    # ---- moving camera (include/rusty_marcher_amd.h, "moving camera") ----
    def camera_sequence(self, first, count, velocity, shutter, turn=(0., 0., 0.), basis=None):
        """camera_sequence of this module with the basis the context renders with where none is given."""
        return camera_sequence(first, count, velocity, shutter, turn, self.camera()[1] if basis is None else basis)

    def accumulate_camera_device(self, params, sum, aperture, focus, table, camera_rows, light_offsets, shape_offsets, n_before, mean=None,
                                 rgb8=None, stream=None):
        """rm_accumulate_camera_device: accumulate_moving_device in which the camera moves as well -- sample row s sees the scene
        from the context's camera + camera_rows[s][0:3] along the basis camera_rows[s][3:12] (right, up, forward).  camera_rows:
        (n_samples, 12); shape_offsets: None where no shape moves -- the scene keeps its hierarchy then.  Tables as
        accumulate_moving_device's.  -> (the table's tensor, the camera rows', the light offsets', the shape offsets' or None)."""
        lens, table = _accumulate_args(self.device, params, sum, aperture, focus, table, n_before, mean, rgb8)
        camera_rows = _camera_rows_tensor(camera_rows, lens.n_samples, sum.device)
        light_offsets = _offset_tensor(light_offsets, "light_offsets", "n_lights", lens.n_samples, sum.device)
        n_lights, n_shapes = int(light_offsets.shape[1]), 0
        if shape_offsets is not None:
            shape_offsets = _offset_tensor(shape_offsets, "shape_offsets", "n_shapes", lens.n_samples, sum.device)
            n_shapes = int(shape_offsets.shape[1])
        _lib.check(self.L.rm_accumulate_camera_device(self.ptr, C.byref(params), C.byref(lens), C.c_void_p(table.data_ptr()),
                                                      C.c_void_p(camera_rows.data_ptr()),
                                                      C.c_void_p(light_offsets.data_ptr()) if n_lights > 0 else None, n_lights,
                                                      C.c_void_p(shape_offsets.data_ptr()) if n_shapes > 0 else None, n_shapes, int(n_before),
                                                      C.c_void_p(sum.data_ptr()), C.c_void_p(mean.data_ptr()) if mean is not None else None,
                                                      C.c_void_p(rgb8.data_ptr()) if rgb8 is not None else None,
                                                      C.c_void_p(self._stream(stream))), self.ptr)
        return table, camera_rows, light_offsets, shape_offsets

    def render_progressive_camera(self, params, camera_velocity, shutter, aperture, focus, n_samples, turn=(0., 0., 0.), velocities=None,
                                  radii=None, restart=False, host_rgb=None, host_rgb8=None):
        """rm_render_progressive_camera: render_progressive_moving with a camera that moves by camera_velocity and turns by
        `turn` = (yaw, pitch, roll) rates while the shutter stands open.  velocities: None where no shape moves.  Its frames are
        its own: a switch to or from any other tick begins the frame again.  -> (rm_timing, samples a pixel in the frame now)."""
        lens = _lens(aperture, focus, n_samples)
        motion, shutter = _camera_motion(camera_velocity, turn), _shutter(shutter)
        v = _velocities(velocities) if velocities is not None else None
        r = _radii(radii) if radii is not None else None
        host = _host_outputs(params, host_rgb, host_rgb8)
        timing, total = _lib.rm_timing(), C.c_uint32(0)
        _lib.check(self.L.rm_render_progressive_camera(self.ptr, C.byref(params), C.byref(lens),
                                                       r.ctypes.data_as(C.POINTER(C.c_double)) if r is not None else None,
                                                       r.shape[0] if r is not None else 0,
                                                       v.ctypes.data_as(C.POINTER(_lib.rm_vec3)) if v is not None else None,
                                                       v.shape[0] if v is not None else 0, shutter, C.byref(motion), 1 if restart else 0,
                                                       *host, C.byref(total), C.byref(timing)), self.ptr)
        return timing, total.value

    # ---- converging frames with a moving camera (include/rusty_marcher_amd.h, "moving camera") ----
    def accumulate_converging_camera_device(self, params, sum, stats, count, aperture, focus, n_samples, table, camera_rows, light_offsets,
                                            shape_offsets, tolerance, min_samples, max_samples, fresh, mean=None, rgb8=None, mask=None,
                                            workspace=None, stream=None):
        """rm_accumulate_converging_camera_device: accumulate_converging_moving_device in which the camera moves as well -- the
        sample that is row r of the tables sees the scene from the camera of camera_rows[r], (rows, 12).  shape_offsets: None
        where no shape moves.  -> the workspace, as accumulate_converging_device."""
        lens, conv, table, workspace = _converging_args(self, params, sum, stats, count, aperture, focus, n_samples, table, tolerance, min_samples,
                                                        max_samples, mean, rgb8, mask, workspace)
        rows = int(table.shape[0])
        camera_rows = _camera_rows_tensor(camera_rows, rows, sum.device)
        light_offsets = _offset_tensor(light_offsets, "light_offsets", "n_lights", rows, sum.device)
        n_lights, n_shapes = int(light_offsets.shape[1]), 0
        if shape_offsets is not None:
            shape_offsets = _offset_tensor(shape_offsets, "shape_offsets", "n_shapes", rows, sum.device)
            n_shapes = int(shape_offsets.shape[1])
        vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        frame = _lib.rm_converge_frame(vp(sum), vp(stats), vp(count), vp(workspace), vp(mean), vp(rgb8), vp(mask))
        _lib.check(self.L.rm_accumulate_converging_camera_device(self.ptr, C.byref(params), C.byref(lens), C.byref(conv), vp(table), rows,
                                                                 vp(camera_rows), vp(light_offsets) if n_lights > 0 else None, n_lights,
                                                                 vp(shape_offsets) if n_shapes > 0 else None, n_shapes, 1 if fresh else 0,
                                                                 C.byref(frame), C.c_void_p(self._stream(stream))), self.ptr)
        return workspace

    def render_converging_camera(self, params, camera_velocity, shutter, aperture, focus, n_samples, tolerance, min_samples, max_samples,
                                 turn=(0., 0., 0.), velocities=None, radii=None, restart=False, host_rgb=None, host_rgb8=None):
        """rm_render_converging_camera: render_converging_moving with a camera that moves by camera_velocity and turns by `turn`
        while the shutter stands open.  velocities: None where no shape moves.  Its frames are its own.
        -> (rm_timing, rm_converge_report)."""
        lens = _lens(aperture, focus, n_samples)
        conv = _converge(tolerance, min_samples, max_samples, lens.n_samples)
        motion, shutter = _camera_motion(camera_velocity, turn), _shutter(shutter)
        v = _velocities(velocities) if velocities is not None else None
        r = _radii(radii) if radii is not None else None
        host = _host_outputs(params, host_rgb, host_rgb8)
        timing, report = _lib.rm_timing(), _lib.rm_converge_report()
        _lib.check(self.L.rm_render_converging_camera(self.ptr, C.byref(params), C.byref(lens), C.byref(conv),
                                                      r.ctypes.data_as(C.POINTER(C.c_double)) if r is not None else None,
                                                      r.shape[0] if r is not None else 0,
                                                      v.ctypes.data_as(C.POINTER(_lib.rm_vec3)) if v is not None else None,
                                                      v.shape[0] if v is not None else 0, shutter, C.byref(motion), 1 if restart else 0,
                                                      *host, C.byref(report), C.byref(timing)), self.ptr)
        return timing, report

    # ---- swept hierarchies under a moving camera (include/rusty_marcher_amd.h, "swept hierarchies under a moving camera") ----
    def _camera_swept_for(self, swept, shape_offsets):
        """_swept_for for the camera calls, whose shape table may be None: the library refuses that by name, but no handle
        can be built from it."""
        if swept is None and shape_offsets is None:
            raise ValueError("shape_offsets is None and no swept handle is given: nothing moves, use the flat camera call")
        return self._swept_for(swept, shape_offsets)

    def accumulate_camera_swept_device(self, params, sum, aperture, focus, table, camera_rows, light_offsets, shape_offsets, n_before,
                                       mean=None, rgb8=None, stream=None, swept=None):
        """rm_accumulate_camera_swept_device: accumulate_camera_device with a shape table through a swept hierarchy -- the same
        bytes, with the scene's hierarchies walked where it has any.  swept: a handle of Context.swept whose extents hold every
        row of shape_offsets (the boxes are in world space: no camera row matters); None builds one from the table itself.
        Arguments and result as accumulate_camera_device's, but that the library refuses shape_offsets None."""
        lens, table = _accumulate_args(self.device, params, sum, aperture, focus, table, n_before, mean, rgb8)
        camera_rows = _camera_rows_tensor(camera_rows, lens.n_samples, sum.device)
        light_offsets = _offset_tensor(light_offsets, "light_offsets", "n_lights", lens.n_samples, sum.device)
        n_lights, n_shapes = int(light_offsets.shape[1]), 0
        if shape_offsets is not None:
            shape_offsets = _offset_tensor(shape_offsets, "shape_offsets", "n_shapes", lens.n_samples, sum.device)
            n_shapes = int(shape_offsets.shape[1])
        handle = self._camera_swept_for(swept, shape_offsets)
        try:
            _lib.check(self.L.rm_accumulate_camera_swept_device(self.ptr, C.byref(params), C.byref(lens), C.c_void_p(table.data_ptr()),
                                                                C.c_void_p(camera_rows.data_ptr()),
                                                                C.c_void_p(light_offsets.data_ptr()) if n_lights > 0 else None, n_lights,
                                                                C.c_void_p(shape_offsets.data_ptr()) if n_shapes > 0 else None, n_shapes,
                                                                handle.ptr, int(n_before), C.c_void_p(sum.data_ptr()),
                                                                C.c_void_p(mean.data_ptr()) if mean is not None else None,
                                                                C.c_void_p(rgb8.data_ptr()) if rgb8 is not None else None,
                                                                C.c_void_p(self._stream(stream))), self.ptr)
        finally:
            if swept is None:
                handle.close()                                  # (waits for the device: the pass is through)
        return table, camera_rows, light_offsets, shape_offsets

    def accumulate_converging_camera_swept_device(self, params, sum, stats, count, aperture, focus, n_samples, table, camera_rows,
                                                  light_offsets, shape_offsets, tolerance, min_samples, max_samples, fresh, mean=None,
                                                  rgb8=None, mask=None, workspace=None, stream=None, swept=None):
        """rm_accumulate_converging_camera_swept_device: accumulate_converging_camera_device with a shape table through a swept
        hierarchy -- the same bytes, lists and counts.  swept: as accumulate_camera_swept_device's.  Arguments and result as
        accumulate_converging_camera_device's."""
        lens, conv, table, workspace = _converging_args(self, params, sum, stats, count, aperture, focus, n_samples, table, tolerance, min_samples,
                                                        max_samples, mean, rgb8, mask, workspace)
        rows = int(table.shape[0])
        camera_rows = _camera_rows_tensor(camera_rows, rows, sum.device)
        light_offsets = _offset_tensor(light_offsets, "light_offsets", "n_lights", rows, sum.device)
        n_lights, n_shapes = int(light_offsets.shape[1]), 0
        if shape_offsets is not None:
            shape_offsets = _offset_tensor(shape_offsets, "shape_offsets", "n_shapes", rows, sum.device)
            n_shapes = int(shape_offsets.shape[1])
        vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        frame = _lib.rm_converge_frame(vp(sum), vp(stats), vp(count), vp(workspace), vp(mean), vp(rgb8), vp(mask))
        handle = self._camera_swept_for(swept, shape_offsets)
        try:
            _lib.check(self.L.rm_accumulate_converging_camera_swept_device(self.ptr, C.byref(params), C.byref(lens), C.byref(conv), vp(table),
                                                                           rows, vp(camera_rows), vp(light_offsets) if n_lights > 0 else None,
                                                                           n_lights, vp(shape_offsets) if n_shapes > 0 else None, n_shapes,
                                                                           handle.ptr, 1 if fresh else 0, C.byref(frame),
                                                                           C.c_void_p(self._stream(stream))), self.ptr)
        finally:
            if swept is None:
                handle.close()
        return workspace

    def swept_tick_info(self):
        """rm_swept_tick_info: what the ticks that move a shape did -> {"walked_swept": whether the last sampled-frame tick's
        launch walked a swept hierarchy, "builds": hierarchies the ticks have built over the context's life}.  Host state only."""
        rep = _lib.rm_swept_tick_report()
        _lib.check(self.L.rm_swept_tick_info(self.ptr, C.byref(rep)), self.ptr)
        return {"walked_swept": int(rep.walked_swept), "builds": int(rep.builds)}

    # ---- variance-guided filter (include/rusty_marcher_amd.h, "variance-guided filter") ----
    def denoise_workspace(self, params):
        """rm_denoise_workspace: bytes of device memory denoise_device needs for `params`."""
        b = C.c_size_t(0)
        _lib.check(self.L.rm_denoise_workspace(C.byref(params), C.byref(b)), None)
        return b.value

    def denoise_device(self, params, sum, stats, count, out, sigma_l=4., sigma_z=.1, epsilon=1e-10, fallback_variance=1., iterations=5,
                       normal_squarings=5, hits=None, variance=None, rgb8=None, workspace=None, stream=None):
        """rm_denoise_device: the edge-avoiding filter of a converging frame -- sum (h, w, 3) and stats (h, w, 2), contiguous
        float64 tensors, and count (h, w), an int32 one, on the context's device, as accumulate_converging_device leaves them --
        into out (h, w, 3) float64 and, where given, variance (h, w) float64 and rgb8 (h, w, 3) uint8.  hits: optionally the
        guide, what primary_hits_device returned for the same params (a DeviceHits, or its raw (h, w, 9) float64 tensor); without
        it only the variance steers the filter.  The keyword defaults are starting values, not tuned ones.  Asynchronous on
        `stream` (torch's current one by default).  -> the workspace, a uint8 tensor that holds nothing a later call needs."""
        torch = _torch()
        h, w = params.frame_height, params.frame_width
        if isinstance(hits, DeviceHits):
            hits = hits.raw
        for name, t, dtype, shape in (("sum", sum, torch.float64, (h, w, 3)), ("stats", stats, torch.float64, (h, w, 2)),
                                      ("count", count, torch.int32, (h, w)), ("out", out, torch.float64, (h, w, 3)),
                                      ("hits", hits, torch.float64, (h, w, 9)), ("variance", variance, torch.float64, (h, w)),
                                      ("rgb8", rgb8, torch.uint8, (h, w, 3))):
            if t is None and name in ("hits", "variance", "rgb8"):
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("%s must be a contiguous %s torch tensor of shape %s" % (name, dtype, shape))
            if t.device.type != "cuda" or t.device.index != self.device:
                raise ValueError("%s must live on cuda:%d (the context's device), not %s" % (name, self.device, t.device))
        for name, t in (("sum", sum), ("stats", stats), ("count", count), ("hits", hits)):
            if t is not None and out.data_ptr() == t.data_ptr():
                raise ValueError("out must not be %s's own tensor" % name)
        ctl = _denoise(sigma_l, sigma_z, epsilon, fallback_variance, iterations, normal_squarings)
        need = Context.denoise_workspace(self, params)
        if workspace is None:
            workspace = torch.empty((need,), dtype=torch.uint8, device=sum.device)
        elif not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1 or workspace.shape[0] < need \
                or not workspace.is_contiguous() or workspace.device != sum.device or workspace.data_ptr() % 16 != 0:
            raise ValueError("workspace must be a contiguous uint8 torch tensor of at least %d bytes on %s, aligned to 16" % (need, sum.device))
        vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self.L.rm_denoise_device(self.ptr, C.byref(params), C.byref(ctl), vp(sum), vp(stats), vp(count), vp(hits), vp(workspace),
                                            vp(out), vp(variance), vp(rgb8), C.c_void_p(self._stream(stream))), self.ptr)
        return workspace

    def render_denoised(self, params, sigma_l=4., sigma_z=.1, epsilon=1e-10, fallback_variance=1., iterations=5, normal_squarings=5,
                        guides=True, host_rgb=None, host_rgb8=None):
        """rm_render_denoised: the filter over the converging frame the context keeps -- whichever render_converging* tick ran
        last -- into buffers of its own; the converging frame is left as it is and its next tick continues it.  guides: steer
        the filter by the hits under the pixels as well, seen through a pinhole from the context's camera as it stands; turn
        them off under a wide aperture, a moving camera or strongly moving shapes, where the picture's edges are not the
        guide's.  The keyword defaults are starting values, not tuned ones.  -> rm_timing."""
        ctl = _denoise(sigma_l, sigma_z, epsilon, fallback_variance, iterations, normal_squarings)
        host = _host_outputs(params, host_rgb, host_rgb8)
        timing = _lib.rm_timing()
        _lib.check(self.L.rm_render_denoised(self.ptr, C.byref(params), C.byref(ctl), 1 if guides else 0, *host, C.byref(timing)), self.ptr)
        return timing

    # ---- temporal reprojection (include/rusty_marcher_amd.h, "temporal reprojection") ----
    def reproject_device(self, params, prev_total, prev_stats, prev_count, prev_hits, cur_hits, previous_view, out_total, out_stats, out_count,
                         sigma_z=.1, min_normal_dot=.9, max_history=32, carried=None, carried_total=None, stream=None):
        """rm_reproject_device: carries a converging frame -- prev_total (h, w, 3) and prev_stats (h, w, 2) float64, prev_count
        (h, w) int32, as accumulate_converging_device leaves them, and prev_hits, what primary_hits_device returned for the view
        they were sampled from (a DeviceHits or its raw (h, w, 9) tensor) -- to the view cur_hits was made for, into out_total,
        out_stats and out_count of the same shapes.  previous_view: the previous camera, an rm_view or what Context.camera()
        returned then.  carried: optionally (h, w) uint8, 1 where history was carried; carried_total: optionally one int32 on the
        device, their number.  The keyword defaults are starting values, not tuned ones.  Asynchronous on `stream` (torch's
        current one by default)."""
        torch = _torch()
        h, w = params.frame_height, params.frame_width
        prev_hits = prev_hits.raw if isinstance(prev_hits, DeviceHits) else prev_hits
        cur_hits = cur_hits.raw if isinstance(cur_hits, DeviceHits) else cur_hits
        inputs = (("prev_total", prev_total, torch.float64, (h, w, 3)), ("prev_stats", prev_stats, torch.float64, (h, w, 2)),
                  ("prev_count", prev_count, torch.int32, (h, w)), ("prev_hits", prev_hits, torch.float64, (h, w, 9)),
                  ("cur_hits", cur_hits, torch.float64, (h, w, 9)))
        outputs = (("out_total", out_total, torch.float64, (h, w, 3)), ("out_stats", out_stats, torch.float64, (h, w, 2)),
                   ("out_count", out_count, torch.int32, (h, w)), ("carried", carried, torch.uint8, (h, w)),
                   ("carried_total", carried_total, torch.int32, (1,)))
        for name, t, dtype, shape in inputs + outputs:
            if t is None and name in ("carried", "carried_total"):
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("%s must be a contiguous %s torch tensor of shape %s" % (name, dtype, shape))
            if t.device.type != "cuda" or t.device.index != self.device:
                raise ValueError("%s must live on cuda:%d (the context's device), not %s" % (name, self.device, t.device))
        for oname, o, _, _ in outputs:
            for iname, i, _, _ in inputs:
                if o is not None and o.data_ptr() == i.data_ptr():
                    raise ValueError("%s must not be %s's own tensor" % (oname, iname))
        ctl = _reproject(sigma_z, min_normal_dot, max_history)
        view = _view(previous_view)
        vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self.L.rm_reproject_device(self.ptr, C.byref(params), C.byref(ctl), C.byref(view), vp(prev_total), vp(prev_stats),
                                              vp(prev_count), vp(prev_hits), vp(cur_hits), vp(out_total), vp(out_stats), vp(out_count),
                                              vp(carried), vp(carried_total), C.c_void_p(self._stream(stream))), self.ptr)

    def converge_history(self, settings):
        """rm_converge_history: history for render_converging.  settings: None turns it off; an rm_reproject, or a dict / tuple of
        (sigma_z, min_normal_dot, max_history), turns it on -- a camera move then reprojects the frame rather than beginning it
        again."""
        if settings is None:
            _lib.check(self.L.rm_converge_history(self.ptr, None), self.ptr)
            return
        if isinstance(settings, dict):
            settings = _reproject(**settings)
        elif not isinstance(settings, _lib.rm_reproject):
            settings = _reproject(*settings)
        _lib.check(self.L.rm_converge_history(self.ptr, C.byref(settings)), self.ptr)

    def history_info(self):
        """rm_converge_history_info -> {"reprojections": frames the ticks have begun from history, "last_reprojected": whether the
        last render_converging tick did, "carried" / "without": the pixels that carried history at the last reprojection and
        those that did not}.  Host state only."""
        rep = _lib.rm_history_report()
        _lib.check(self.L.rm_converge_history_info(self.ptr, C.byref(rep)), self.ptr)
        return {"reprojections": int(rep.reprojections), "last_reprojected": int(rep.last_reprojected), "carried": int(rep.carried),
                "without": int(rep.without)}

    def primary_hits_device(self, params, out=None, stream=None):
        """rm_primary_hits_device: the closest hit under every pixel rm_render_device writes with `params` (the whole
        patch rows), as DeviceHits of [frame_height][frame_width].  `out`: a float64 tensor of shape
        (frame_height, frame_width, 9) on the context's device (zeros by default); rows the render leaves untouched
        keep what it holds."""
        torch = _torch()
        h, w = params.frame_height, params.frame_width
        if out is None:
            out = torch.zeros((h, w, 9), dtype=torch.float64, device="cuda:%d" % self.device)
        if out.dtype != torch.float64 or tuple(out.shape) != (h, w, 9) or not out.is_contiguous():
            raise ValueError("out must be a contiguous float64 tensor of shape (%d, %d, 9)" % (h, w))
        _lib.check(self.L.rm_primary_hits_device(self.ptr, C.byref(params), C.c_void_p(out.data_ptr()),
                                                 C.c_void_p(self._stream(stream))), self.ptr)
        return _device_hits(out)

    def pick(self, params, x, y):
        """rm_pick: the rm_hit under pixel (x = column, y = row) of the frame `params` describes."""
        hit = _lib.rm_hit()
        _lib.check(self.L.rm_pick(self.ptr, C.byref(params), int(x), int(y), C.byref(hit)), self.ptr)
        return hit

    # ---- multi-GPU frames (include/rusty_marcher_amd.h, rm_comm_* / rm_frame_*) ----
    @staticmethod
    def comm_unique_id():
        """RM_COMM_ID_BYTES from RCCL: rank 0 makes one and hands it to the other ranks."""
        buf = C.create_string_buffer(_lib.RM_COMM_ID_BYTES)
        _lib.check(_lib.lib().rm_comm_unique_id(buf), None)
        return buf.raw

    def comm_init(self, rank, world, unique_id=None):
        """unique_id None: the layout of `world` ranks without a transport (tests)."""
        if unique_id is not None and len(unique_id) != _lib.RM_COMM_ID_BYTES:
            raise ValueError("unique_id must be %d bytes" % _lib.RM_COMM_ID_BYTES)
        _lib.check(self.L.rm_comm_init(self.ptr, unique_id, rank, world), self.ptr)

    def comm_exchange(self, all_ranks):
        """False (default): chunks gathered at rank 0; True: all-gathered on every rank."""
        _lib.check(self.L.rm_comm_exchange(self.ptr, 1 if all_ranks else 0), self.ptr)

    def comm_destroy(self):
        self.L.rm_comm_destroy(self.ptr)

    def exchange_layout(self, params, world):
        rows, chunk = C.c_uint32(0), C.c_size_t(0)
        _lib.check(self.L.rm_exchange_layout(C.byref(params), world, C.byref(rows), C.byref(chunk)), self.ptr)
        return rows.value, chunk.value

    def frame_submit(self, params, device_ptr, gather_ptr, display_ptr=None, slot=0):
        _lib.check(self.L.rm_frame_submit(self.ptr, C.byref(params), C.c_void_p(device_ptr), C.c_void_p(gather_ptr),
                                          C.c_void_p(display_ptr) if display_ptr else None, slot), self.ptr)

    def frame_submit_f64(self, params, gather_ptr, frame_ptr=None, slot=0):
        """The f64 rows themselves: rendered packed into this rank's chunk of gather_ptr,
        all-gathered in place, written in image order to frame_ptr where given."""
        _lib.check(self.L.rm_frame_submit_f64(self.ptr, C.byref(params), C.c_void_p(gather_ptr),
                                              C.c_void_p(frame_ptr) if frame_ptr else None, slot), self.ptr)

    def frame_wait(self, slot=0, timeout_ms=None):
        """Raises BackendError(RM_ERR_TIMEOUT) instead of hanging when a peer never joins."""
        if timeout_ms is None:
            _lib.check(self.L.rm_frame_wait(self.ptr, slot), self.ptr)
        else:
            _lib.check(self.L.rm_frame_wait_for(self.ptr, slot, int(timeout_ms)), self.ptr)

    def frame_timing_enable(self, on=True):
        _lib.check(self.L.rm_frame_timing_enable(self.ptr, 1 if on else 0), self.ptr)

    def frame_timing(self, slot=0):
        t = _lib.rm_frame_times()
        _lib.check(self.L.rm_frame_timing(self.ptr, slot, C.byref(t)), self.ptr)
        return t

    def comm_info(self):
        """(rank, world, communicators in use) as the RCCL communicator itself reports them."""
        r, w, n = C.c_int(0), C.c_int(0), C.c_int(0)
        _lib.check(self.L.rm_comm_info(self.ptr, C.byref(r), C.byref(w), C.byref(n)), self.ptr)
        return r.value, w.value, n.value

    # ---- device buffers without torch (rm_buffer_*) ----
    def buffer_alloc(self, nbytes):
        p = C.c_void_p()
        _lib.check(self.L.rm_buffer_alloc(self.ptr, int(nbytes), C.byref(p)), self.ptr)
        return p

    def buffer_free(self, dptr):
        self.L.rm_buffer_free(self.ptr, dptr)

    def buffer_write(self, dptr, host_array):
        _lib.check(self.L.rm_buffer_write(self.ptr, dptr, host_array.ctypes.data_as(C.c_void_p), host_array.nbytes), self.ptr)

    def buffer_read(self, dptr, host_array):
        _lib.check(self.L.rm_buffer_read(self.ptr, dptr, host_array.ctypes.data_as(C.c_void_p), host_array.nbytes), self.ptr)

    def kernel_name(self, params):
        buf = C.create_string_buffer(256)
        _lib.check(self.L.rm_kernel_name(self.ptr, C.byref(params), buf, 256), self.ptr)
        return buf.value.decode()

    def device_info(self):
        name = C.create_string_buffer(256)
        cus, lds = C.c_int(0), C.c_size_t(0)
        _lib.check(self.L.rm_device_info(self.ptr, name, 256, C.byref(cus), C.byref(lds)), self.ptr)
        return {"name": name.value.decode(), "cus": cus.value, "lds_per_block": lds.value}


_contexts = {}


def default_context(device=0):
    if device not in _contexts:
        _contexts[device] = Context(device)
    return _contexts[device]


def make_params(fov, height, width, max_depth=3, band=None):
    """rm_create_renderer + optional overrides."""
    p = _lib.rm_params()
    _lib.lib().rm_create_renderer(float(fov), float(height), float(width), C.byref(p))
    p.max_depth = int(max_depth)
    if band is not None:
        p.patch_row_begin, p.patch_row_end = int(band[0]), int(band[1])
        if len(band) > 2:
            p.patch_row_stride = int(band[2])
    return p


# ---- the oriented camera's host arithmetic (no GPU, no context) ----
FIXED_VIEW = ((1., 0., 0.), (0., 1., 0.), (0., 0., -1.))


def basis_look_at(eye, target, up=(0., 1., 0.)):
    """rm_camera_basis_look_at: forward = unit(target - eye), right = unit(forward x up), up = right x forward."""
    out = _lib.rm_camera_basis()
    _lib.check(_lib.lib().rm_camera_basis_look_at(_lib.vec3(eye), _lib.vec3(target), _lib.vec3(up), C.byref(out)))
    return out


def basis_turn(basis, yaw=0., pitch=0., roll=0.):
    """rm_camera_basis_turn: about the basis' own up, right, forward (radians; positive yaw turns left)."""
    out = _lib.rm_camera_basis()
    _lib.check(_lib.lib().rm_camera_basis_turn(C.byref(_lib.camera_basis(basis)), float(yaw), float(pitch), float(roll), C.byref(out)))
    return out


# ---- the moving camera's host arithmetic (no GPU, no context) ----
def camera_sequence(first, count, velocity, shutter, turn=(0., 0., 0.), basis=FIXED_VIEW):
    """rm_camera_sequence: rows first .. first + count - 1 of the library's camera sequence, (count, 12) float64 rows (offset,
    right, up, forward): row s moves the camera by velocity times the row's time within the shutter -- rm_motion_sequence's time
    for that row -- and turns `basis` by turn = (yaw, pitch, roll) rates times it.  Rates of zero keep the basis byte for byte."""
    first, count = _sequence_rows(first, count)
    motion, shutter = _camera_motion(velocity, turn), _shutter(shutter)
    rows = np.zeros((int(count), 12), dtype=np.float64)
    _lib.check(_lib.lib().rm_camera_sequence(int(first), int(count), C.byref(motion), C.byref(_lib.camera_basis(basis)), shutter,
                                             rows.ctypes.data_as(C.POINTER(C.c_double))))
    return rows


def bounce_sequence(first, count):
    """rm_bounce_sequence: rows first .. first + count - 1 of the library's bounce sequence, (count, 2) float64 points of [0, 1)
    (the radical inverses in base 19 and 23).  Host arithmetic: needs neither a context nor a GPU."""
    first, count = _sequence_rows(first, count)
    t = np.zeros((int(count), 2), dtype=np.float64)
    _lib.check(_lib.lib().rm_bounce_sequence(int(first), int(count), t.ctypes.data_as(C.POINTER(C.c_double))), None)
    return t


def swept_extents(table):
    """rm_swept_extents: the per-shape componentwise minimum and maximum of a host shape offset table (rows, n_shapes, 3) ->
    (lo, hi), each (n_shapes, 3).  Host arithmetic: needs neither a context nor a GPU."""
    t = np.ascontiguousarray(table, dtype=np.float64)
    if t.ndim != 3 or t.shape[2] != 3:
        raise ValueError("table must have the shape (rows, n_shapes, 3), got %s" % (t.shape,))
    lo, hi = np.zeros(t.shape[1:]), np.zeros(t.shape[1:])
    D = C.POINTER(C.c_double)
    _lib.check(_lib.lib().rm_swept_extents(t.ctypes.data_as(D), t.shape[0], t.shape[1], lo.ctypes.data_as(D), hi.ctypes.data_as(D)), None)
    return lo, hi


def swept_motion_extents(velocities, shutter):
    """rm_swept_motion_extents: the extents that hold every row of motion_sequence(velocities, shutter) -> (lo, hi)."""
    v, shutter = _velocities(velocities), _shutter(shutter)
    lo, hi = np.zeros((v.shape[0], 3)), np.zeros((v.shape[0], 3))
    D = C.POINTER(C.c_double)
    _lib.check(_lib.lib().rm_swept_motion_extents(v.ctypes.data_as(C.POINTER(_lib.rm_vec3)), v.shape[0], shutter, lo.ctypes.data_as(D),
                                                  hi.ctypes.data_as(D)), None)
    return lo, hi
