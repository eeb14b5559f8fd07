"""The yardstick of the moving spheres' tests (include/rusty_marcher_amd.h, "moving spheres"): rm_motion_sequence restated in
numpy, operation for operation as the header states it, and the motion frame from the oracle alone.  No GPU, no product code.

A shape offset depends on the sample row and the shape, not on the pixel -- as the lens point and the light offsets do -- so
sample row s of every pixel is orc_cast_ray against one scene whose spheres stand at the moved centres and whose lights stand
at the moved positions: MovedScene builds that scene with ctypes, an oracle Scene struct that owns a copy of the shapes array
with only `center` of the ORC_SPHERE shapes changed (one addition a component; vertices, triangles and materials stay the
source's, pointers and all) and a lights array as soft_reference.MovedScene's.  The rays are lens_reference.lens_rays', the fold
is progressive_reference.accumulate.  tests/test_motion_abi.py pins this file on the library's sequence and on
soft_reference.samples and shows it is not vacuous; tests/test_gpu_motion.py holds the GPU to it."""
import ctypes as C

import numpy as np

import lens_reference as LR
import progressive_reference as PR
import soft_reference as SR

TIGHT = PR.TIGHT                     # the project's parity bound, per channel, no pixel left out
MAX_SAMPLES = PR.MAX_SAMPLES
GOLDEN = SR.GOLDEN                   # the turn of the test velocities from one sphere to the next
ORC_SPHERE = 0                       # oracle/rm_oracle.h
SHUTTER = 1.
# Pixels of a 32 x 32 frame (aperture 0, point lights, shutter 1, 16 rows of the library's sequences, velocities(shapes)) whose
# motion mean differs from the still mean of the same table by more than 0.05 in some channel, counted with the oracle alone
# (tests/test_motion_abi.py): name -> (depth, rows, pixels)
BLURRED = {"demo": (3, 16, 434), "synthetic256": (6, 16, 404)}
# ... and of the nine cells of variant_matrix.CELLS (its aperture and focus, 8 rows, the same velocities): cell id -> pixels
BLURRED_CELLS = {"flat-integer-5": 84, "flat-integer-6": 84, "flat-generic-5": 139, "flat-generic-6": 139, "spheres-integer-5": 169,
                 "spheres-integer-6": 170, "spheres-generic-5": 220, "spheres-generic-6": 222, "mesh-integer-5": 81}
CELL_ROWS = 8


def motion_sequence(first, count, velocities, shutter):
    """rm_motion_sequence: rows first .. first + count - 1, (count, len(velocities), 3) offsets, every operation rounded once:
    t = shutter * phi_17(s), off[s][k].c = velocities[k].c * t."""
    v = np.asarray(velocities, dtype=np.float64).reshape(-1, 3)
    shutter = np.float64(shutter)
    assert first >= 0 and count >= 0 and first + count <= MAX_SAMPLES
    assert np.isfinite(v).all() and np.isfinite(shutter) and shutter >= 0.
    off = np.empty((count, v.shape[0], 3))
    for k in range(count):
        r, q = PR.digit_reversed(first + k, 17)
        t = shutter * (np.float64(r) / np.float64(q))                # (r, q < 2^53: exact before the one division)
        off[k] = v * t                                               # one product a component
    return off


def velocities(kinds):
    """The test velocities: sphere shape k moves with (2 cos(2 pi g k), 2 sin(2 pi g k), 0.5), g the golden ratio's fraction, k the
    shape's index in the list; every other shape stands still.  kinds: the kind of every shape (ORC_SPHERE = 0 for a sphere)."""
    v = np.zeros((len(kinds), 3))
    for k, kind in enumerate(kinds):
        if kind == ORC_SPHERE:
            a = 2. * np.pi * GOLDEN * k
            v[k] = (2. * np.cos(a), 2. * np.sin(a), 0.25 * 2.)
    return v


def kinds_of(oscene):
    """The kind of every shape of an oracle scene, in list order."""
    return [int(oscene.c.shapes[k].kind) for k in range(oscene.c.n_shapes)]


def random_offsets(rng, count, n_shapes, scale=1.):
    """A shape offset table that is not the library's: another offset for every row and every shape, none of them zero."""
    off = rng.uniform(-scale, scale, (count, n_shapes, 3))
    off[np.abs(off) < 1e-3] = 0.25
    return off


class MovedScene:
    """An oracle Scene struct with shapes and lights of its own: the source's, sphere k moved by shape_row[k] and light l by
    light_row[l]; .ptr as OracleScene's."""

    def __init__(self, O, oscene, light_row, shape_row):
        src = oscene.c
        loff = np.asarray(light_row, dtype=np.float64).reshape(-1, 3)
        soff = np.asarray(shape_row, dtype=np.float64).reshape(-1, 3)
        assert loff.shape[0] == src.n_lights and soff.shape[0] == src.n_shapes
        self.source = oscene                                         # vertices, triangles and materials are borrowed: keep their owner alive
        self.lights = (O.Light * max(1, src.n_lights))()
        for l in range(src.n_lights):
            lt = src.lights[l]
            p = O.Vec3(float(np.float64(lt.position.x) + loff[l, 0]), float(np.float64(lt.position.y) + loff[l, 1]),
                       float(np.float64(lt.position.z) + loff[l, 2]))     # one addition, rounded once
            self.lights[l] = O.Light(p, O.Vec3(lt.color.x, lt.color.y, lt.color.z), lt.intensity)
        self.shapes = (O.Shape * max(1, src.n_shapes))()
        if src.n_shapes:
            C.memmove(self.shapes, src.shapes, C.sizeof(O.Shape) * src.n_shapes)      # every field as it is, byte for byte
        for k in range(src.n_shapes):
            if src.shapes[k].kind == ORC_SPHERE:                     # rows of other shapes are never read
                c = src.shapes[k].center
                self.shapes[k].center = O.Vec3(float(np.float64(c.x) + soff[k, 0]), float(np.float64(c.y) + soff[k, 1]),
                                               float(np.float64(c.z) + soff[k, 2]))   # one addition, rounded once
        self.struct = O.Scene(C.cast(self.lights, C.POINTER(O.Light)), src.n_lights, C.cast(self.shapes, C.POINTER(O.Shape)), src.n_shapes,
                              O.Vec3(src.camera.x, src.camera.y, src.camera.z))
        self.ptr = C.pointer(self.struct)

    @property
    def c(self):
        return self.struct


def samples(O, orc, oscene, eye, basis, width, height, depth, aperture, focus, table, light_offsets, shape_offsets):
    """The radiance of every lens ray of the rows a frame writes, row s shaded with the lights at light_offsets[s] and the
    spheres at shape_offsets[s]: [pixel][s][3], pixels row-major."""
    rows = LR.rows_of(height)
    table = np.asarray(table, dtype=np.float64)
    light_offsets, shape_offsets = np.asarray(light_offsets, dtype=np.float64), np.asarray(shape_offsets, dtype=np.float64)
    n = table.shape[0]
    assert light_offsets.shape[0] == n and shape_offsets.shape[0] == n
    o, d = LR.lens_rays(width, rows, orc.renderer(width, height), eye, basis, aperture, focus, table)
    o, d = o.reshape(rows * width, n, 3), d.reshape(rows * width, n, 3)
    out = np.empty((rows * width, n, 3))
    for s in range(n):
        out[:, s] = orc.cast(MovedScene(O, oscene, light_offsets[s], shape_offsets[s]), np.ascontiguousarray(o[:, s]),
                             np.ascontiguousarray(d[:, s]), depth, normalize=True)
    return out


def frames(O, orc, oscene, eye, basis, width, height, depth, aperture, focus, table, light_offsets, shape_offsets, passes):
    """progressive_reference.frames with both offset tables: (sum, mean) after the passes, each [height][width][3]."""
    rows = LR.rows_of(height)
    assert sum(passes) == np.asarray(table).shape[0]
    s = samples(O, orc, oscene, eye, basis, width, height, depth, aperture, focus, table, light_offsets, shape_offsets)
    acc, mean, done = None, None, 0
    for n in passes:
        acc, mean = PR.accumulate(acc, s[:, done:done + n], done)
        done += n
    out_sum, out_mean = np.zeros((height, width, 3)), np.zeros((height, width, 3))
    out_sum[:rows], out_mean[:rows] = acc.reshape(rows, width, 3), mean.reshape(rows, width, 3)
    return out_sum, out_mean


class Yardstick(SR.Yardstick):
    """SR.Yardstick with reference motion frames, each made once and shared (never written to)."""

    def __init__(self, pkg, O, orc):
        super().__init__(pkg, O, orc)
        self._motion = {}

    def n_shapes(self, name):
        return int(self.scene(name)[1].c.n_shapes)

    def kinds(self, name):
        return kinds_of(self.scene(name)[1])

    def motion(self, name, w, h, depth, aperture, focus, table, light_offsets, shape_offsets, passes, view=None):
        """(sum, mean) after the passes over `table` and both offset tables; view = (eye, basis) of an oriented context, None:
        the fixed view."""
        t = np.ascontiguousarray(table, dtype=np.float64)
        f = np.ascontiguousarray(light_offsets, dtype=np.float64)
        g = np.ascontiguousarray(shape_offsets, dtype=np.float64)
        key = (name, w, h, depth, float(aperture), float(focus), t.tobytes(), f.tobytes(), g.tobytes(), tuple(passes), view)
        if key not in self._motion:
            eye, basis = (self.eye(name), None) if view is None else view
            pair = frames(self.O, self.orc, self.scene(name)[1], eye, basis, w, h, depth, aperture, focus, t, f, g, passes)
            for a in pair:
                a.setflags(write=False)
            self._motion[key] = pair
        return self._motion[key]
