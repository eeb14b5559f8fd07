"""The yardstick of the moving camera's tests (include/rusty_marcher_amd.h, "moving camera"): frames whose every sample sees the
scene from a camera of its own, from the oracle alone.  No GPU, no product code.

Nothing new is restated: for table row s the rays are lens_reference.lens_rays called with that row alone, the eye
eye + off[s] (one numpy float64 addition a component) and the row's basis -- always a basis, so always the oriented formula --
and they are cast by the CPU oracle against moving_reference.MovedScene(light_offsets[s], shape_offsets[s]).  The fold is
progressive_reference.accumulate; the converging frames go through converge_reference's select and fold over the same samples,
as converge_moving_reference does.  So parity is the project's TIGHT with no pixel left out.

camera_rows below is the yardstick's own linear camera path (numpy: the offsets are the library's byte for byte, the turned
bases only to rounding, which is why the GPU tests hand the yardstick whatever table the GPU got).  tests/test_camera_motion_abi.py
pins this file and shows it is not vacuous; tests/test_gpu_camera_motion.py and tests/test_gpu_converge_camera.py hold the GPU
to it."""
import numpy as np

import converge_reference as CR
import lens_reference as LR
import motion_reference as MR
import moving_reference as MV
import progressive_reference as PR
import radiance_reference as RR

TIGHT = MV.TIGHT                     # the project's parity bound, per channel, no pixel left out
SHUTTER = MV.SHUTTER
FIXED = RR.FIXED_VIEW

# The test motions, a case: name -> (scene, depth, camera velocity in the scene's units a shutter, (yaw, pitch, roll) in radians a
# shutter).  The velocities start from moving_reference.SPEED's scale (6 for the demo and the 256 spheres, 3 for the pool scene,
# 150 for the Cornell box); the turns are a few pixels' worth of the 1.5 rad field of view over 32 pixels.
MOTIONS = {
    "demo-translate": ("demo", 3, (6., 1.5, 0.), (0., 0., 0.)),
    "demo-turn": ("demo", 3, (0., 0., 0.), (0.35, -0.1, 0.2)),
    "demo-both": ("demo", 3, (4., 0., -2.), (0.2, 0.1, 0.)),
    "cornell": ("cornell", 3, (150., 40., 0.), (0.1, 0., 0.)),
    "synthetic256": ("synthetic256", 6, (6., 2., 0.), (0.15, 0., 0.1)),
    "pool": ("pool", 3, (3., 1., 0.), (0.2, 0., 0.)),
}
# Pixels of a 32 x 32 frame (aperture 0, point lights, shapes standing still, shutter 1, 16 rows of the sequences) whose mean
# differs by more than 0.05 in some channel from the mean with the motion all zero, counted with the oracle alone
# (tests/test_camera_motion_abi.py): each above 5 % of 1,024.
BLURRED = {"demo-translate": 691, "demo-turn": 610, "demo-both": 606, "cornell": 255, "synthetic256": 579, "pool": 290}
ROWS = 16


def _unit(v):
    return v / np.sqrt(np.dot(v, v))


def basis_turn(basis, yaw, pitch, roll):
    """rm_camera_basis_turn for a right-handed basis: yaw about up, pitch about right, roll about forward, then orthonormal
    again from forward."""
    r, u, f = (np.array(v, dtype=np.float64) for v in basis)
    c, s = np.cos(yaw), np.sin(yaw)
    f, r = f * c - r * s, r * c + f * s
    c, s = np.cos(pitch), np.sin(pitch)
    f, u = f * c + u * s, u * c - f * s
    c, s = np.cos(roll), np.sin(roll)
    u, r = u * c + r * s, r * c - u * s
    f = _unit(f)
    r = _unit(r - f * np.dot(r, f))
    return r, np.cross(r, f), f


def camera_rows(first, count, velocity, turn, basis=FIXED, shutter=SHUTTER):
    """(count, 12) rows (off, right, up, forward): t = shutter * phi_17(s), motion_reference.motion_sequence's instant; off =
    velocity * t; rates of zero keep `basis` as given."""
    off = MR.motion_sequence(first, count, [velocity], shutter)[:, 0]
    t = MR.motion_sequence(first, count, [(1., 0., 0.)], shutter)[:, 0, 0]
    rows = np.empty((count, 12))
    rows[:, :3] = off
    for k in range(count):
        b = basis if all(a == 0. for a in turn) else basis_turn(basis, turn[0] * t[k], turn[1] * t[k], turn[2] * t[k])
        rows[k, 3:] = np.concatenate([np.asarray(v, dtype=np.float64) for v in b])
    return rows


def standing_rows(count, basis=FIXED, off=(0., 0., 0.)):
    """Every row the same camera."""
    return np.tile(np.concatenate([np.asarray(off, dtype=np.float64)] + [np.asarray(v, dtype=np.float64) for v in basis]), (count, 1))


def random_rows(rng, count, scale, basis=FIXED):
    """A camera table that is not the library's: another offset and another turn for every row, none of them zero."""
    rows = np.empty((count, 12))
    for k in range(count):
        rows[k, :3] = rng.uniform(0.2, 1., 3) * rng.choice([-1., 1.], 3) * scale
        a = rng.uniform(0.02, 0.2, 3) * rng.choice([-1., 1.], 3)
        rows[k, 3:] = np.concatenate(basis_turn(basis, a[0], a[1], a[2]))
    return rows


def samples(O, orc, oscene, eye, width, height, depth, aperture, focus, table, camera, light_offsets, shape_offsets=None):
    """The radiance of every lens ray of the rows a frame writes, row s cast from the camera of camera[s] with the lights at
    light_offsets[s] and the shapes at shape_offsets[s] (None: as they stand): [pixel][s][3], pixels row-major."""
    rows = LR.rows_of(height)
    table, camera = np.asarray(table, dtype=np.float64), np.asarray(camera, dtype=np.float64)
    light_offsets = np.asarray(light_offsets, dtype=np.float64)
    n = table.shape[0]
    assert camera.shape == (n, 12) and light_offsets.shape[0] == n
    still = np.zeros((oscene.c.n_shapes, 3))
    eye = np.asarray(eye, dtype=np.float64)
    r = orc.renderer(width, height)
    out = np.empty((rows * width, n, 3))
    for s in range(n):
        row = camera[s]
        basis = (tuple(row[3:6]), tuple(row[6:9]), tuple(row[9:12]))
        o, d = LR.lens_rays(width, rows, r, eye + row[:3], basis, aperture, focus, table[s:s + 1])
        moved = MV.MovedScene(O, oscene, light_offsets[s], still if shape_offsets is None else np.asarray(shape_offsets, dtype=np.float64)[s])
        out[:, s] = orc.cast(moved, np.ascontiguousarray(o), np.ascontiguousarray(d), depth, normalize=True)
    return out


def fold(s, width, height, passes):
    """progressive_reference.accumulate over the passes: (sum, mean), each [height][width][3]."""
    rows = LR.rows_of(height)
    assert sum(passes) == s.shape[1]
    acc, mean, done = None, None, 0
    for n in passes:
        acc, mean = PR.accumulate(acc, s[:, done:done + n], done)
        done += n
    out_sum, out_mean = np.zeros((height, width, 3)), np.zeros((height, width, 3))
    out_sum[:rows], out_mean[:rows] = acc.reshape(rows, width, 3), mean.reshape(rows, width, 3)
    return out_sum, out_mean


class Yardstick(MV.Yardstick):
    """MV.Yardstick with the moving camera's samples and frames, each made once and shared (never written to)."""

    def __init__(self, pkg, O, orc):
        super().__init__(pkg, O, orc)
        self._camera = {}

    def camera_samples(self, name, w, h, depth, aperture, focus, table, camera, lights, shapes=None, eye=None):
        """[pixel][row][3]; eye: the context's position, the scene's camera by default."""
        arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in (table, camera, lights)]
        g = None if shapes is None else np.ascontiguousarray(shapes, dtype=np.float64)
        key = (name, w, h, depth, float(aperture), float(focus), eye) + tuple(a.tobytes() for a in arrays) + (None if g is None else g.tobytes(),)
        if key not in self._camera:
            s = samples(self.O, self.orc, self.scene(name)[1], self.eye(name) if eye is None else eye, w, h, depth, aperture, focus,
                        arrays[0], arrays[1], arrays[2], g)
            s.setflags(write=False)
            self._camera[key] = s
        return self._camera[key]

    def camera(self, name, w, h, depth, aperture, focus, table, camera, lights, shapes, passes, eye=None):
        """(sum, mean) after the passes over the four tables."""
        return fold(self.camera_samples(name, w, h, depth, aperture, focus, table, camera, lights, shapes, eye), w, h, passes)

    def blurred(self, case):
        """The pixels of the case's 32 x 32 pinhole frame that the motion changes by more than 0.05 in some channel."""
        name, depth, velocity, turn = MOTIONS[case]
        table, lights = PR.lens_sequence(0, ROWS), np.zeros((ROWS, self.n_lights(name), 3))
        moved = self.camera(name, 32, 32, depth, 0., LR.FOCUS, table, camera_rows(0, ROWS, velocity, turn), lights, None, (ROWS,))[1]
        still = self.camera(name, 32, 32, depth, 0., LR.FOCUS, table, standing_rows(ROWS), lights, None, (ROWS,))[1]
        return int((np.abs(moved - still) > 0.05).any(axis=2).sum())


def converging(s, width, rows, ns, tolerance, min_samples, max_samples, passes=None, check=True):
    """converge_reference.run over the camera's samples."""
    return CR.run(s, width, rows, ns, tolerance, min_samples, max_samples, passes, check)
