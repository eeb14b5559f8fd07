"""The yardstick of the tests of the converging frames with moving shapes (include/rusty_marcher_amd.h, "converging frames with
moving shapes"): converge_reference.run / one_pass -- the select rule and the fold in numpy -- over moving_reference.samples,
which hold every row of the three sequences for every pixel of a scene whose every shape is moved, cast by the CPU oracle.  No
GPU, no product code.

The rows are those of progressive_reference.lens_sequence, soft_reference.light_sequence (zeros where a case has no radii) and
motion_reference.motion_sequence(0, max_samples, moving_reference.velocities(kinds, SPEED[case]), moving_reference.SHUTTER).

Exact masks, lists and counts are legitimate only where no free decision lies within 12 n ymax TIGHT of its bound
(converge_reference.py has the derivation); converge_reference.run asserts it.  Every case below was run on the CPU with the
oracle alone first: all six hold the margin (the nearest decision is 143 margins away, in demo-moving-soft-64) and all six
pass the 5 % condition with moving_reference.SPEED's speeds, so no tolerance and no speed had to change.
tests/test_converge_moving_abi.py pins the numbers
below and shows the cases are not vacuous; tests/test_gpu_converge_moving.py holds the GPU to this file."""
import numpy as np

import converge_reference as CR
import lens_reference as LR
import motion_reference as MR
import moving_reference as MV
import progressive_reference as PR
import soft_reference as SR

TIGHT = CR.TIGHT

# The cases both test files use, 32 x 32, LR.FOCUS:
# name -> (scene, depth, aperture, radii or None, n_samples, tolerance, min_samples, max_samples)
#   demo-moving-8        the floor quad moves
#   cornell-moving-8     meshes only: no sphere, so the tick's staging rule is exercised
#   pool-moving-5        pentagon and hexagon, so the vertex pool is read; 5 samples leave four idle lanes
#   spheres-moving-8     STACK 32; a hierarchy in the image, walked flat
#   demo-moving-soft-64  area lights, 64 samples a pass
#   pool-moving-1        one sample a pass
CASES = {
    "demo-moving-8": ("demo", 3, LR.APERTURE, None, 8, 0.1, 16, 256),
    "cornell-moving-8": ("cornell", 3, 0., None, 8, 0.1, 16, 256),
    "pool-moving-5": ("pool", 3, LR.APERTURE, None, 5, 0.1, 16, 256),
    "spheres-moving-8": ("synthetic256", 6, LR.APERTURE, None, 8, 0.1, 16, 256),
    "demo-moving-soft-64": ("demo", 3, LR.APERTURE, (1.5, 3.), 64, 0.05, 16, 256),
    "pool-moving-1": ("pool", 3, LR.APERTURE, None, 1, 0.1, 16, 40),
}
# The speed of the shapes that are not spheres, a case: moving_reference.SPEED of the case's scene, as proposed
SPEED = {name: MV.SPEED[case[0]] for name, case in CASES.items()}
# The cases of converge_motion_reference.CASES with the same parameters: with zero velocities on everything but the spheres
# the yardstick must find their FOUND
MOTION = {"demo-moving-8": "demo-motion-8", "spheres-moving-8": "spheres-motion-8", "demo-moving-soft-64": "demo-motion-soft-64"}
# What the reference alone finds for them: name -> (passes until nothing is listed, samples cast, distinct final counts)
FOUND = {"demo-moving-8": (25, 39176, 19), "cornell-moving-8": (33, 45768, 29), "pool-moving-5": (32, 44250, 27),
         "spheres-moving-8": (29, 54896, 25), "demo-moving-soft-64": (5, 144768, 4), "pool-moving-1": (41, 24891, 24)}
# ... and the pixels whose final count differs from the same case with only the spheres moving (moving_reference.spheres_only):
# the polygons' and meshes' motion changes what is sampled, in each case more than 5 % of the frame
DIFFER = {"demo-moving-8": 341, "cornell-moving-8": 178, "pool-moving-5": 366, "spheres-moving-8": 249, "demo-moving-soft-64": 278,
          "pool-moving-1": 191}


class Yardstick(MV.Yardstick):
    """MV.Yardstick with every row of the three sequences for every pixel of the moved scene, made once a case and shared
    (never written to)."""

    def __init__(self, pkg, O, orc):
        super().__init__(pkg, O, orc)
        self._moved = {}

    def tables(self, name, n_rows, radii=None, speed=None):
        """Rows [0, n_rows) of the three sequences for the scene: lens rows, light offsets (zeros without radii), shape offsets
        of the test velocities with the shapes that are not spheres at `speed` (moving_reference.SPEED's by default)."""
        lights = SR.light_sequence(0, n_rows, radii) if radii is not None else np.zeros((n_rows, self.n_lights(name), 3))
        v = MV.velocities(self.kinds(name), MV.SPEED[name] if speed is None else speed)
        return PR.lens_sequence(0, n_rows), lights, MR.motion_sequence(0, n_rows, v, MV.SHUTTER)

    def moving_samples(self, name, w, h, depth, aperture, focus, table, lights, shapes, view=None):
        """[pixel][row][3]: row r of every pixel cast with the lights at lights[r] and every shape at shapes[r]."""
        t, f, g = (np.ascontiguousarray(a, dtype=np.float64) for a in (table, lights, shapes))
        key = (name, w, h, depth, float(aperture), float(focus), t.tobytes(), f.tobytes(), g.tobytes(), view)
        if key not in self._moved:
            eye, basis = (self.eye(name), None) if view is None else view
            s = MV.samples(self.O, self.orc, self.scene(name)[1], eye, basis, w, h, depth, aperture, focus, t, f, g)
            s.setflags(write=False)
            self._moved[key] = s
        return self._moved[key]


def case_tables(Y, name):
    """The three tables of a case: max_samples rows."""
    scene, depth, aperture, radii, ns, tol, lo, hi = CASES[name]
    return Y.tables(scene, hi, radii, SPEED[name])


def case_samples(Y, name, w=32, h=32, view=None, spheres_only=False):
    """The samples of a case: max_samples rows of the three sequences; spheres_only: with zero rows for every other shape."""
    scene, depth, aperture, radii, ns, tol, lo, hi = CASES[name]
    table, lights, shapes = case_tables(Y, name)
    if spheres_only:
        shapes = MV.spheres_only(shapes, Y.kinds(scene))
    return Y.moving_samples(scene, w, h, depth, aperture, LR.FOCUS, table, lights, shapes, view)
