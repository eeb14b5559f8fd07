"""The yardstick of the tests of the converging frames with moving spheres (include/rusty_marcher_amd.h, "converging frames with
moving spheres"): converge_reference.run / one_pass -- the select rule and the fold in numpy -- over motion_reference.samples,
which hold every row of the three sequences for every pixel of a moved scene, cast by the CPU oracle.  No GPU, no product code.

The rows are those of progressive_reference.lens_sequence, soft_reference.light_sequence (zeros where a case has no radii) and
motion_reference.motion_sequence(0, max_samples, motion_reference.velocities(kinds), motion_reference.SHUTTER).

Exact masks, lists and counts are legitimate only where no free decision lies within 12 n ymax TIGHT of its bound
(converge_reference.py has the derivation); converge_reference.run asserts it.  tests/test_converge_motion_abi.py pins the
numbers below and shows the cases are not vacuous; tests/test_gpu_converge_motion.py holds the GPU to this file."""
import numpy as np

import converge_reference as CR
import lens_reference as LR
import motion_reference as MR
import progressive_reference as PR
import soft_reference as SR

TIGHT = CR.TIGHT

# The cases both test files use: converge_reference.CASES' parameters with the spheres moving, 32 x 32, LR.FOCUS:
# name -> (scene, depth, aperture, radii or None, n_samples, tolerance, min_samples, max_samples)
CASES = {
    "demo-motion-8": ("demo", 3, LR.APERTURE, None, 8, 0.1, 16, 256),
    "penumbra-motion-8": ("penumbra", 3, 0., SR.PENUMBRA_RADII, 8, 0.1, 16, 256),
    "demo-motion-5": ("demo", 3, LR.APERTURE, None, 5, 0.1, 16, 256),
    "spheres-motion-8": ("synthetic256", 6, LR.APERTURE, None, 8, 0.1, 16, 256),
    "demo-motion-soft-64": ("demo", 3, LR.APERTURE, (1.5, 3.), 64, 0.05, 16, 256),
    "penumbra-motion-1": ("penumbra", 3, LR.APERTURE, SR.PENUMBRA_RADII, 1, 0.1, 16, 40),
}
# The case of converge_reference.CASES with the same parameters and the spheres standing still
STILL = {"demo-motion-8": "demo-8", "penumbra-motion-8": "penumbra-8", "demo-motion-5": "demo-5", "spheres-motion-8": "spheres-8",
         "demo-motion-soft-64": "demo-soft-64", "penumbra-motion-1": "penumbra-1"}
# What the reference alone finds for them: name -> (passes until nothing is listed, samples cast, distinct final counts)
FOUND = {"demo-motion-8": (25, 35280, 19), "penumbra-motion-8": (21, 34864, 18), "demo-motion-5": (40, 36920, 27),
         "spheres-motion-8": (29, 55448, 25), "demo-motion-soft-64": (5, 133888, 4), "penumbra-motion-1": (41, 22864, 18)}
# ... and the pixels whose final count differs from the still case's: the motion changes what is sampled, in each case more than
# 5 % of the frame
DIFFER = {"demo-motion-8": 395, "penumbra-motion-8": 186, "demo-motion-5": 358, "spheres-motion-8": 562, "demo-motion-soft-64": 343,
          "penumbra-motion-1": 100}


class Yardstick(CR.Yardstick):
    """CR.Yardstick with every row of the three sequences for every pixel of the moved scene, made once a case and shared
    (never written to)."""

    def __init__(self, pkg, O, orc):
        super().__init__(pkg, O, orc)
        self._moved = {}

    def n_shapes(self, name):
        return int(self.scene(name)[1].c.n_shapes)

    def kinds(self, name):
        return MR.kinds_of(self.scene(name)[1])

    def tables(self, name, n_rows, radii=None):
        """Rows [0, n_rows) of the three sequences for the scene: lens rows, light offsets (zeros without radii), shape offsets
        of the test velocities."""
        lights = SR.light_sequence(0, n_rows, radii) if radii is not None else np.zeros((n_rows, self.n_lights(name), 3))
        shapes = MR.motion_sequence(0, n_rows, MR.velocities(self.kinds(name)), MR.SHUTTER)
        return PR.lens_sequence(0, n_rows), lights, shapes

    def motion_samples(self, name, w, h, depth, aperture, focus, table, lights, shapes, view=None):
        """[pixel][row][3]: row r of every pixel cast with the lights at lights[r] and the spheres at shapes[r]."""
        t, f, g = (np.ascontiguousarray(a, dtype=np.float64) for a in (table, lights, shapes))
        key = (name, w, h, depth, float(aperture), float(focus), t.tobytes(), f.tobytes(), g.tobytes(), view)
        if key not in self._moved:
            eye, basis = (self.eye(name), None) if view is None else view
            s = MR.samples(self.O, self.orc, self.scene(name)[1], eye, basis, w, h, depth, aperture, focus, t, f, g)
            s.setflags(write=False)
            self._moved[key] = s
        return self._moved[key]


def case_samples(Y, name, w=32, h=32, view=None):
    """The samples of a case: max_samples rows of the three sequences."""
    scene, depth, aperture, radii, ns, tol, lo, hi = CASES[name]
    table, lights, shapes = Y.tables(scene, hi, radii)
    return Y.motion_samples(scene, w, h, depth, aperture, LR.FOCUS, table, lights, shapes, view)
