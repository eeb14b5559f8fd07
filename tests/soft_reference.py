"""The yardstick of the area lights' tests (include/rusty_marcher_amd.h, "area lights"): rm_light_sequence restated in numpy,
operation for operation as the header states it, and the soft frame from the oracle alone.  No GPU, no product code.

A light offset depends on the sample row and the light, not on the pixel -- as the lens point does -- so sample row s of every
pixel is orc_cast_ray against one scene whose lights stand at the moved positions: moved_scene builds that scene with ctypes,
an oracle Scene struct that borrows the original's shapes and owns a lights array with only `position` changed.  The rays are
lens_reference.lens_rays', the fold is progressive_reference.accumulate.  tests/test_soft_abi.py pins this file on the
library's sequence and on progressive_reference.samples and shows it is not vacuous; tests/test_gpu_soft.py holds the GPU to it."""
import ctypes as C

import numpy as np

import lens_reference as LR
import progressive_reference as PR
import radiance_reference as RR

TIGHT = PR.TIGHT                     # the project's parity bound, per channel, no pixel left out
MAX_SAMPLES = PR.MAX_SAMPLES
GOLDEN = 0.6180339887498949          # the shift of the light sequence from one light to the next
# Pixels of a 32 x 32 frame (aperture 0, radii 1.5 for every light, the library's two sequences) whose soft mean differs from the
# hard-shadow mean of the same table by more than 0.05 in some channel, counted with the oracle alone
# (tests/test_soft_abi.py): name -> (depth, rows, pixels)
SOFTENED = {"demo": (3, 64, 197), "synthetic256": (6, 16, 16), "penumbra": (3, 64, 68)}


def light_sequence(first, count, radii):
    """rm_light_sequence: rows first .. first + count - 1, (count, len(radii), 3) offsets, every operation rounded once in the
    header's order: light l of row s is radii[l] times a point of the unit sphere."""
    radii = [np.float64(r) for r in radii]
    assert first >= 0 and count >= 0 and first + count <= MAX_SAMPLES
    assert all(np.isfinite(r) and r >= 0. for r in radii)
    off = np.empty((count, len(radii), 3))
    for k in range(count):
        r11, q11 = PR.digit_reversed(first + k, 11)
        r13, q13 = PR.digit_reversed(first + k, 13)
        p11, p13 = np.float64(r11) / np.float64(q11), np.float64(r13) / np.float64(q13)
        for l, radius in enumerate(radii):
            x = p11 + np.float64(l) * GOLDEN
            x = x - np.floor(x)
            y = p13 + np.float64(l) * GOLDEN
            y = y - np.floor(y)
            a, b = 2. * x - 1., 2. * y - 1.
            u, v = a * np.sqrt(1. - b * b / 2.), b * np.sqrt(1. - a * a / 2.)
            r2 = u * u + v * v
            h = 2. * np.sqrt(np.fmax(1. - r2, 0.))
            off[k, l] = (radius * (u * h), radius * (v * h), radius * (1. - 2. * r2))
    return off


def random_offsets(rng, count, n_lights, scale=2.):
    """An offset table that is not the library's: another offset for every row and every light, none of them zero."""
    off = rng.uniform(-scale, scale, (count, n_lights, 3))
    off[np.abs(off) < 1e-3] = 0.5
    return off


class MovedScene:
    """An oracle Scene struct whose shapes are the source scene's and whose lights are its own; .ptr as OracleScene's."""

    def __init__(self, O, oscene, offsets_row):
        src = oscene.c
        off = np.asarray(offsets_row, dtype=np.float64).reshape(-1, 3)
        assert off.shape[0] == src.n_lights
        self.source = oscene                                         # the shapes are borrowed: keep their owner alive
        self.lights = (O.Light * max(1, src.n_lights))()
        for l in range(src.n_lights):
            lt = src.lights[l]
            p = O.Vec3(float(np.float64(lt.position.x) + off[l, 0]), float(np.float64(lt.position.y) + off[l, 1]),
                       float(np.float64(lt.position.z) + off[l, 2]))     # one addition, rounded once
            self.lights[l] = O.Light(p, O.Vec3(lt.color.x, lt.color.y, lt.color.z), lt.intensity)
        self.struct = O.Scene(C.cast(self.lights, C.POINTER(O.Light)), src.n_lights, src.shapes, src.n_shapes,
                              O.Vec3(src.camera.x, src.camera.y, src.camera.z))
        self.ptr = C.pointer(self.struct)

    @property
    def c(self):
        return self.struct


def moved_scene(O, oscene, offsets_row):
    """`oscene` with light l at position + offsets_row[l]; colour and intensity copied as they are (orc_scene_add_light would
    normalise the colour a second time)."""
    return MovedScene(O, oscene, offsets_row)


def samples(O, orc, oscene, eye, basis, width, height, depth, aperture, focus, table, offsets):
    """The radiance of every lens ray of the rows a frame writes, row s shaded with the lights at offsets[s]:
    [pixel][s][3], pixels row-major."""
    rows = LR.rows_of(height)
    table, offsets = np.asarray(table, dtype=np.float64), np.asarray(offsets, dtype=np.float64)
    n = table.shape[0]
    assert offsets.shape[0] == n
    o, d = LR.lens_rays(width, rows, orc.renderer(width, height), eye, basis, aperture, focus, table)
    o, d = o.reshape(rows * width, n, 3), d.reshape(rows * width, n, 3)
    out = np.empty((rows * width, n, 3))
    for s in range(n):
        out[:, s] = orc.cast(moved_scene(O, oscene, offsets[s]), np.ascontiguousarray(o[:, s]), np.ascontiguousarray(d[:, s]),
                             depth, normalize=True)
    return out


def frames(O, orc, oscene, eye, basis, width, height, depth, aperture, focus, table, offsets, passes):
    """progressive_reference.frames with the offset table: (sum, mean) after the passes, each [height][width][3]."""
    rows = LR.rows_of(height)
    assert sum(passes) == np.asarray(table).shape[0]
    s = samples(O, orc, oscene, eye, basis, width, height, depth, aperture, focus, table, offsets)
    acc, mean, done = None, None, 0
    for n in passes:
        acc, mean = PR.accumulate(acc, s[:, done:done + n], done)
        done += n
    out_sum, out_mean = np.zeros((height, width, 3)), np.zeros((height, width, 3))
    out_sum[:rows], out_mean[:rows] = acc.reshape(rows, width, 3), mean.reshape(rows, width, 3)
    return out_sum, out_mean


# ---------------------------------------------------------------- the penumbra scene
# A floor, a glass sphere above it and a light overhead: the sphere's shadow lies in the middle of the view.  The second light
# sits below the floor plane, so every lane that shades the floor has its first two lights on opposite sides of its surface (and
# lanes on the sphere mostly do not); the third makes the count odd: the last light walks alone.
# (the reference's polygon test looks at the projection on the xy-plane -- polygon.rs:54-56 --, so a floor has to be tilted to
# be seen at all: this one rises away from the camera as the demo's does, in the demo floor's vertex order)
PENUMBRA_FLOOR = [(14., -3., -34.), (-14., -3., -34.), (-12., -6., -3.), (12., -6., -3.)]
PENUMBRA_FLOOR_MATERIAL = dict(diffusion=1., diffuse_color=(0.8, 0.8, 0.7), specular=0.3, specular_exponent=20.,
                               is_glass_like=False, reflection=0., refractive_index=1.)
PENUMBRA_SPHERE = ((0., -2., -9.), 2.)
PENUMBRA_LIGHTS = [((0., 8., -9.), (1., 1., 1.), 1.), ((3., -14., -10.), (0.5, 0.5, 1.), 0.6), ((-8., 5., -2.), (1., 0.6, 0.4), 0.5)]
PENUMBRA_RADII = (1.5, 1.5, 1.5)


def penumbra_scenes(pkg, O):
    """-> (product Scene, oracle scene), from the one recipe above."""
    s, o = pkg.Scene.new(), O.OracleScene()
    V = pkg.Vec3f
    s.shapes.append(pkg.polygon.ConvexPolygon.create([V(*p) for p in PENUMBRA_FLOOR], pkg.Reflectance(**PENUMBRA_FLOOR_MATERIAL)))
    o.add_polygon(PENUMBRA_FLOOR, O.reflectance(**PENUMBRA_FLOOR_MATERIAL))
    s.shapes.append(pkg.sphere.create(V(*PENUMBRA_SPHERE[0]), PENUMBRA_SPHERE[1], pkg.Reflectance(**RR.GLASS)))
    o.add_sphere(PENUMBRA_SPHERE[0], PENUMBRA_SPHERE[1], O.reflectance(**RR.GLASS))
    for pos, col, inten in PENUMBRA_LIGHTS:
        s.lights.append(pkg.create_light(V(*pos), V(*col), inten))
        o.add_light(pos, col, inten)
    return s, o


class Yardstick(PR.Yardstick):
    """PR.Yardstick with the penumbra scene and reference soft frames, each made once and shared (never written to)."""

    def __init__(self, pkg, O, orc):
        super().__init__(pkg, O, orc)
        self._soft = {}

    def scene(self, name):
        if name == "penumbra" and name not in self._scene:
            self._scene[name] = penumbra_scenes(self.pkg, self.O)
        return super().scene(name)

    def n_lights(self, name):
        return int(self.scene(name)[1].c.n_lights)

    def soft(self, name, w, h, depth, aperture, focus, table, offsets, passes, view=None):
        """(sum, mean) after the passes over `table` and `offsets`; view = (eye, basis) of an oriented context, None: the fixed view."""
        t = np.ascontiguousarray(table, dtype=np.float64)
        f = np.ascontiguousarray(offsets, dtype=np.float64)
        key = (name, w, h, depth, float(aperture), float(focus), t.tobytes(), f.tobytes(), tuple(passes), view)
        if key not in self._soft:
            eye, basis = (self.eye(name), None) if view is None else view
            pair = frames(self.O, self.orc, self.scene(name)[1], eye, basis, w, h, depth, aperture, focus, t, f, passes)
            for a in pair:
                a.setflags(write=False)
            self._soft[key] = pair
        return self._soft[key]
