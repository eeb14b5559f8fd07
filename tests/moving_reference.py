"""The yardstick of the moving shapes' tests (include/rusty_marcher_amd.h, "moving shapes"): the moving-shapes frame from the
oracle alone.  No GPU, no product code.

As in motion_reference, sample row s of every pixel is orc_cast_ray against one scene that stands as row s of the two offset
tables says.  MovedScene builds that scene with ctypes: an oracle Scene struct that owns a copy of the shapes array, and, unlike
motion_reference.MovedScene, copies of the vertex and triangle arrays of the shapes it moves:
  a sphere    center + off                                                      (as motion_reference)
  a polygon   plane_point + off and every vertex + off; the normal stays        (polygon.rs:44-49)
  an Obj      every triangle's center + off and vertices + off; normals stay    (triangle.rs:19-24, obj.rs:24-29)
each one numpy float64 addition a component.  The rays are lens_reference.lens_rays', the fold is
progressive_reference.accumulate.  tests/test_moving_abi.py pins this file on motion_reference.samples and on the oracle's own
orc_triangle_offset and shows it is not vacuous; tests/test_gpu_moving.py holds the GPU to it."""
import ctypes as C
import os

import numpy as np

import lens_reference as LR
import motion_reference as MR
import progressive_reference as PR
import workloads

TIGHT = MR.TIGHT                     # the project's parity bound, per channel, no pixel left out
GOLDEN = MR.GOLDEN
ORC_SPHERE, ORC_POLYGON, ORC_OBJ = 0, 1, 2       # oracle/rm_oracle.h
SHUTTER = MR.SHUTTER
DODECAHEDRON = os.path.join(workloads.GOLDEN, "dodecahedron.obj")

# The speed of the test velocities of the shapes that are not spheres, in the scene's own units a shutter: the demo, the matrix
# cells and the 256 spheres span tens of units, the meshes of the .obj files hundreds.
SPEED = {"demo": 6., "synthetic256": 6., "pool": 3., "cornell": 150., "dodecahedron": 300.}
CELL_SPEED = 3.
# Pixels of a 32 x 32 frame (aperture 0, point lights, shutter 1, 16 rows of the library's sequences) whose moving-shapes mean,
# with velocities(kinds, SPEED[name]), differs by more than 0.05 in some channel from the mean with motion_reference.velocities
# alone -- only the spheres moving --, counted with the oracle alone (tests/test_moving_abi.py): name -> (depth, rows, pixels).
# In "cornell-one" only Obj CORNELL_MOVER moves.
BLURRED = {"demo": (3, 16, 301), "cornell": (3, 16, 149), "cornell-one": (3, 16, 133), "dodecahedron": (3, 16, 95), "pool": (3, 16, 268),
           "synthetic256": (6, 16, 208)}
# ... and of the nine cells of variant_matrix.CELLS (its aperture and focus, 8 rows, CELL_SPEED): cell id -> pixels
BLURRED_CELLS = {"flat-integer-5": 204, "flat-integer-6": 206, "flat-generic-5": 210, "flat-generic-6": 212, "spheres-integer-5": 207,
                 "spheres-integer-6": 214, "spheres-generic-5": 215, "spheres-generic-6": 221, "mesh-integer-5": 229}
CELL_ROWS = MR.CELL_ROWS
CORNELL_MOVER = 6


def velocities(kinds, speed, only=None):
    """The test velocities: a sphere moves as motion_reference.velocities says; shape k of another kind moves with
    speed x (cos(2 pi g k + 1), 0.5 sin(2 pi g k + 1), 0.25), g the golden ratio's fraction -- every polygon and every Obj a
    velocity that is not zero.  only: the one shape that is not a sphere and moves (the others stand still)."""
    v = MR.velocities(kinds)
    for k, kind in enumerate(kinds):
        if kind != ORC_SPHERE and only in (None, k):
            a = 2. * np.pi * GOLDEN * k + 1.
            v[k] = (speed * np.cos(a), speed * 0.5 * np.sin(a), speed * 0.25)
    return v


def spheres_only(offsets, kinds):
    """The table with zero rows for every shape that is not a sphere."""
    out = np.array(offsets, dtype=np.float64)
    out[:, [k for k, kind in enumerate(kinds) if kind != ORC_SPHERE]] = 0.
    return out


def random_offsets(rng, count, kinds, scale=1.):
    """A shape offset table that is not the library's: another offset for every row and every shape, none of them zero; shapes
    that are not spheres get theirs `scale` times as large."""
    off = MR.random_offsets(rng, count, len(kinds))
    for k, kind in enumerate(kinds):
        if kind != ORC_SPHERE:
            off[:, k] *= scale
    return off


def _moved(O, v, off):
    return O.Vec3(float(np.float64(v.x) + off[0]), float(np.float64(v.y) + off[1]), float(np.float64(v.z) + off[2]))   # one addition, rounded once


def moved_triangle(O, t, off):
    """triangle.rs:19-24: center += off, every vertex += off; the normal stays."""
    out = O.Triangle.from_buffer_copy(bytes(t))
    out.center = _moved(O, t.center, off)
    for i in range(3):
        out.vertices[i] = _moved(O, t.vertices[i], off)
    return out


class MovedScene:
    """An oracle Scene struct with shapes, vertices, triangles and lights of its own: the source's, shape k moved by shape_row[k]
    and light l by light_row[l]; .ptr as OracleScene's.  Materials are borrowed from the source."""

    def __init__(self, O, oscene, light_row, shape_row):
        src = oscene.c
        loff = np.asarray(light_row, dtype=np.float64).reshape(-1, 3)
        soff = np.asarray(shape_row, dtype=np.float64).reshape(-1, 3)
        assert loff.shape[0] == src.n_lights and soff.shape[0] == src.n_shapes
        self.source = oscene                                         # the materials are borrowed: keep their owner alive
        self.lights = (O.Light * max(1, src.n_lights))()
        for l in range(src.n_lights):
            lt = src.lights[l]
            self.lights[l] = O.Light(_moved(O, lt.position, loff[l]), O.Vec3(lt.color.x, lt.color.y, lt.color.z), lt.intensity)
        self.shapes = (O.Shape * max(1, src.n_shapes))()
        if src.n_shapes:
            C.memmove(self.shapes, src.shapes, C.sizeof(O.Shape) * src.n_shapes)      # every field as it is, byte for byte
        self.owned = []                                              # the vertex and triangle arrays of the moved shapes
        for k in range(src.n_shapes):
            s, off = src.shapes[k], soff[k]
            if s.kind == ORC_SPHERE:
                self.shapes[k].center = _moved(O, s.center, off)
            elif s.kind == ORC_POLYGON:                              # polygon.rs:44-49
                verts = (O.Vec3 * max(1, s.n_vertices))()
                for i in range(s.n_vertices):
                    verts[i] = _moved(O, s.vertices[i], off)
                self.owned.append(verts)
                self.shapes[k].vertices = C.cast(verts, C.POINTER(O.Vec3))
                self.shapes[k].plane_point = _moved(O, s.plane_point, off)
            else:                                                    # obj.rs:24-29
                assert s.kind == ORC_OBJ
                tris = (O.Triangle * max(1, s.n_triangles))()
                for i in range(s.n_triangles):
                    tris[i] = moved_triangle(O, s.triangles[i], off)
                self.owned.append(tris)
                self.shapes[k].triangles = C.cast(tris, C.POINTER(O.Triangle))
        self.struct = O.Scene(C.cast(self.lights, C.POINTER(O.Light)), src.n_lights, C.cast(self.shapes, C.POINTER(O.Shape)), src.n_shapes,
                              O.Vec3(src.camera.x, src.camera.y, src.camera.z))
        self.ptr = C.pointer(self.struct)

    @property
    def c(self):
        return self.struct


def samples(O, orc, oscene, eye, basis, width, height, depth, aperture, focus, table, light_offsets, shape_offsets):
    """The radiance of every lens ray of the rows a frame writes, row s shaded with the lights at light_offsets[s] and every
    shape at shape_offsets[s]: [pixel][s][3], pixels row-major."""
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


# ---------------------------------------------------------------- the pool scene
# A pentagon and a hexagon, both tilted towards the camera and counter-clockwise in xy, above the penumbra scene's floor: the
# polygons whose fifth and sixth vertices the device keeps in its vertex pool.  The hexagon is glass: children go through it.
def _ngon(n, centre, radius, tilt):
    out = []
    for i in range(n):
        a = 2. * np.pi * i / n + 0.3
        x, y = radius * np.cos(a), radius * np.sin(a)
        out.append((float(centre[0] + x), float(centre[1] + y), float(centre[2] + tilt * y + 0.1 * x)))
    return out


POOL_PENTAGON = _ngon(5, (-3., 0.5, -11.), 3., 0.5)
POOL_HEXAGON = _ngon(6, (3., 0., -8.), 2.5, -0.4)
POOL_PENTAGON_MATERIAL = dict(diffusion=0.9, diffuse_color=(0.9, 0.4, 0.2), specular=0.5, specular_exponent=20., is_glass_like=False,
                              reflection=0., refractive_index=1.)
POOL_HEXAGON_MATERIAL = dict(diffusion=0.3, diffuse_color=(0.6, 0.8, 0.9), specular=0.8, specular_exponent=30., is_glass_like=True,
                             reflection=0.3, refractive_index=1.5)


def pool_scenes(pkg, O):
    """-> (product Scene, oracle scene), from the one recipe above and soft_reference's penumbra floor, sphere and lights."""
    import radiance_reference as RR
    import soft_reference as SR
    s, o = pkg.Scene.new(), O.OracleScene()
    V = pkg.Vec3f
    for verts, m in ((SR.PENUMBRA_FLOOR, SR.PENUMBRA_FLOOR_MATERIAL), (POOL_PENTAGON, POOL_PENTAGON_MATERIAL), (POOL_HEXAGON, POOL_HEXAGON_MATERIAL)):
        s.shapes.append(pkg.polygon.ConvexPolygon.create([V(*p) for p in verts], pkg.Reflectance(**m)))
        o.add_polygon(verts, O.reflectance(**m))
    s.shapes.append(pkg.sphere.create(V(*SR.PENUMBRA_SPHERE[0]), SR.PENUMBRA_SPHERE[1], pkg.Reflectance(**RR.GLASS)))
    o.add_sphere(SR.PENUMBRA_SPHERE[0], SR.PENUMBRA_SPHERE[1], O.reflectance(**RR.GLASS))
    for pos, col, inten in SR.PENUMBRA_LIGHTS:
        s.lights.append(pkg.create_light(V(*pos), V(*col), inten))
        o.add_light(pos, col, inten)
    return s, o


def dodecahedron_scenes(pkg, O):
    """-> (product Scene, oracle scene) of tests/golden/dodecahedron.obj by the recipe of main.rs:261-327, as workloads builds
    the Cornell box."""
    from oracle import obj_oracle
    o = O.OracleScene()
    for _, tris in obj_oracle.load_models(DODECAHEDRON):
        o.add_obj(np.array(tris, dtype=np.float64), (0., 0., -500.))
    for pos, col, inten in workloads.DEMO_LIGHTS:
        o.add_light(pos, col, inten)
    return pkg.Scene.open_obj(DODECAHEDRON), o


class Yardstick(MR.Yardstick):
    """MR.Yardstick with the pool scene, the dodecahedron and reference moving-shapes frames, each made once and shared."""

    def __init__(self, pkg, O, orc):
        super().__init__(pkg, O, orc)
        self._moving = {}

    def scene(self, name):
        if name not in self._scene and name in ("pool", "dodecahedron"):
            self._scene[name] = pool_scenes(self.pkg, self.O) if name == "pool" else dodecahedron_scenes(self.pkg, self.O)
        return super().scene(name)

    def moving(self, name, w, h, depth, aperture, focus, table, light_offsets, shape_offsets, passes, view=None):
        """(sum, mean) after the passes over `table` and both offset tables; view = (eye, basis) of an oriented context, None:
        the fixed view."""
        t = np.ascontiguousarray(table, dtype=np.float64)
        f = np.ascontiguousarray(light_offsets, dtype=np.float64)
        g = np.ascontiguousarray(shape_offsets, dtype=np.float64)
        key = (name, w, h, depth, float(aperture), float(focus), t.tobytes(), f.tobytes(), g.tobytes(), tuple(passes), view)
        if key not in self._moving:
            eye, basis = (self.eye(name), None) if view is None else view
            pair = frames(self.O, self.orc, self.scene(name)[1], eye, basis, w, h, depth, aperture, focus, t, f, g, passes)
            for a in pair:
                a.setflags(write=False)
            self._moving[key] = pair
        return self._moving[key]
