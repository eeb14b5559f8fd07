"""A second, independent reading of the reference's render path.

Scalar Python, IEEE doubles, one operation at a time in the reference's own
order.  It exists so that the C oracle (``oracle/rm_oracle.c``), on which
every GPU test rests, is itself held to something that was not written by
the same hand from the same reading.

THE WRITING RULE.  This file was written from the Rust source alone
(``engine/src/*.rs`` of the reference), with ``file.rs:line`` cited beside
each function.  ``rm_oracle.c``, ``rm_trace.inc`` and the package's Python
mirror were not opened while it was written, and it is never "fixed" to
agree with them: where the two readings disagree the Rust decides, and the
disagreement is a finding to be written up in DESIGN.md.  If this file is
the one that misread, the misread line is recorded in the section
"Misreadings" below, as evidence of where the Rust is easy to misread.

It is structured the way the Rust is: a shape is an object with
``intersect(orig, dir) -> Intersection | None``, a scene holds a list of
such objects, and ``find_closest_intersect`` / ``intersect_shape_set`` loop
over that list.  No tagged union, no flattened records, no numpy, no fma,
no reassociation, no hypot.  Vectors are tuples of three floats.

It imports nothing of the project.  ``.obj`` text may be handed to it
through ``oracle/obj_oracle.py`` by the tests; this module only takes the
positions and indices.

The one generalisation: the depth cap (``n_recursion > 3`` in
renderer.rs:262) is a parameter, as in the oracle and the product.

Oddities of the reference kept on purpose:
  * ``inside()`` looks at the z of the cross product only;
  * the polygon's parallel test is ``== 0.``, the triangle's ``abs() < 1e-6``;
  * ``dist < 0.`` rejects, so ``dist == 0.`` hits;
  * ties go to the first shape / first triangle (strict ``<``);
  * ``shape_hit as u8`` wraps;
  * a miss gives zero at recursion 1 and the background deeper;
  * shadow origins are offset by 1e-3, children by 1e-4, each side chosen
    by its own dot product; ``reflect_ray`` tests the original normal,
    ``refract_ray`` the possibly flipped one;
  * the specular term is ``(factor * specular).powf(exponent)``;
  * directions are asserted normalised within 1e-4: ``NotNormalised``.

Misreadings: none recorded.
"""

import math
import os
import struct
from collections import namedtuple

PATCH_SIZE = 32                      # renderer.rs:47
BACKGROUND = (0.1, 0.1, 0.1)         # renderer.rs:40-44
DEFAULT_FOV = 1.5                    # main.rs:368


class NotNormalised(AssertionError):
    """The reference's assert![(dir.squared_norm() - 1.).abs() < 1e-4]."""


# --------------------------------------------------------------------------
# geometry.rs
# --------------------------------------------------------------------------

def _fmax(a, b):
    # f64::max: the other operand when one is NaN.
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def _fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a < b else b


def _sqrt(x):
    # f64::sqrt gives NaN below zero; math.sqrt raises there.
    if x < 0.:
        return math.nan
    return math.sqrt(x)


def _powf(x, e):
    # f64::powf never traps.
    try:
        return math.pow(x, e)
    except ValueError:
        return math.nan
    except OverflowError:
        return math.inf


def dot(a, b):                       # geometry.rs:180-182
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def squared_norm(a):                 # geometry.rs:67-69
    return dot(a, a)


def scaled(a, s):                    # geometry.rs:35-39, 49-53
    return (a[0] * s, a[1] * s, a[2] * s)


def add(a, b):                       # geometry.rs:118-128
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def sub(a, b):                       # geometry.rs:163-172
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def mul(a, b):                       # geometry.rs:152-161
    return (a[0] * b[0], a[1] * b[1], a[2] * b[2])


def neg(a):                          # geometry.rs:130-140
    return (-a[0], -a[1], -a[2])


def cross(a, b):                     # geometry.rs:59-65
    return (a[1] * b[2] - a[2] * b[1],
            a[2] * b[0] - a[0] * b[2],
            a[0] * b[1] - a[1] * b[0])


def normalized(a):                   # geometry.rs:19-23, 104-109
    norm = _sqrt(dot(a, a))
    if norm > 0.:
        return scaled(a, 1. / norm)
    return a


def normalized_l0(a):                # geometry.rs:29-33, 111-116
    norm = _fmax(_fmax(a[0], a[1]), a[2])
    if norm > 0.:
        return scaled(a, 1. / norm)
    return a


def _assert_normalised(d):           # sphere.rs:31, polygon.rs:62, triangle.rs:53
    if not (abs(squared_norm(d) - 1.) < 1e-4):
        raise NotNormalised(d)


ZERO = (0., 0., 0.)
ONES = (1., 1., 1.)


# --------------------------------------------------------------------------
# shapes.rs
# --------------------------------------------------------------------------

Reflectance = namedtuple("Reflectance", [       # shapes.rs:21-32
    "diffusion", "diffuse_color", "specular", "specular_exponent",
    "is_glass_like", "reflection", "refractive_index"])

Intersection = namedtuple("Intersection",       # shapes.rs:4-8
                          ["point", "normal", "reflectance"])


def default_reflectance():           # shapes.rs:50-60
    return Reflectance(diffusion=1., diffuse_color=ONES, specular=1.,
                       specular_exponent=30., is_glass_like=False,
                       reflection=0.95, refractive_index=1.)


def intersect_shape_set(orig, dir, shapes):     # shapes.rs:92-108
    for shape in shapes:
        if shape.intersect(orig, dir) is not None:
            return True
    return False


def find_closest_intersect(orig, dir, shapes):  # shapes.rs:110-143
    final = None
    hit = False
    shape_hit = 0
    dist_closest = 0.
    for shape_index, shape in enumerate(shapes):
        test = shape.intersect(orig, dir)
        if test is not None:
            dist_hit = squared_norm(sub(test.point, orig))
            if (not hit) or dist_hit < dist_closest:
                final = test
                hit = True
                shape_hit = shape_index
                dist_closest = dist_hit
    if hit:
        return final, shape_hit & 0xFF           # `as u8`, shapes.rs:140
    return None


# --------------------------------------------------------------------------
# sphere.rs
# --------------------------------------------------------------------------

class Sphere:
    def __init__(self, center, radius, reflectance):     # sphere.rs:13-23
        self.center = center
        self.radius_square = radius * radius
        self.reflectance = reflectance

    def intersect(self, orig, dir):                      # sphere.rs:27-61
        line = sub(self.center, orig)
        _assert_normalised(dir)
        tca = dot(line, dir)
        d2 = dot(line, line) - tca * tca
        if d2 > self.radius_square:
            return None
        thc = _sqrt(self.radius_square - d2)
        t0 = tca - thc
        t1 = tca + thc
        if t0 < 0.:
            t0 = t1
        if t0 < 0.:
            return None
        point = add(orig, scaled(dir, t0))
        return Intersection(point, normalized(sub(point, self.center)),
                            self.reflectance)


# --------------------------------------------------------------------------
# polygon.rs
# --------------------------------------------------------------------------

def inside(a, p1, p2):               # polygon.rs:54-56, triangle.rs:13-15
    return cross(sub(p1, a), sub(p2, a))[2] > 0.


class ConvexPolygon:
    def __init__(self, vertices, reflectance):           # polygon.rs:16-42
        assert len(vertices) > 2
        self.vertices = [tuple(v) for v in vertices]
        self.reflectance = reflectance
        mean = ZERO
        for v in self.vertices:
            mean = add(mean, v)
        mean = scaled(mean, 1. / float(len(self.vertices)))
        edge_1 = sub(self.vertices[1], self.vertices[0])
        edge_2 = sub(self.vertices[2], self.vertices[1])
        self.plane_normal = normalized(cross(edge_1, edge_2))
        self.plane_point = mean

    def offset(self, off):                               # polygon.rs:44-49
        self.plane_point = add(self.plane_point, off)
        self.vertices = [add(v, off) for v in self.vertices]

    def intersect(self, orig, dir):                      # polygon.rs:60-98
        _assert_normalised(dir)
        dotprod = dot(dir, self.plane_normal)
        if dotprod == 0.:
            return None
        dist = dot(sub(self.plane_point, orig), self.plane_normal) / dotprod
        if dist < 0.:
            return None
        point = add(orig, scaled(dir, dist))
        n = len(self.vertices)
        for i in range(n):
            if not inside(point, self.vertices[i], self.vertices[(i + 1) % n]):
                return None
        return Intersection(point, self.plane_normal, self.reflectance)


# --------------------------------------------------------------------------
# triangle.rs
# --------------------------------------------------------------------------

class Triangle:
    def __init__(self, vertices):                        # triangle.rs:33-47
        assert len(vertices) == 3
        self.vertices = [tuple(v) for v in vertices]
        v = self.vertices
        mean = scaled(add(add(v[0], v[1]), v[2]), 1. / 3.)
        edge_1 = sub(v[1], v[0])
        edge_2 = sub(v[2], v[1])
        self.normal = normalized(cross(edge_1, edge_2))
        self.center = mean

    def offset(self, off):                               # triangle.rs:19-24
        self.center = add(self.center, off)
        self.vertices = [add(v, off) for v in self.vertices]

    def intersect(self, orig, dir):                      # triangle.rs:49-83
        _assert_normalised(dir)
        dot_product = dot(dir, self.normal)
        if abs(dot_product) < 1e-6:
            return None
        dist = dot(sub(self.center, orig), self.normal) / dot_product
        if dist < 0.:
            return None
        point = add(orig, scaled(dir, dist))
        for i in range(3):
            if not inside(point, self.vertices[i], self.vertices[(i + 1) % 3]):
                return None
        return Intersection(point, self.normal, default_reflectance())


# --------------------------------------------------------------------------
# obj.rs (what follows the parser)
# --------------------------------------------------------------------------

def widen_f32(x):
    """`positions[k] as f64` (obj.rs:103-105): the value an f32 holds."""
    return struct.unpack("f", struct.pack("f", x))[0]


class Obj:
    def __init__(self, positions, indices, widen=widen_f32):   # obj.rs:79-146
        """positions: flat x,y,z floats (rounded to f32 here, as tobj
        stores them); indices: flat, three per triangle.  ``widen=float``
        is for synthetic meshes whose vertices never were f32 (the render
        fuzz hands the oracle and the product doubles too)."""
        n_triangles = len(indices) // 3
        self.triangles = []
        for t in range(n_triangles):
            vertices = []
            for v in range(3):
                i_v = int(indices[t * 3 + v])
                vertices.append((widen(positions[3 * i_v]),
                                 widen(positions[3 * i_v + 1]),
                                 widen(positions[3 * i_v + 2])))
            self.triangles.append(Triangle(vertices))
        self.reflectances = []
        for t in range(n_triangles):                     # obj.rs:125-138
            t_f = float(t)
            self.reflectances.append(default_reflectance()._replace(
                diffuse_color=(1. - t_f / float(n_triangles),
                               t_f / float(n_triangles),
                               1.)))

    def offset(self, off):                               # obj.rs:24-29
        for t in self.triangles:
            t.offset(off)

    def intersect(self, orig, dir):                      # obj.rs:186-216
        final = None
        hit_triangle = False
        dist_closest = 0.
        for i, t in enumerate(self.triangles):
            res = t.intersect(orig, dir)
            if res is not None:
                dist_hit = squared_norm(sub(res.point, orig))
                if (not hit_triangle) or dist_hit < dist_closest:
                    final = Intersection(res.point, res.normal,
                                         self.reflectances[i])
                    hit_triangle = True
                    dist_closest = dist_hit
        if hit_triangle:
            return final
        return None


# --------------------------------------------------------------------------
# optics.rs
# --------------------------------------------------------------------------

def reflect(incident, normal):                           # optics.rs:4-6
    return sub(incident, scaled(normal, 2. * dot(incident, normal)))


def reflect_ray(incident, intersection, refractive_index):   # optics.rs:8-48
    normal = intersection.normal
    c = dot(normal, incident)
    r = refractive_index if c < 0. else 1. / refractive_index
    if c < 0.:
        c = -c
        normal = neg(normal)
    cos_theta_2 = 1. - r * r * (1. - c * c)
    if cos_theta_2 > 0.:
        return None
    reflected = reflect(incident, normal)
    if dot(reflected, intersection.normal) < 0.:         # the ORIGINAL normal
        orig = sub(intersection.point, scaled(intersection.normal, 1e-4))
    else:
        orig = add(intersection.point, scaled(intersection.normal, 1e-4))
    return orig, reflected


def refract_ray(incident, intersection, refractive_index):   # optics.rs:50-89
    normal = intersection.normal
    c = -dot(normal, incident)
    r = refractive_index if c < 0. else 1. / refractive_index
    if c < 0.:
        c = -c
        normal = neg(normal)
    cos_theta_2 = 1. - r * r * (1. - c * c)
    if cos_theta_2 < 0.:
        return None
    refracted = normalized(add(scaled(incident, r),
                               scaled(normal, r * c - _sqrt(cos_theta_2))))
    if dot(refracted, normal) > 0.:                      # the FLIPPED normal
        orig = add(intersection.point, scaled(normal, 1e-4))
    else:
        orig = sub(intersection.point, scaled(normal, 1e-4))
    return orig, refracted


# --------------------------------------------------------------------------
# lights.rs, scene.rs
# --------------------------------------------------------------------------

class Light:
    def __init__(self, position, color, intensity):      # lights.rs:10-16
        self.position = position
        self.color = normalized_l0(color)
        self.intensity = intensity


class Scene:
    def __init__(self):                                  # scene.rs:16-23
        self.lights = []
        self.shapes = []
        self.camera = ZERO

    def offset_camera(self, offset):                     # scene.rs:25-27
        self.camera = add(self.camera, offset)

    @staticmethod
    def create_default():                                # scene.rs:28-211
        r = default_reflectance()
        r = r._replace(diffuse_color=(0.8, 0., 0.), specular_exponent=100.)
        sphere_red = Sphere((-5., 0., -16.), 4., r)

        r = r._replace(diffuse_color=(0.6, 0., 0.7))
        triangle = ConvexPolygon(
            [(7., -4., -8.), (15., 0., -9.), (6., 3., -8.)], r)

        r = r._replace(diffusion=1.0, specular=1., is_glass_like=True,
                       refractive_index=1.5, reflection=0.5,
                       diffuse_color=(0.3, 0.9, 0.9))
        square = ConvexPolygon(
            [(20., -3., -50.), (-20., -3., -50.),
             (-15., -6., -3.), (15., -6., -3.)], r)

        r = r._replace(specular=1.0, diffusion=0.1,
                       diffuse_color=(0., 0., 0.2), is_glass_like=True,
                       refractive_index=1.5, reflection=0.2)
        sphere_blue = Sphere((-0.5, -1.5, -5.), 2., r)

        r = r._replace(diffusion=1., reflection=1., is_glass_like=False,
                       specular=0.8, diffuse_color=(0., 1., 0.))
        sphere_green = Sphere((6., -0.5, -18.), 3., r)

        r = r._replace(diffuse_color=(0.9, 0.9, 0.9))
        sphere_white = Sphere((-10., 6., -14.), 4., r)

        scene = Scene()
        scene.lights = [Light((0., 0., 0.), ONES, 1.),
                        Light((20., 20., 20.), (1., 0.5, 0.5), 0.8)]
        scene.shapes = [sphere_blue, sphere_green, sphere_red, sphere_white,
                        triangle, square]
        scene.camera = ZERO
        return scene


# --------------------------------------------------------------------------
# renderer.rs
# --------------------------------------------------------------------------

class Tally:
    """What one primary ray met; filled in by cast_ray when handed one.
    Counting only: no arithmetic depends on it."""
    __slots__ = ("first", "blocked", "primary_blocked", "tir")

    def __init__(self):
        self.first = None            # (Intersection, u8 index) of the primary
        self.blocked = 0             # shadow tests that found an occluder
        self.primary_blocked = 0     # ... of those, at the primary hit
        self.tir = 0                 # refract_ray calls that gave None


def diffusion_factor(intersection, light_dir):           # renderer.rs:138-140
    return _fmax(dot(light_dir, intersection.normal), 0.)


def specular_factor(intersection, origin, light_dir):    # renderer.rs:142-151
    incident = neg(light_dir)
    reflected = reflect(incident, intersection.normal)
    dir_to_viewer = normalized(sub(origin, intersection.point))
    return _fmax(dot(reflected, dir_to_viewer), 0.)


def direct_lighting(origin, intersection, shapes, lights, tally=None):
    # renderer.rs:153-193
    light_intensity = ZERO
    refl = intersection.reflectance
    for light in lights:
        light_dir = normalized(sub(light.position, intersection.point))
        if dot(light_dir, intersection.normal) < 0.:
            intersect_orig = sub(intersection.point,
                                 scaled(intersection.normal, 1e-3))
        else:
            intersect_orig = add(intersection.point,
                                 scaled(intersection.normal, 1e-3))
        if intersect_shape_set(intersect_orig, light_dir, shapes):
            if tally is not None:
                tally.blocked += 1
            continue
        diffusion = diffusion_factor(intersection, light_dir)
        light_intensity = add(
            light_intensity,
            scaled(scaled(mul(light.color, refl.diffuse_color), diffusion),
                   light.intensity))
        specular = _powf(
            specular_factor(intersection, origin, light_dir) * refl.specular,
            refl.specular_exponent)
        light_intensity = add(light_intensity, scaled(light.color, specular))
    return scaled(light_intensity, refl.diffusion)


def reflected_lighting(incident, intersection, shapes, lights, background,
                       n_recursion, max_depth, tally=None):
    # renderer.rs:195-222
    reflection = reflect_ray(incident, intersection,
                             intersection.reflectance.refractive_index)
    if reflection is not None:
        return scaled(cast_ray(reflection[0], reflection[1], shapes, lights,
                               background, n_recursion + 1, max_depth, tally),
                      intersection.reflectance.reflection)
    return ZERO


def refracted_lighting(incident, intersection, shapes, lights, background,
                       n_recursion, max_depth, tally=None):
    # renderer.rs:225-252
    refracted = refract_ray(incident, intersection,
                            intersection.reflectance.refractive_index)
    if refracted is not None:
        return scaled(cast_ray(refracted[0], refracted[1], shapes, lights,
                               background, n_recursion + 1, max_depth, tally),
                      1. - intersection.reflectance.reflection)
    if tally is not None:
        tally.tir += 1
    return ZERO


def cast_ray(orig, dir, shapes, lights, background, n_recursion,
             max_depth=3, tally=None):
    # renderer.rs:254-309; `> 3` generalised to `> max_depth`.
    if n_recursion > max_depth:
        return background
    result = find_closest_intersect(orig, dir, shapes)
    if tally is not None and n_recursion == 1:
        tally.first = result
    if result is None:
        if n_recursion > 1:
            return background
        return ZERO
    intersection = result[0]
    light_intensity = background
    before = tally.blocked if tally is not None else 0
    light_intensity = add(light_intensity,
                          direct_lighting(orig, intersection, shapes, lights,
                                          tally))
    if tally is not None and n_recursion == 1:
        tally.primary_blocked = tally.blocked - before
    if intersection.reflectance.is_glass_like:
        light_intensity = add(
            light_intensity,
            reflected_lighting(dir, intersection, shapes, lights, background,
                               n_recursion, max_depth, tally))
        light_intensity = add(
            light_intensity,
            refracted_lighting(dir, intersection, shapes, lights, background,
                               n_recursion, max_depth, tally))
    return light_intensity


class Renderer:
    def __init__(self, fov, height, width):              # renderer.rs:25-33
        self.fov = fov
        self.half_fov = math.tan(fov / 2.)
        self.height = float(height)
        self.width = float(width)
        self.ratio = self.width / self.height

    def backproject(self, i, j):                         # renderer.rs:128-135
        return normalized((
            2. * (float(i) / self.width - 0.5) * self.half_fov * self.ratio,
            -2. * (float(j) / self.height - 0.5) * self.half_fov,
            -1.))

    def render_patch(self, p, n_width, scene, max_depth=3, probe=False):
        # The closure of renderer.rs:65-88.
        buffer = []
        tallies = [] if probe else None
        p_line = p % n_width * PATCH_SIZE
        p_col = p // n_width * PATCH_SIZE
        for i in range(p_col, p_col + PATCH_SIZE):
            for j in range(p_line, p_line + PATCH_SIZE):
                tally = Tally() if probe else None
                buffer.append(cast_ray(scene.camera, self.backproject(j, i),
                                       scene.shapes, scene.lights, BACKGROUND,
                                       1, max_depth, tally))
                if probe:
                    first = tally.first
                    tallies.append((
                        first is not None,
                        first[1] if first is not None else -1,
                        bool(first is not None
                             and first[0].reflectance.is_glass_like),
                        tally.primary_blocked, tally.tir,
                        first[0].point if first is not None else None))
        return buffer, tallies

    def render(self, frame, scene, max_depth=3, workers=1, probe=False):
        """renderer.rs:36-126.  Patches of 32x32; rows at or past
        ``height - height % 32`` (and columns likewise) are never written.
        ``workers > 1`` spreads the patches over processes, as the
        reference spreads them over threads.  With ``probe`` returns
        {(row, col): (hit, index, glass, primary_blocked, tir, point)}."""
        if frame.width % PATCH_SIZE != 0:
            # The reference prints "Dimensions mismatch" and its reassembly
            # (renderer.rs:107) then walks off the patch grid.
            raise ValueError("width must be a multiple of the patch size")
        n_height = frame.height // PATCH_SIZE
        n_width = frame.width // PATCH_SIZE
        n_patches = n_height * n_width
        jobs = [(self, p, n_width, scene, max_depth, probe)
                for p in range(n_patches)]
        if workers > 1 and n_patches > 1:
            import multiprocessing
            ctx = multiprocessing.get_context("spawn")
            with ctx.Pool(min(workers, n_patches)) as pool:
                render_queue = pool.map(_render_patch_job, jobs, chunksize=1)
        else:
            render_queue = [_render_patch_job(job) for job in jobs]

        probes = {} if probe else None
        p_width = 0
        for p, (render_patch, tallies) in enumerate(render_queue):
            p_height = (p // n_width) * PATCH_SIZE       # renderer.rs:95-108
            p_height_end = p_height + PATCH_SIZE
            p_width_end = p_width + PATCH_SIZE
            k = 0
            for j in range(p_height, p_height_end):
                for i in range(p_width, p_width_end):
                    frame.buffer[j][i] = render_patch[k]
                    if probe:
                        probes[(j, i)] = tallies[k]
                    k += 1
            p_width = p_width_end % frame.width
        return probes


def _render_patch_job(job):
    renderer, p, n_width, scene, max_depth, probe = job
    return renderer.render_patch(p, n_width, scene, max_depth, probe)


def pool_size():
    return min(16, os.cpu_count() or 1)


# --------------------------------------------------------------------------
# framebuffer.rs
# --------------------------------------------------------------------------

def quantize(f):                                         # framebuffer.rs:80-82
    return int(255. * _fmin(_fmax(f, 0.), 1.))


class FrameBuffer:
    def __init__(self, width, height):                   # framebuffer.rs:12-22
        self.width = width
        self.height = height
        self.buffer = [[ZERO] * width for _ in range(height)]

    def normalize(self):                                 # framebuffer.rs:58-77
        mx = my = mz = 0.
        for row in self.buffer:
            for px in row:
                mx = _fmax(mx, px[0])
                my = _fmax(my, px[1])
                mz = _fmax(mz, px[2])
        max_val = _fmax(_fmax(mx, my), mz)
        if max_val > 0.:
            s = 1. / max_val
            for row in self.buffer:
                for j in range(self.width):
                    row[j] = scaled(row[j], s)

    def to_vec(self):                                    # framebuffer.rs:40-55
        out = bytearray(self.width * self.height * 3)
        i_ = 0
        for i in range(self.height):
            row = self.buffer[i]
            for j in range(self.width):
                px = row[j]
                out[i_] = quantize(px[0])
                out[i_ + 1] = quantize(px[1])
                out[i_ + 2] = quantize(px[2])
                i_ += 3
        return bytes(out)

    def ppm_bytes(self):                                 # framebuffer.rs:26-38
        header = "P6\n%d %d\n255\n" % (self.width, self.height)
        return header.encode("ascii") + self.to_vec()


def render_frame(scene, width, height, max_depth=3, fov=DEFAULT_FOV,
                 workers=1, probe=False):
    """main.rs:240,364-369 and 329-334: a framebuffer, a renderer sized by
    it, one render.  Returns (frame, probes)."""
    frame = FrameBuffer(width, height)
    renderer = Renderer(fov, height, width)
    probes = renderer.render(frame, scene, max_depth, workers, probe)
    return frame, probes
