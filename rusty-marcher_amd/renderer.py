"""`Renderer` / `create_renderer` of engine/src/renderer.rs:17-126.  render() keeps
the reference's contract -- synchronous, fills the caller's FrameBuffer, returns the
status string -- and runs the patch loop on the MI355X through the C ABI."""
import collections
import ctypes as C
import time

from . import _lib, backend
from .geometry import Vec3f

# What is under a pixel: Intersection (shapes.rs:3-8) without the reflectance, with the ray parameter and where in
# Scene.shapes it lies (shape: index into scene.shapes; element: the triangle inside an Obj, 0 otherwise).
PickHit = collections.namedtuple("PickHit", "t point normal shape element")


class Renderer:
    def __init__(self, fov, height, width):
        p = backend.make_params(fov, height, width)
        self.fov, self.half_fov, self.height, self.width, self.ratio = (p.fov, p.half_fov, p.height,
                                                                        p.width, p.ratio)
        # The reference hard-codes the recursion cap (renderer.rs:262); exposed here.
        self.max_depth = 3
        self.device = 0
        self.last_timing = None
        self.last_refined = None                                           # render_antialiased: pixels it refined
        self.last_samples = None                                           # render_progressive: samples a pixel in its frame
        self.last_report = None                                            # render_converging, render_converging_motion, render_converging_moving: the last tick's rm_converge_report

    def render(self, frame, scene):
        t0 = time.perf_counter()
        ctx = backend.default_context(self.device)
        if frame.height % 32 != 0 or frame.width % 32 != 0:
            print("Dimensions mismatch")                                   # renderer.rs:49-51
        n_patches = (frame.height // 32) * (frame.width // 32)
        print("Rendering using patches of size %d, using %d patches overall" % (32, n_patches))

        p = backend.make_params(self.fov, self.height, self.width, self.max_depth)
        p.frame_width, p.frame_height = frame.width, frame.height         # renderer.rs:53-54
        handle = scene.flatten()
        ctx.upload(handle)
        ctx.orient(getattr(scene, "basis", None))                        # (the default context is shared: None resets)
        self.last_timing = ctx.render(p, frame.buffer)

        ms = int((time.perf_counter() - t0) * 1000.)                      # renderer.rs:111-112
        buf = C.create_string_buffer(256)
        _lib.lib().rm_format_status(buf, 256, ms, frame.width, frame.height)
        message = buf.value.decode()
        print(message)
        info = ctx.device_info()
        print("%d compute units used" % info["cus"])                     # renderer.rs:124 prints the thread count
        return message

    def render_supersampled(self, frame, scene, n):
        """render() with n x n rays a pixel: pixel (x, y) is the mean of the radiance at (x + i/n, y + j/n), i, j in
        0..n-1 -- no pixel-centre offset, so n = 1 casts the render's own ray.  One radiance query over sample positions
        built on the device (rm_radiance_samples_device), averaged there in float64; the whole patch rows of
        frame.buffer are filled, rows from height - height % 32 on are left untouched, as render() leaves them."""
        if int(n) != n or not 1 <= n <= 8:
            raise ValueError("n must be an integer in 1..8, got %r" % (n,))
        n = int(n)
        import torch
        t0 = time.perf_counter()
        ctx = backend.default_context(self.device)
        if frame.height % 32 != 0 or frame.width % 32 != 0:
            print("Dimensions mismatch")                                   # renderer.rs:49-51
        rows = (frame.height // 32) * 32
        print("Rendering using patches of size %d, using %d patches overall" % (32, (frame.height // 32) * (frame.width // 32)))

        p = backend.make_params(self.fov, self.height, self.width, self.max_depth)
        p.frame_width, p.frame_height = frame.width, frame.height
        ctx.upload(scene.flatten())
        ctx.orient(getattr(scene, "basis", None))
        if rows:
            dev = torch.device("cuda:%d" % self.device)
            f64 = torch.float64
            sub = torch.arange(n, dtype=f64, device=dev) / n               # i / n: one rounding, as the samples are defined
            sx = (torch.arange(frame.width, dtype=f64, device=dev)[:, None] + sub[None, :])       # [x][i]
            sy = (torch.arange(rows, dtype=f64, device=dev)[:, None] + sub[None, :])              # [y][j]
            xy = torch.empty((rows, frame.width, n, n, 2), dtype=f64, device=dev)                 # [y][x][j][i]
            xy[..., 0] = sx[None, :, None, :]
            xy[..., 1] = sy[:, None, :, None]
            rgb = ctx.radiance_samples_device(p, xy.view(-1, 2))
            mean = rgb.view(rows, frame.width, n * n, 3).sum(dim=2) / float(n * n)
            frame.buffer[:rows] = mean.cpu().numpy()

        ms = int((time.perf_counter() - t0) * 1000.)
        buf = C.create_string_buffer(256)
        _lib.lib().rm_format_status(buf, 256, ms, frame.width, frame.height)
        message = buf.value.decode()
        print(message)
        return message

    def render_antialiased(self, frame, scene, n, threshold):
        """render() with adaptive anti-aliasing (rm_render_antialiased): the frame is rendered once, and every pixel that
        differs from a left / right / upper / lower neighbour by more than `threshold` in a channel -- on the radiance as
        rendered -- is replaced by the mean of the radiance at (x + i/n, y + j/n), i, j in 0..n-1, the samples of
        render_supersampled.  Found, shaded and resolved on the device; the whole patch rows of frame.buffer are filled,
        rows from height - height % 32 on are left untouched.  Prints and returns what render() does; the number of refined
        pixels is left in self.last_refined."""
        backend._refine(n, threshold)                                      # ValueError before the library sees anything
        t0 = time.perf_counter()
        ctx = backend.default_context(self.device)
        if frame.height % 32 != 0 or frame.width % 32 != 0:
            print("Dimensions mismatch")                                   # renderer.rs:49-51
        n_patches = (frame.height // 32) * (frame.width // 32)
        print("Rendering using patches of size %d, using %d patches overall" % (32, n_patches))

        p = backend.make_params(self.fov, self.height, self.width, self.max_depth)
        p.frame_width, p.frame_height = frame.width, frame.height
        ctx.upload(scene.flatten())
        ctx.orient(getattr(scene, "basis", None))
        self.last_timing, self.last_refined = ctx.render_antialiased(p, frame.buffer, n, threshold)

        ms = int((time.perf_counter() - t0) * 1000.)
        buf = C.create_string_buffer(256)
        _lib.lib().rm_format_status(buf, 256, ms, frame.width, frame.height)
        message = buf.value.decode()
        print(message)
        info = ctx.device_info()
        print("%d compute units used" % info["cus"])
        return message

    def render_depth_of_field(self, frame, scene, aperture, focus, n_samples):
        """render() through a thin lens (rm_render_lens): n_samples rays a pixel, each from a point of its own of a lens of
        radius `aperture` towards the point its sample ray reaches at the distance `focus` along the view direction, so
        what lies at that distance is sharp and the rest blurs with the aperture.  The sample table is the library's
        (rm_lens_table); sampled, shaded and averaged on the device.  The whole patch rows of frame.buffer are filled, rows
        from height - height % 32 on are left untouched.  Prints and returns what render() does."""
        backend._lens(aperture, focus, n_samples)                          # ValueError before the library sees anything
        t0 = time.perf_counter()
        ctx = backend.default_context(self.device)
        if frame.height % 32 != 0 or frame.width % 32 != 0:
            print("Dimensions mismatch")                                   # renderer.rs:49-51
        n_patches = (frame.height // 32) * (frame.width // 32)
        print("Rendering using patches of size %d, using %d patches overall" % (32, n_patches))

        p = backend.make_params(self.fov, self.height, self.width, self.max_depth)
        p.frame_width, p.frame_height = frame.width, frame.height
        ctx.upload(scene.flatten())
        ctx.orient(getattr(scene, "basis", None))
        self.last_timing = ctx.render_lens(p, frame.buffer, aperture, focus, ctx.lens_table(n_samples))

        ms = int((time.perf_counter() - t0) * 1000.)
        buf = C.create_string_buffer(256)
        _lib.lib().rm_format_status(buf, 256, ms, frame.width, frame.height)
        message = buf.value.decode()
        print(message)
        info = ctx.device_info()
        print("%d compute units used" % info["cus"])
        return message

    def render_progressive(self, frame, scene, aperture, focus, n_samples, restart=False):
        """A tick of a standing view (rm_render_progressive): n_samples (1..64) more lens samples a pixel of the library's
        unbounded sequence are added on the device to the frame the context keeps, and frame.buffer gets the mean of all of
        them so far.  The frame begins again when `restart` is set or anything it depends on changed since the last tick: the
        renderer, the frame's size, the lens, the camera, the view direction, the scene.  The whole patch rows of frame.buffer
        are filled, rows from height - height % 32 on are left untouched.  Prints and returns what render() does; the
        samples a pixel in the frame are left in self.last_samples (at most 65536: further ticks change nothing)."""
        backend._lens(aperture, focus, n_samples)                          # ValueError before the library sees anything
        return self._tick(frame, scene, lambda ctx, p: ctx.render_progressive(p, aperture, focus, n_samples, restart, host_rgb=frame.buffer))

    def render_progressive_soft(self, frame, scene, light_radii, aperture, focus, n_samples, restart=False):
        """render_progressive with area lights (rm_render_progressive_soft): light l of the scene is a sphere of radius
        light_radii[l] -- one radius a light, 0 for a point -- sampled at another point for every sample, so the frame
        converges to soft shadows.  Beyond what begins a frame again in render_progressive, a changed radius does, and so
        does a switch between the two calls."""
        backend._lens(aperture, focus, n_samples)
        radii = backend._radii(light_radii, len(scene.lights))
        return self._tick(frame, scene, lambda ctx, p: ctx.render_progressive_soft(p, radii, aperture, focus, n_samples, restart,
                                                                                    host_rgb=frame.buffer))

    def render_soft_shadows(self, frame, scene, light_radii, n_samples, aperture=0., focus=1.):
        """One frame with soft shadows: a restarted tick of render_progressive_soft -- n_samples (1..64) samples a pixel, through
        a pinhole unless an aperture is given."""
        return self.render_progressive_soft(frame, scene, light_radii, aperture, focus, n_samples, restart=True)

    def render_progressive_motion(self, frame, scene, velocities, shutter, n_samples, light_radii=None, aperture=0., focus=1., restart=False):
        """render_progressive_soft with moving spheres (rm_render_progressive_motion): shape k of the scene, a sphere, moves by
        velocities[k] -- one Vec3f or None a shape, None or zero for what is not a sphere -- while the shutter stands open for
        `shutter`, and every sample sees it at a time of its own, so the frame converges to a picture blurred along the motion.
        light_radii: one radius a light for area lights, None for points.  Beyond what begins a frame again in
        render_progressive_soft, a changed velocity or shutter does, and so does a switch between the calls.  Every ray of such
        a frame tests every primitive: a hierarchy holds for spheres that stand still."""
        backend._lens(aperture, focus, n_samples)                          # ValueError before the library sees anything
        v = backend._velocities(velocities, len(scene.shapes))
        backend._shutter(shutter)
        radii = backend._radii(light_radii, len(scene.lights)) if light_radii is not None else None
        return self._tick(frame, scene, lambda ctx, p: ctx.render_progressive_motion(p, v, shutter, aperture, focus, n_samples, radii, restart,
                                                                                      host_rgb=frame.buffer))

    def render_motion_blur(self, frame, scene, velocities, shutter, n_samples):
        """One frame with motion blur: a restarted render_progressive_motion ticked in slices of at most 64 until the frame holds
        n_samples samples a pixel, through a pinhole, point lights.  Prints and returns what the last tick does."""
        if isinstance(n_samples, bool) or int(n_samples) != n_samples or not 1 <= n_samples <= backend.PROGRESSIVE_MAX_SAMPLES:
            raise ValueError("n_samples must be an integer in 1..%d, got %r" % (backend.PROGRESSIVE_MAX_SAMPLES, n_samples))
        left, message = int(n_samples), None
        while left > 0:
            step = min(left, 64)
            message = self.render_progressive_motion(frame, scene, velocities, shutter, step, restart=left == n_samples)
            left -= step
        return message

    def render_progressive_moving(self, frame, scene, velocities, shutter, n_samples, light_radii=None, aperture=0., focus=1., restart=False):
        """render_progressive_motion in which every shape moves (rm_render_progressive_moving): shape k of the scene -- a sphere,
        a polygon or a mesh -- moves by velocities[k], one Vec3f or None a shape, while the shutter stands open for `shutter`.
        A polygon's plane point and vertices and a mesh's triangles are moved as the reference's offset() moves them; the
        normals stay.  The frame is not render_progressive_motion's: a switch between the two begins it again."""
        backend._lens(aperture, focus, n_samples)                          # ValueError before the library sees anything
        v = backend._velocities(velocities, len(scene.shapes))
        backend._shutter(shutter)
        radii = backend._radii(light_radii, len(scene.lights)) if light_radii is not None else None
        return self._tick(frame, scene, lambda ctx, p: ctx.render_progressive_moving(p, v, shutter, aperture, focus, n_samples, radii, restart,
                                                                                      host_rgb=frame.buffer))

    def render_moving_shapes(self, frame, scene, velocities, shutter, n_samples):
        """One frame with motion blur of every shape: a restarted render_progressive_moving ticked in slices of at most 64 until
        the frame holds n_samples samples a pixel, through a pinhole, point lights.  Prints and returns what the last tick does."""
        if isinstance(n_samples, bool) or int(n_samples) != n_samples or not 1 <= n_samples <= backend.PROGRESSIVE_MAX_SAMPLES:
            raise ValueError("n_samples must be an integer in 1..%d, got %r" % (backend.PROGRESSIVE_MAX_SAMPLES, n_samples))
        left, message = int(n_samples), None
        while left > 0:
            step = min(left, 64)
            message = self.render_progressive_moving(frame, scene, velocities, shutter, step, restart=left == n_samples)
            left -= step
        return message

    def render_converging(self, frame, scene, tolerance, n_samples, min_samples=16, max_samples=1024, light_radii=None, aperture=0., focus=1.,
                          restart=False):
        """A tick of a converging frame (rm_render_converging): render_progressive -- with area lights where light_radii is
        given, one radius a light -- that casts its n_samples (1..64) more samples only for the pixels still noisy and their
        neighbours.  A pixel is settled once it has min_samples samples and the standard error of the mean of r + g + b is at
        most `tolerance`; none gets more than max_samples.  The frame is the context's own for this call -- render_progressive's
        is left alone -- and begins again as render_progressive_soft's does; the tolerance and the sample numbers may change
        while it goes on.  Prints what render() does and returns the tick's report: .listed pixels sampled by this tick (0: the
        picture is finished, further ticks change nothing), .passes so far, .samples_cast over the frame's life, .max_count the
        most samples a pixel can hold (also left in self.last_samples)."""
        backend._converge(tolerance, min_samples, max_samples, backend._lens(aperture, focus, n_samples).n_samples)
        radii = backend._radii(light_radii, len(scene.lights)) if light_radii is not None else None
        got = []

        def call(ctx, p):
            timing, report = ctx.render_converging(p, aperture, focus, n_samples, tolerance, min_samples, max_samples, radii, restart,
                                                   host_rgb=frame.buffer)
            got.append(report)
            return timing, report.max_count

        self._tick(frame, scene, call)
        self.last_report = got[0]
        return got[0]

    def render_converged(self, frame, scene, tolerance, n_samples, min_samples=16, max_samples=1024, light_radii=None, aperture=0., focus=1.):
        """A finished picture: a restarted render_converging ticked until a tick lists nothing.  -> the last tick's report."""
        report = self.render_converging(frame, scene, tolerance, n_samples, min_samples, max_samples, light_radii, aperture, focus, restart=True)
        while report.listed > 0:
            report = self.render_converging(frame, scene, tolerance, n_samples, min_samples, max_samples, light_radii, aperture, focus)
        return report

    def render_progressive_bounce(self, frame, scene, n_samples, strength=1., light_radii=None, aperture=0., focus=1., restart=False):
        """render_progressive with one bounce of diffuse light (rm_render_progressive_bounce): where a sample first hits a surface
        that is not glass, one more ray leaves it in a cosine-distributed direction, and what it brings back, times `strength`
        and the surface's diffusion and diffuse colour, is added -- surfaces light each other and colours bleed.  light_radii:
        one radius a light for area lights, None for points.  Static scene, standing camera.  Beyond what begins a frame again
        in render_progressive_soft, a changed strength does, and so does a switch between the calls.  strength=1. is a
        starting value, not a tuned one."""
        backend._lens(aperture, focus, n_samples)                          # ValueError before the library sees anything
        backend._strength(strength)
        radii = backend._radii(light_radii, len(scene.lights)) if light_radii is not None else None
        return self._tick(frame, scene, lambda ctx, p: ctx.render_progressive_bounce(p, aperture, focus, n_samples, strength, radii, restart,
                                                                                      host_rgb=frame.buffer))

    def render_global_illumination(self, frame, scene, n_samples, strength=1.):
        """One frame with bounce light: a restarted render_progressive_bounce ticked in slices of at most 64 until the frame holds
        n_samples samples a pixel, through a pinhole, point lights.  Prints and returns what the last tick does."""
        if isinstance(n_samples, bool) or int(n_samples) != n_samples or not 1 <= n_samples <= backend.PROGRESSIVE_MAX_SAMPLES:
            raise ValueError("n_samples must be an integer in 1..%d, got %r" % (backend.PROGRESSIVE_MAX_SAMPLES, n_samples))
        left, message = int(n_samples), None
        while left > 0:
            step = min(left, 64)
            message = self.render_progressive_bounce(frame, scene, step, strength, restart=left == n_samples)
            left -= step
        return message

    def render_converging_bounce(self, frame, scene, tolerance, n_samples, strength=1., min_samples=16, max_samples=1024, light_radii=None,
                                 aperture=0., focus=1., restart=False):
        """render_converging with one bounce of diffuse light (rm_render_converging_bounce), as render_progressive_bounce adds it:
        only the pixels still noisy go on being sampled.  The frame is render_converging's own: beyond what begins it again
        there, a changed strength does, a switch between the two calls does, and every camera move does, keep_history or not.
        Returns the tick's report, as render_converging does."""
        backend._converge(tolerance, min_samples, max_samples, backend._lens(aperture, focus, n_samples).n_samples)
        backend._strength(strength)
        radii = backend._radii(light_radii, len(scene.lights)) if light_radii is not None else None
        got = []

        def call(ctx, p):
            timing, report = ctx.render_converging_bounce(p, aperture, focus, n_samples, tolerance, min_samples, max_samples, strength, radii,
                                                          restart, host_rgb=frame.buffer)
            got.append(report)
            return timing, report.max_count

        self._tick(frame, scene, call)
        self.last_report = got[0]
        return got[0]

    def render_converged_bounce(self, frame, scene, tolerance, n_samples, strength=1., min_samples=16, max_samples=1024, light_radii=None,
                                aperture=0., focus=1.):
        """A finished picture with bounce light: a restarted render_converging_bounce ticked until a tick lists nothing.
        -> the last tick's report."""
        report = self.render_converging_bounce(frame, scene, tolerance, n_samples, strength, min_samples, max_samples, light_radii, aperture,
                                               focus, restart=True)
        while report.listed > 0:
            report = self.render_converging_bounce(frame, scene, tolerance, n_samples, strength, min_samples, max_samples, light_radii,
                                                   aperture, focus)
        return report

    def keep_history(self, sigma_z=.1, min_normal_dot=.9, max_history=32):
        """History for render_converging, render_converged and render_denoised (rm_converge_history): once the camera moves, the
        frame is no longer begun again but carried to the new view -- every pixel finds the point under it in the previous
        picture and begins with what the samples around it on the same surface held, at most max_history samples' worth; a
        sample is taken only from the same shape, where the normals' dot product exceeds min_normal_dot and the point lies
        within sigma_z (1 + distance) of the pixel's tangent plane.  Pixels that see something new begin at nothing.  Light that
        depends on the view (mirror, glass) is carried as if it stuck to the surface: max_history bounds how long that error
        lives and should stay well under max_samples.  The keyword defaults are starting values, not tuned ones.  The setting is
        the device context's and holds until drop_history()."""
        settings = backend._reproject(sigma_z, min_normal_dot, max_history)   # ValueError before the library sees anything
        backend.default_context(self.device).converge_history(settings)

    def drop_history(self):
        """Turns keep_history off again: a camera move begins the converging frame again, as it does by default."""
        backend.default_context(self.device).converge_history(None)

    def render_denoised(self, frame, scene, sigma_l=4., sigma_z=.1, iterations=5, normal_squarings=5, guides=True, epsilon=1e-10,
                        fallback_variance=1.):
        """The converging frame the last render_converging* call built, filtered (rm_render_denoised): an edge-avoiding a-trous
        filter of `iterations` (0..5) steps 1, 2, 4, ... steered by each pixel's variance -- a settled pixel passes almost
        untouched, a noisy one borrows from neighbours whose r + g + b lies within about sigma_l standard errors -- and, with
        `guides`, by the hits under the pixels: nothing is borrowed across a silhouette, from a surface that faces another way
        (the normals' dot product to the power 2^normal_squarings) or from off the pixel's tangent plane (sigma_z, relative to
        1 + the hit's distance).  The guide is the pinhole view: turn it off under a wide aperture, a moving camera or strongly
        moving shapes.  The frame must be the one that call rendered into (same size); the converging frame itself is left
        alone and its next tick continues it.  The keyword defaults are starting values, not tuned ones.  Prints what render()
        does and returns its message; the samples a pixel holds stay in self.last_samples."""
        backend._denoise(sigma_l, sigma_z, epsilon, fallback_variance, iterations, normal_squarings)
        samples = self.last_samples

        def call(ctx, p):
            return ctx.render_denoised(p, sigma_l, sigma_z, epsilon, fallback_variance, iterations, normal_squarings, guides,
                                       host_rgb=frame.buffer), samples

        return self._tick(frame, scene, call)

    def render_converging_motion(self, frame, scene, velocities, shutter, tolerance, n_samples, min_samples=16, max_samples=1024,
                                 light_radii=None, aperture=0., focus=1., restart=False):
        """render_converging with moving spheres (rm_render_converging_motion): shape k of the scene, a sphere, moves by
        velocities[k] -- one Vec3f or None a shape, None or zero for what is not a sphere -- while the shutter stands open for
        `shutter`, and every sample sees it at a time of its own; only the pixels still noisy, the blurred band among them, go on
        being sampled.  The frame is render_converging's own: beyond what begins it again there, a changed velocity or shutter
        does, and so does a switch between the two calls.  Every ray of such a frame tests every primitive: a hierarchy holds
        for spheres that stand still.  Returns the tick's report, as render_converging does."""
        backend._converge(tolerance, min_samples, max_samples, backend._lens(aperture, focus, n_samples).n_samples)
        v = backend._velocities(velocities, len(scene.shapes))
        backend._shutter(shutter)
        radii = backend._radii(light_radii, len(scene.lights)) if light_radii is not None else None
        got = []

        def call(ctx, p):
            timing, report = ctx.render_converging_motion(p, v, shutter, aperture, focus, n_samples, tolerance, min_samples, max_samples, radii,
                                                          restart, host_rgb=frame.buffer)
            got.append(report)
            return timing, report.max_count

        self._tick(frame, scene, call)
        self.last_report = got[0]
        return got[0]

    def render_converged_motion(self, frame, scene, velocities, shutter, tolerance, n_samples, min_samples=16, max_samples=1024,
                                light_radii=None, aperture=0., focus=1.):
        """A finished picture with motion blur: a restarted render_converging_motion ticked until a tick lists nothing.
        -> the last tick's report."""
        report = self.render_converging_motion(frame, scene, velocities, shutter, tolerance, n_samples, min_samples, max_samples, light_radii,
                                               aperture, focus, restart=True)
        while report.listed > 0:
            report = self.render_converging_motion(frame, scene, velocities, shutter, tolerance, n_samples, min_samples, max_samples, light_radii,
                                                   aperture, focus)
        return report

    def render_converging_moving(self, frame, scene, velocities, shutter, tolerance, n_samples, min_samples=16, max_samples=1024,
                                 light_radii=None, aperture=0., focus=1., restart=False):
        """render_converging_motion in which every shape moves (rm_render_converging_moving): shape k of the scene -- a sphere, a
        polygon or a mesh -- moves by velocities[k], one Vec3f or None a shape, while the shutter stands open for `shutter`.  A
        polygon's plane point and vertices and a mesh's triangles are moved as the reference's offset() moves them; the normals
        stay.  The frame is not render_converging_motion's: a switch between the two begins it again.  Returns the tick's
        report, as render_converging does."""
        backend._converge(tolerance, min_samples, max_samples, backend._lens(aperture, focus, n_samples).n_samples)
        v = backend._velocities(velocities, len(scene.shapes))
        backend._shutter(shutter)
        radii = backend._radii(light_radii, len(scene.lights)) if light_radii is not None else None
        got = []

        def call(ctx, p):
            timing, report = ctx.render_converging_moving(p, v, shutter, aperture, focus, n_samples, tolerance, min_samples, max_samples, radii,
                                                          restart, host_rgb=frame.buffer)
            got.append(report)
            return timing, report.max_count

        self._tick(frame, scene, call)
        self.last_report = got[0]
        return got[0]

    def render_converged_moving(self, frame, scene, velocities, shutter, tolerance, n_samples, min_samples=16, max_samples=1024,
                                light_radii=None, aperture=0., focus=1.):
        """A finished picture with motion blur of every shape: a restarted render_converging_moving ticked until a tick lists
        nothing.  -> the last tick's report."""
        report = self.render_converging_moving(frame, scene, velocities, shutter, tolerance, n_samples, min_samples, max_samples, light_radii,
                                               aperture, focus, restart=True)
        while report.listed > 0:
            report = self.render_converging_moving(frame, scene, velocities, shutter, tolerance, n_samples, min_samples, max_samples, light_radii,
                                                   aperture, focus)
        return report

    def render_progressive_camera(self, frame, scene, camera_velocity, shutter, n_samples, turn=(0., 0., 0.), velocities=None,
                                  light_radii=None, aperture=0., focus=1., restart=False):
        """render_progressive_moving with a moving camera (rm_render_progressive_camera): the camera moves by camera_velocity
        and turns by `turn` = (yaw, pitch, roll) in radians, both a unit of time, while the shutter stands open for `shutter`,
        and every sample sees the scene from a camera of its own, so the frame converges to a view blurred along the camera's
        motion.  velocities: one Vec3f or None a shape, or None where no shape moves -- the scene keeps its hierarchy then.  The
        frame is the call's own: a switch to or from another progressive call begins it again, and so does a changed velocity,
        turn or shutter."""
        backend._lens(aperture, focus, n_samples)                          # ValueError before the library sees anything
        backend._camera_motion(camera_velocity, turn)
        v = backend._velocities(velocities, len(scene.shapes)) if velocities is not None else None
        backend._shutter(shutter)
        radii = backend._radii(light_radii, len(scene.lights)) if light_radii is not None else None
        return self._tick(frame, scene, lambda ctx, p: ctx.render_progressive_camera(p, camera_velocity, shutter, aperture, focus, n_samples, turn,
                                                                                      v, radii, restart, host_rgb=frame.buffer))

    def render_camera_blur(self, frame, scene, camera_velocity, shutter, n_samples, turn=(0., 0., 0.)):
        """One frame with the blur of a moving camera: a restarted render_progressive_camera ticked in slices of at most 64 until
        the frame holds n_samples samples a pixel, through a pinhole, point lights, shapes standing still.  Prints and returns
        what the last tick does."""
        if isinstance(n_samples, bool) or int(n_samples) != n_samples or not 1 <= n_samples <= backend.PROGRESSIVE_MAX_SAMPLES:
            raise ValueError("n_samples must be an integer in 1..%d, got %r" % (backend.PROGRESSIVE_MAX_SAMPLES, n_samples))
        left, message = int(n_samples), None
        while left > 0:
            step = min(left, 64)
            message = self.render_progressive_camera(frame, scene, camera_velocity, shutter, step, turn, restart=left == n_samples)
            left -= step
        return message

    def render_converging_camera(self, frame, scene, camera_velocity, shutter, tolerance, n_samples, turn=(0., 0., 0.), velocities=None,
                                 min_samples=16, max_samples=1024, light_radii=None, aperture=0., focus=1., restart=False):
        """render_converging_moving with a moving camera (rm_render_converging_camera): camera_velocity, turn and velocities as
        render_progressive_camera's.  The frame is the call's own.  Returns the tick's report, as render_converging does."""
        backend._converge(tolerance, min_samples, max_samples, backend._lens(aperture, focus, n_samples).n_samples)
        backend._camera_motion(camera_velocity, turn)
        v = backend._velocities(velocities, len(scene.shapes)) if velocities is not None else None
        backend._shutter(shutter)
        radii = backend._radii(light_radii, len(scene.lights)) if light_radii is not None else None
        got = []

        def call(ctx, p):
            timing, report = ctx.render_converging_camera(p, camera_velocity, shutter, aperture, focus, n_samples, tolerance, min_samples,
                                                          max_samples, turn, v, radii, restart, host_rgb=frame.buffer)
            got.append(report)
            return timing, report.max_count

        self._tick(frame, scene, call)
        self.last_report = got[0]
        return got[0]

    def render_converged_camera(self, frame, scene, camera_velocity, shutter, tolerance, n_samples, turn=(0., 0., 0.), velocities=None,
                                min_samples=16, max_samples=1024, light_radii=None, aperture=0., focus=1.):
        """A finished picture with the blur of a moving camera: a restarted render_converging_camera ticked until a tick lists
        nothing.  -> the last tick's report."""
        report = self.render_converging_camera(frame, scene, camera_velocity, shutter, tolerance, n_samples, turn, velocities, min_samples,
                                               max_samples, light_radii, aperture, focus, restart=True)
        while report.listed > 0:
            report = self.render_converging_camera(frame, scene, camera_velocity, shutter, tolerance, n_samples, turn, velocities, min_samples,
                                                   max_samples, light_radii, aperture, focus)
        return report

    def _tick(self, frame, scene, call):
        """What the progressive renders share: the prints and the return value of render(); call(ctx, params) ->
        (rm_timing, samples a pixel in the frame)."""
        t0 = time.perf_counter()
        ctx = backend.default_context(self.device)
        if frame.height % 32 != 0 or frame.width % 32 != 0:
            print("Dimensions mismatch")                                   # renderer.rs:49-51
        n_patches = (frame.height // 32) * (frame.width // 32)
        print("Rendering using patches of size %d, using %d patches overall" % (32, n_patches))

        p = backend.make_params(self.fov, self.height, self.width, self.max_depth)
        p.frame_width, p.frame_height = frame.width, frame.height
        ctx.upload(scene.flatten())
        ctx.orient(getattr(scene, "basis", None))
        self.last_timing, self.last_samples = call(ctx, p)

        ms = int((time.perf_counter() - t0) * 1000.)
        buf = C.create_string_buffer(256)
        _lib.lib().rm_format_status(buf, 256, ms, frame.width, frame.height)
        message = buf.value.decode()
        print(message)
        info = ctx.device_info()
        print("%d compute units used" % info["cus"])
        return message

    def pick(self, frame, scene, x, y):
        """What render(frame, scene) shows at pixel (x = column, y = row): the closest hit of the ray renderer.rs:80
        casts there (bit for bit the strict render's direction), or None where that ray leaves the scene."""
        ctx = backend.default_context(self.device)
        p = backend.make_params(self.fov, self.height, self.width, self.max_depth)
        p.frame_width, p.frame_height = frame.width, frame.height
        ctx.upload(scene.flatten())
        ctx.orient(getattr(scene, "basis", None))
        h = ctx.pick(p, x, y)
        if not h.hit:
            return None
        return PickHit(h.t, Vec3f(h.point.x, h.point.y, h.point.z), Vec3f(h.normal.x, h.normal.y, h.normal.z), h.shape, h.element)


def create_renderer(fov, height, width):
    """renderer.rs:25-33 -- argument order (fov, height, width)."""
    return Renderer(fov, height, width)
