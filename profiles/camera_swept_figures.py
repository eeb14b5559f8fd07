"""Swept hierarchies under a moving camera, and the moving spheres' ticks through one, on one MI355X.
Three GPU steps, --part pass, --part converge and --part ticks, each a process of its own; run each under a time limit of its own
and chain them with &&:

    timeout -k 10 400 python profiles/camera_swept_figures.py --part pass --out <file> &&
    timeout -k 10 400 python profiles/camera_swept_figures.py --part converge --out <file> &&
    timeout -k 10 400 python profiles/camera_swept_figures.py --part ticks --out <file>

pass.      One pass with all three outputs at 1920x1056, depth 5, n_before = n_samples, 8 and 64 samples, point lights, the rows
           of rm_camera_sequence for a camera that translates and turns: rm_accumulate_camera_device with a shape table (the
           flat walk, the baseline) against rm_accumulate_camera_swept_device over the same rows and buffers -- once with a shape
           offset table of zeros (the refit's boxes are the image's: the price or gain of the walk alone), once with the rows of
           rm_motion_sequence for the test velocities of profiles/swept_figures.py.  The handle is built once a setting from
           rm_swept_extents of the rows, outside the timed region.
converge.  The same columns for a converging pass that lists every pixel (tolerance < 0, every count n_samples beforehand):
           rm_accumulate_converging_camera_device against rm_accumulate_converging_camera_swept_device, memset + select + shade.
ticks.     The moving spheres' ticks, rm_render_progressive_motion and rm_render_converging_motion (tolerance < 0: every pixel
           listed), in two contexts: the default, whose pass goes through the swept kernel, and RM_SWEPT_BVH=0, the flat walk.
           The tick's own kernel_ms (HIP events about its launch); the first tick of a side begins the frame, the others go on.
           Scenes: the 256 spheres and the smallest sphere hierarchy the suite has, tests/swept_reference.py's 17 spheres.

WARM warm-up launches of each side, then REPS of each, interleaved (flat, swept, flat, ...): median, minimum, maximum; the flat
pass's own max / min is the spread a ratio has to leave to mean anything.

Scenes of pass and converge: the Cornell box (36 triangles, the smallest hierarchy in the suite), the 256 spheres, and two
icospheres of profiles/mk_icosphere.py (320 and 1,280 triangles, one mesh each).  Before anything is timed the sides are checked
on 64x64: the swept pass is the flat pass byte for byte, and the velocities are another picture.

Usage: python profiles/camera_swept_figures.py --part pass|converge|ticks [--reps 20] [--out profiles/raw/camera_swept_<part>.txt]
"""
import argparse
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import __graft_entry__ as G  # noqa: E402
import swept_figures as SF  # noqa: E402
import workloads  # noqa: E402

WARM = SF.WARM
WIDTH, HEIGHT, DEPTH, SHUTTER = SF.WIDTH, SF.HEIGHT, SF.DEPTH, SF.SHUTTER
SCENES = SF.SCENES
# the camera over the shutter: a fiftieth of the scene's test speed along (1, 0.4, -0.5), and (yaw, pitch, roll) in radians
CAMERA_TURN = (0.05, 0.02, -0.03)
TICK_SCENES = ("synthetic256", "seventeen")


def camera_velocity(speed):
    return (speed / 50., 0.4 * speed / 50., -0.5 * speed / 50.)


def summary(ms, out, label, verdict):
    med = {side: statistics.median(v) for side, v in ms.items()}
    spread = max(ms["flat"]) / min(ms["flat"])
    ratio = med["swept"] / med["flat"]
    verdict.append(ratio <= spread)
    out.append("  %-22s  flat %9.3f (%9.3f .. %9.3f)   swept %9.3f (%9.3f .. %9.3f)   swept / flat %.4f   flat max / min %.4f"
               % (label, med["flat"], min(ms["flat"]), max(ms["flat"]), med["swept"], min(ms["swept"]), max(ms["swept"]), ratio, spread))


def measure(pkg, ctx, name, part, reps, out, tmp):
    aperture, focus, speed, _ = SCENES[name]
    s = torch.cuda.current_stream()
    f64, u8, i32, dev = torch.float64, torch.uint8, torch.int32, "cuda:0"
    scene = SF.scene_of(pkg, name, tmp)
    ctx.orient(None)
    handle_desc = scene.flatten()
    ctx.upload(handle_desc)
    desc = handle_desc.desc()
    n_lights, n_shapes = ctx.n_lights(), len(scene.shapes)
    velocities = SF.test_velocities(pkg, scene, speed)
    converge = part == "converge"

    def buffers(h, w, fill=0.):
        return dict(sum=torch.full((h, w, 3), fill, dtype=f64, device=dev), stats=torch.full((h, w, 2), fill, dtype=f64, device=dev),
                    count=torch.zeros((h, w), dtype=i32, device=dev), mean=torch.full((h, w, 3), fill, dtype=f64, device=dev),
                    rgb8=torch.zeros((h, w, 3), dtype=u8, device=dev))

    def tables(first, n_rows):
        rows = ctx.motion_sequence(first, n_rows, velocities, SHUTTER)
        camera = ctx.camera_sequence(first, n_rows, camera_velocity(speed), SHUTTER, CAMERA_TURN)
        return (torch.from_numpy(ctx.lens_sequence(first, n_rows)).to(dev), torch.from_numpy(camera).to(dev),
                torch.zeros((n_rows, n_lights, 3), dtype=f64, device=dev),
                {"zero": torch.zeros((n_rows, n_shapes, 3), dtype=f64, device=dev), "velocities": torch.from_numpy(rows).to(dev)})

    def launch(p, b, n, first, table, camera, lights, shapes, swept, ws=None):
        kw = dict(swept=swept) if swept is not None else {}
        if converge:                                                    # (the tables hold rows [0, 2 n): a pixel with count n casts n .. 2 n - 1)
            call = ctx.accumulate_converging_camera_swept_device if swept is not None else ctx.accumulate_converging_camera_device
            call(p, b["sum"], b["stats"], b["count"], aperture, focus, n, table, camera, lights, shapes, -1., 0, 2 * n, False, mean=b["mean"],
                 rgb8=b["rgb8"], workspace=ws, **kw)
        else:
            call = ctx.accumulate_camera_swept_device if swept is not None else ctx.accumulate_camera_device
            call(p, b["sum"], aperture, focus, table, camera, lights, shapes, first, mean=b["mean"], rgb8=b["rgb8"], **kw)

    def handle_for(shapes):
        return ctx.swept(*pkg.backend.swept_extents(shapes.cpu().numpy()))

    # ---- the sides agree before either is timed (64 x 64, rows 8 .. 16 after 8)
    small = pkg.backend.make_params(workloads.FOV, 64., 64., DEPTH)
    first = 0 if converge else 8
    table, camera, lights, both = tables(first, 16 if converge else 8)
    means = {}
    for setting, shapes in both.items():
        handle = handle_for(shapes)
        flat, swept = buffers(64, 64), buffers(64, 64)
        for b in (flat, swept):
            b["count"].fill_(8)
        launch(small, flat, 8, 8, table, camera, lights, shapes, None)
        launch(small, swept, 8, 8, table, camera, lights, shapes, handle)
        torch.cuda.synchronize()
        handle.close()
        for key in flat:
            assert flat[key].cpu().numpy().tobytes() == swept[key].cpu().numpy().tobytes(), "%s, %s: the swept pass is not the flat pass: %s" % (name, setting, key)
        means[setting] = flat["mean"]
    moved = int(((means["velocities"] - means["zero"]).abs() > 0.05).any(dim=2).sum())
    assert moved > 0, "the velocities moved nothing"

    out.append("%s (%d shapes, %d spheres, %d triangles, %d lights; aperture %g, focus %g, speed %g; %d of 4,096 pixels of the 64x64 check differ with the velocities):"
               % (name, n_shapes, desc.n_spheres, desc.n_triangles, n_lights, aperture, focus, speed, moved))
    p = pkg.backend.make_params(workloads.FOV, float(HEIGHT), float(WIDTH), DEPTH)
    b = buffers(HEIGHT, WIDTH)
    ws = torch.empty((ctx.converge_workspace(p) // 4,), dtype=i32, device=dev) if converge else None
    verdict = []
    for n in (8, 64):
        table, camera, lights, both = tables(0 if converge else n, 2 * n if converge else n)
        for setting, shapes in both.items():
            handle = handle_for(shapes)

            def reset():
                if converge:
                    b["count"].fill_(n)

            sides = (("flat", lambda: launch(p, b, n, n, table, camera, lights, shapes, None, ws)),
                     ("swept", lambda: launch(p, b, n, n, table, camera, lights, shapes, handle, ws)))
            for _ in range(WARM):
                for _, fn in sides:
                    reset()
                    fn()
            torch.cuda.synchronize()
            ms = {side: [] for side, _ in sides}
            for _ in range(reps):
                for side, fn in sides:
                    ms[side].append(SF.event_ms(reset, fn, s))
            torch.cuda.synchronize()
            handle.close()
            summary(ms, out, "%2d samples, %s" % (n, setting), verdict)
    out.append("  swept not slower than flat by more than flat's own spread in %d of %d rows" % (sum(verdict), len(verdict)))
    out.append("")


def tick_scene(pkg, name):
    if name != "seventeen":
        return workloads.product_scene(pkg, name), SCENES[name][:2]
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import swept_reference as SW                                        # (the suite's own 17 spheres; no oracle is asked for)
    scene = pkg.Scene.new()
    for k, (c, r) in enumerate(SW.seventeen_spheres()):
        m = SW._GLASS if k % 5 == 0 else dict(SW._OPAQUE, diffuse_color=(0.2 + 0.04 * k, 0.9 - 0.04 * k, 0.5))
        scene.shapes.append(pkg.sphere.create(pkg.Vec3f(*c), r, pkg.Reflectance(**m)))
    for pos, col, inten in SW.SMALL_LIGHTS:
        scene.lights.append(pkg.create_light(pkg.Vec3f(*pos), pkg.Vec3f(*col), inten))
    scene.camera = pkg.Vec3f(0., 0., 0.)
    return scene, (0.4, 12.)


def measure_ticks(pkg, name, reps, out):
    """Two contexts, RM_SWEPT_BVH read at rm_init: the flat one first, then the default."""
    scene, (aperture, focus) = tick_scene(pkg, name)
    velocities = SF.test_velocities(pkg, scene, 0.)                     # (every shape of both scenes but the 256 spheres' floor is a sphere)
    for k, shape in enumerate(scene.shapes):
        if not isinstance(shape, pkg.sphere.Sphere):
            velocities[k] = 0.
    os.environ["RM_SWEPT_BVH"] = "0"
    flat = pkg.backend.Context(0)
    del os.environ["RM_SWEPT_BVH"]
    swept = pkg.backend.Context(0)
    sides = (("flat", flat), ("swept", swept))
    try:
        for _, c in sides:
            c.upload(scene.flatten())
        # ---- the sides agree before either is timed (64 x 64, two ticks of 8), and say which walk they took
        small = pkg.backend.make_params(workloads.FOV, 64., 64., DEPTH)
        got = {}
        for side, c in sides:
            rgb = np.zeros((64, 64, 3))
            c.render_progressive_motion(small, velocities, SHUTTER, aperture, focus, 8, restart=True)
            c.render_progressive_motion(small, velocities, SHUTTER, aperture, focus, 8, host_rgb=rgb)
            got[side] = (rgb.tobytes(), c.swept_tick_info()["walked_swept"])
        assert got["flat"][0] == got["swept"][0] and (got["flat"][1], got["swept"][1]) == (0, 1), name
        n_spheres = sum(isinstance(shape, pkg.sphere.Sphere) for shape in scene.shapes)
        out.append("%s (%d shapes, %d spheres; aperture %g, focus %g):" % (name, len(scene.shapes), n_spheres, aperture, focus))
        p = pkg.backend.make_params(workloads.FOV, float(HEIGHT), float(WIDTH), DEPTH)
        verdict = []
        for tick in ("progressive", "converging"):
            for n in (8, 64):
                def run(c, restart):
                    if tick == "progressive":
                        return c.render_progressive_motion(p, velocities, SHUTTER, aperture, focus, n, restart=restart)[0].kernel_ms
                    return c.render_converging_motion(p, velocities, SHUTTER, aperture, focus, n, -1., n, 65536, restart=restart)[0].kernel_ms
                for k in range(WARM):
                    for _, c in sides:
                        run(c, k == 0)
                ms = {side: [] for side, _ in sides}
                for _ in range(reps):
                    for side, c in sides:
                        ms[side].append(run(c, False))
                assert swept.swept_tick_info()["walked_swept"] == 1 and flat.swept_tick_info()["walked_swept"] == 0
                summary(ms, out, "%s, %2d samples" % (tick, n), verdict)
        out.append("  swept not slower than flat by more than flat's own spread in %d of %d rows" % (sum(verdict), len(verdict)))
        out.append("")
    finally:
        flat.close()
        swept.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["pass", "converge", "ticks"], required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scenes", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    path = args.out or os.path.join(ROOT, "profiles", "raw", "camera_swept_%s.txt" % args.part)
    pkg = G.load_package()
    what = {"pass": "rm_accumulate_camera_device with a shape table (flat) against rm_accumulate_camera_swept_device",
            "converge": "rm_accumulate_converging_camera_device with a shape table (flat) against rm_accumulate_converging_camera_swept_device, every pixel listed",
            "ticks": "rm_render_progressive_motion and rm_render_converging_motion (every pixel listed) under RM_SWEPT_BVH=0 (flat) against the default (swept); the ticks' kernel_ms"}
    out = ["Swept hierarchies under a moving camera on %s (profiles/camera_swept_figures.py --part %s, %d launches a side, %d warm-up, interleaved)." % (
               torch.cuda.get_device_name(0), args.part, args.reps, WARM),
           "%s; %dx%d, depth %d, shutter %g; median (min .. max) in ms, HIP events." % (what[args.part], WIDTH, HEIGHT, DEPTH, SHUTTER), ""]
    scenes = args.scenes.split(",") if args.scenes else list(TICK_SCENES if args.part == "ticks" else SCENES)
    ctx = pkg.backend.Context(0) if args.part != "ticks" else None
    text = ""
    with tempfile.TemporaryDirectory() as tmp:
        for name in scenes:
            if args.part == "ticks":
                measure_ticks(pkg, name, args.reps, out)
            else:
                measure(pkg, ctx, name, args.part, args.reps, out, tmp)
            text = "\n".join(out) + "\n"
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:                                 # (after every scene: a step cut short keeps what it measured)
                fh.write(text)
    if ctx is not None:
        ctx.close()
    print(text)


if __name__ == "__main__":
    main()
