"""Moving shapes on one MI355X, one GPU step.

Kernel against the moving spheres' kernel of the same build (its code is the parent's, instruction for instruction:
profiles/moving_resource_usage.txt).  1920x1056, depth 5, the demo scene and the Cornell box, 8 and 64 samples a pass: one
rm_accumulate_moving_device pass with all three outputs (n_before > 0: the sum is read) -- once with a shape offset table of
zeros, once with the rows of rm_motion_sequence for the test velocities (spheres: (2 cos(2 pi g k), 2 sin(2 pi g k), 0.5); other
shapes: speed x (cos(2 pi g k + 1), 0.5 sin(2 pi g k + 1), 0.25), speed 6 in the demo and 150 in the Cornell box; g =
0.6180339887498949, shutter 1) -- against one rm_accumulate_motion_device pass over the same table rows, light offsets (zeros:
point lights), zero shape offsets and buffers.  HIP events around each launch on one stream, WARM warm-up launches of each,
then REPS launches of each, interleaved (motion, zero, moving, motion, ...): median, minimum and maximum.  The zero-offset pass
casts the motion pass's rays and shadow rays exactly, so its ratio is the price of the rule itself -- a map word, three loads a
shape and walk, one addition at each use of a coordinate -- to be judged against the motion pass's own spread between
launches; with velocities the rays meet other things, and the ratio is that plus whatever the moved shapes do to the walks.

Before anything is timed the sides are checked on 64x64: a zero-offset pass is the motion pass byte for byte, and a pass with
velocities is another picture.

Usage: python profiles/moving_figures.py [--reps 20] [--out profiles/raw/moving_figures.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402
import workloads  # noqa: E402

WARM = 3
WIDTH, HEIGHT, DEPTH = 1920, 1056, 5
GOLDEN, SHUTTER = 0.6180339887498949, 1.
SCENES = {"demo": (0.4, 5., 6.), "cornell": (12., 500., 150.)}       # aperture, focus, speed of what is not a sphere


def event_ms(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw", "moving_figures.json"))
    args = ap.parse_args()
    pkg = G.load_package()
    ctx = pkg.backend.Context(0)
    s = torch.cuda.current_stream()
    f64, u8, dev = torch.float64, torch.uint8, "cuda:0"
    rows_out = []
    for name, (aperture, focus, speed) in SCENES.items():
        scene = workloads.product_scene(pkg, name)
        ctx.orient(None)
        ctx.upload(scene.flatten())
        n_lights, n_shapes = ctx.n_lights(), len(scene.shapes)
        velocities = np.zeros((n_shapes, 3))
        for k, shape in enumerate(scene.shapes):
            if isinstance(shape, pkg.sphere.Sphere):
                velocities[k] = (2. * np.cos(2. * np.pi * GOLDEN * k), 2. * np.sin(2. * np.pi * GOLDEN * k), 0.5)
            else:
                a = 2. * np.pi * GOLDEN * k + 1.
                velocities[k] = (speed * np.cos(a), speed * 0.5 * np.sin(a), speed * 0.25)

        # ---- the sides agree before either is timed (64 x 64)
        small = pkg.backend.make_params(workloads.FOV, 64., 64., DEPTH)
        t8 = torch.from_numpy(ctx.lens_sequence(0, 8)).to(dev)
        l8, z8 = np.zeros((8, n_lights, 3)), np.zeros((8, n_shapes, 3))
        motion, zero, moving = (torch.full((64, 64, 3), float("nan"), dtype=f64, device=dev) for _ in range(3))
        ctx.accumulate_motion_device(small, motion, aperture, focus, t8, l8, z8, 0)
        ctx.accumulate_moving_device(small, zero, aperture, focus, t8, l8, z8, 0)
        ctx.accumulate_moving_device(small, moving, aperture, focus, t8, l8, ctx.motion_sequence(0, 8, velocities, SHUTTER), 0)
        torch.cuda.synchronize()
        assert motion.cpu().numpy().tobytes() == zero.cpu().numpy().tobytes(), "a zero-offset pass is not the motion pass"
        moved = int(((moving - motion).abs() > 0.05 * 8).any(dim=2).sum())
        assert moved > 0, "the velocities moved nothing"

        p = pkg.backend.make_params(workloads.FOV, float(HEIGHT), float(WIDTH), DEPTH)
        total = torch.zeros((HEIGHT, WIDTH, 3), dtype=f64, device=dev)
        mean = torch.zeros((HEIGHT, WIDTH, 3), dtype=f64, device=dev)
        rgb8 = torch.zeros((HEIGHT, WIDTH, 3), dtype=u8, device=dev)
        for n in (8, 64):
            table = torch.from_numpy(ctx.lens_sequence(n, n)).to(dev)           # rows n .. 2n - 1: the second pass of a frame
            lights = torch.zeros((n, n_lights, 3), dtype=f64, device=dev)
            zeros = torch.zeros((n, n_shapes, 3), dtype=f64, device=dev)
            offsets = torch.from_numpy(ctx.motion_sequence(n, n, velocities, SHUTTER)).to(dev)

            def run_motion():
                ctx.accumulate_motion_device(p, total, aperture, focus, table, lights, zeros, n, mean=mean, rgb8=rgb8)

            def run_zero():
                ctx.accumulate_moving_device(p, total, aperture, focus, table, lights, zeros, n, mean=mean, rgb8=rgb8)

            def run_moving():
                ctx.accumulate_moving_device(p, total, aperture, focus, table, lights, offsets, n, mean=mean, rgb8=rgb8)

            for _ in range(WARM):
                run_motion()
                run_zero()
                run_moving()
            torch.cuda.synchronize()
            motion_ms, zero_ms, moving_ms = [], [], []
            for _ in range(args.reps):
                motion_ms.append(event_ms(run_motion, s))
                zero_ms.append(event_ms(run_zero, s))
                moving_ms.append(event_ms(run_moving, s))
            row = {"what": "moving_vs_motion_pass", "scene": name, "width": WIDTH, "height": HEIGHT, "max_depth": DEPTH, "n_samples": n,
                   "shapes": n_shapes, "shutter": SHUTTER, "motion_zero_ms": stats(motion_ms), "moving_zero_ms": stats(zero_ms),
                   "moving_velocities_ms": stats(moving_ms), "zero_over_motion": stats(zero_ms)[0] / stats(motion_ms)[0],
                   "velocities_over_motion": stats(moving_ms)[0] / stats(motion_ms)[0], "moved_pixels_64x64": moved}
            print(json.dumps(row), flush=True)
            rows_out.append(row)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "warm": WARM, "rows": rows_out}, fh, indent=1)


if __name__ == "__main__":
    main()
