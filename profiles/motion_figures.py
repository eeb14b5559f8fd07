"""Moving spheres on one MI355X, one GPU step.

Kernel against the area lights' kernel of the same build (its code is the parent's, instruction for instruction:
profiles/motion_resource_usage.txt).  1920x1056, depth 5, the demo scene, 8 and 64 samples a pass: one
rm_accumulate_motion_device pass with all three outputs (n_before > 0: the sum is read) -- once with a shape offset table of
zeros, once with the rows of rm_motion_sequence for the test velocities (sphere shape k: (2 cos(2 pi g k), 2 sin(2 pi g k), 0.5),
g = 0.6180339887498949, shutter 1) -- against one rm_accumulate_soft_device pass over the same table rows, light offsets (zeros:
point lights) and buffers.  HIP events around each launch on one stream, WARM warm-up launches of each, then REPS launches of
each, interleaved (soft, zero, motion, soft, ...): median, minimum and maximum.  The zero-velocity pass casts the soft pass's rays
and shadow rays exactly, so its ratio is the price of the rule itself: the soft pass reads its sphere centres through scalar
operands, the motion pass forms them per lane (a map word, three loads and three additions a sphere and walk); with velocities
the rays meet other things, and the ratio is that plus whatever the moved spheres do to the walks.

Before anything is timed the sides are checked on 64x64: a zero-offset pass is the soft pass byte for byte, and a pass with
velocities is another picture.

Usage: python profiles/motion_figures.py [--reps 20] [--out profiles/raw/motion_figures.json]
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

WARM = 5
APERTURE, FOCUS = 0.4, 5.
WIDTH, HEIGHT, DEPTH = 1920, 1056, 5
GOLDEN, SHUTTER = 0.6180339887498949, 1.


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw", "motion_figures.json"))
    args = ap.parse_args()
    pkg = G.load_package()
    ctx = pkg.backend.Context(0)
    s = torch.cuda.current_stream()
    f64, u8, dev = torch.float64, torch.uint8, "cuda:0"
    scene = workloads.product_scene(pkg, "demo")
    ctx.orient(None)
    ctx.upload(scene.flatten())
    n_lights, n_shapes = ctx.n_lights(), len(scene.shapes)
    velocities = np.zeros((n_shapes, 3))
    for k, shape in enumerate(scene.shapes):
        if isinstance(shape, pkg.sphere.Sphere):
            velocities[k] = (2. * np.cos(2. * np.pi * GOLDEN * k), 2. * np.sin(2. * np.pi * GOLDEN * k), 0.5)
    n_spheres = int((velocities != 0.).any(axis=1).sum())

    # ---- the sides agree before either is timed (64 x 64)
    small = pkg.backend.make_params(workloads.FOV, 64., 64., DEPTH)
    t8 = torch.from_numpy(ctx.lens_sequence(0, 8)).to(dev)
    l8 = np.zeros((8, n_lights, 3))
    soft, zero, motion = (torch.full((64, 64, 3), float("nan"), dtype=f64, device=dev) for _ in range(3))
    ctx.accumulate_soft_device(small, soft, APERTURE, FOCUS, t8, l8, 0)
    ctx.accumulate_motion_device(small, zero, APERTURE, FOCUS, t8, l8, np.zeros((8, n_shapes, 3)), 0)
    ctx.accumulate_motion_device(small, motion, APERTURE, FOCUS, t8, l8, ctx.motion_sequence(0, 8, velocities, SHUTTER), 0)
    torch.cuda.synchronize()
    assert soft.cpu().numpy().tobytes() == zero.cpu().numpy().tobytes(), "a zero-offset pass is not the soft pass"
    moved = int(((motion - soft).abs() > 0.05 * 8).any(dim=2).sum())
    assert moved > 0, "the velocities moved nothing"

    p = pkg.backend.make_params(workloads.FOV, float(HEIGHT), float(WIDTH), DEPTH)
    total = torch.zeros((HEIGHT, WIDTH, 3), dtype=f64, device=dev)
    mean = torch.zeros((HEIGHT, WIDTH, 3), dtype=f64, device=dev)
    rgb8 = torch.zeros((HEIGHT, WIDTH, 3), dtype=u8, device=dev)
    rows_out = []
    for n in (8, 64):
        table = torch.from_numpy(ctx.lens_sequence(n, n)).to(dev)           # rows n .. 2n - 1: the second pass of a frame
        lights = torch.zeros((n, n_lights, 3), dtype=f64, device=dev)
        zeros = torch.zeros((n, n_shapes, 3), dtype=f64, device=dev)
        offsets = torch.from_numpy(ctx.motion_sequence(n, n, velocities, SHUTTER)).to(dev)

        def run_soft():
            ctx.accumulate_soft_device(p, total, APERTURE, FOCUS, table, lights, n, mean=mean, rgb8=rgb8)

        def run_zero():
            ctx.accumulate_motion_device(p, total, APERTURE, FOCUS, table, lights, zeros, n, mean=mean, rgb8=rgb8)

        def run_motion():
            ctx.accumulate_motion_device(p, total, APERTURE, FOCUS, table, lights, offsets, n, mean=mean, rgb8=rgb8)

        for _ in range(WARM):
            run_soft()
            run_zero()
            run_motion()
        torch.cuda.synchronize()
        soft_ms, zero_ms, motion_ms = [], [], []
        for _ in range(args.reps):
            soft_ms.append(event_ms(run_soft, s))
            zero_ms.append(event_ms(run_zero, s))
            motion_ms.append(event_ms(run_motion, s))
        row = {"what": "motion_vs_soft_pass", "scene": "demo", "width": WIDTH, "height": HEIGHT, "max_depth": DEPTH, "n_samples": n,
               "moving_spheres": n_spheres, "shutter": SHUTTER, "soft_ms": stats(soft_ms), "zero_velocities_ms": stats(zero_ms),
               "velocities_ms": stats(motion_ms), "zero_over_soft": stats(zero_ms)[0] / stats(soft_ms)[0],
               "velocities_over_soft": stats(motion_ms)[0] / stats(soft_ms)[0], "moved_pixels_64x64": moved}
        print(json.dumps(row), flush=True)
        rows_out.append(row)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "warm": WARM, "rows": rows_out}, fh, indent=1)


if __name__ == "__main__":
    main()
