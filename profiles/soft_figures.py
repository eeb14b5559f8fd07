"""Area lights on one MI355X, one GPU step.

Kernel against the progressive frames' kernel of the same build.  1920x1056, depth 5, the demo scene, 8 and 64 samples a
pass: one rm_accumulate_soft_device pass with all three outputs (n_before > 0: the sum is read) -- once with an offset table of
zeros, once with the rows of rm_light_sequence for radii of 1.5 -- against one rm_accumulate_lens_device pass over the same
table rows and buffers.  HIP events around each launch on one stream, WARM warm-up launches of each, then REPS launches of
each, interleaved (plain, zero, soft, plain, ...): median, minimum and maximum.  The zero-offset pass casts the plain pass's
rays and shadow rays exactly, so its ratio is the price of the hook itself (three loads and three additions a light and ray
step); with radii the shadow rays are others, and the ratio is that plus whatever the moved lights do to the walks.

Before anything is timed the sides are checked on 64x64: a zero-offset pass is the plain pass byte for byte, and a pass with
radii is another picture.

Usage: python profiles/soft_figures.py [--reps 20] [--out profiles/raw/soft_figures.json]
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
RADIUS = 1.5


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw", "soft_figures.json"))
    args = ap.parse_args()
    pkg = G.load_package()
    ctx = pkg.backend.Context(0)
    s = torch.cuda.current_stream()
    f64, u8, dev = torch.float64, torch.uint8, "cuda:0"
    ctx.orient(None)
    ctx.upload(workloads.product_scene(pkg, "demo").flatten())
    n_lights = ctx.n_lights()
    radii = (RADIUS,) * n_lights

    # ---- the sides agree before either is timed (64 x 64)
    small = pkg.backend.make_params(workloads.FOV, 64., 64., DEPTH)
    t8 = torch.from_numpy(ctx.lens_sequence(0, 8)).to(dev)
    plain, zero, soft = (torch.full((64, 64, 3), float("nan"), dtype=f64, device=dev) for _ in range(3))
    ctx.accumulate_lens_device(small, plain, APERTURE, FOCUS, t8, 0)
    ctx.accumulate_soft_device(small, zero, APERTURE, FOCUS, t8, np.zeros((8, n_lights, 3)), 0)
    ctx.accumulate_soft_device(small, soft, APERTURE, FOCUS, t8, ctx.light_sequence(0, 8, radii), 0)
    torch.cuda.synchronize()
    assert plain.cpu().numpy().tobytes() == zero.cpu().numpy().tobytes(), "a zero-offset pass is not the plain pass"
    moved = int(((soft - plain).abs() > 0.05 * 8).any(dim=2).sum())
    assert moved > 0, "radii of %g moved no shadow" % RADIUS

    p = pkg.backend.make_params(workloads.FOV, float(HEIGHT), float(WIDTH), DEPTH)
    total = torch.zeros((HEIGHT, WIDTH, 3), dtype=f64, device=dev)
    mean = torch.zeros((HEIGHT, WIDTH, 3), dtype=f64, device=dev)
    rgb8 = torch.zeros((HEIGHT, WIDTH, 3), dtype=u8, device=dev)
    rows_out = []
    for n in (8, 64):
        table = torch.from_numpy(ctx.lens_sequence(n, n)).to(dev)           # rows n .. 2n - 1: the second pass of a frame
        zeros = torch.zeros((n, n_lights, 3), dtype=f64, device=dev)
        offsets = torch.from_numpy(ctx.light_sequence(n, n, radii)).to(dev)

        def run_plain():
            ctx.accumulate_lens_device(p, total, APERTURE, FOCUS, table, n, mean=mean, rgb8=rgb8)

        def run_zero():
            ctx.accumulate_soft_device(p, total, APERTURE, FOCUS, table, zeros, n, mean=mean, rgb8=rgb8)

        def run_soft():
            ctx.accumulate_soft_device(p, total, APERTURE, FOCUS, table, offsets, n, mean=mean, rgb8=rgb8)

        for _ in range(WARM):
            run_plain()
            run_zero()
            run_soft()
        torch.cuda.synchronize()
        plain_ms, zero_ms, soft_ms = [], [], []
        for _ in range(args.reps):
            plain_ms.append(event_ms(run_plain, s))
            zero_ms.append(event_ms(run_zero, s))
            soft_ms.append(event_ms(run_soft, s))
        row = {"what": "soft_vs_plain_pass", "scene": "demo", "width": WIDTH, "height": HEIGHT, "max_depth": DEPTH, "n_samples": n,
               "radius": RADIUS, "plain_ms": stats(plain_ms), "zero_offsets_ms": stats(zero_ms), "radii_ms": stats(soft_ms),
               "zero_over_plain": stats(zero_ms)[0] / stats(plain_ms)[0], "radii_over_plain": stats(soft_ms)[0] / stats(plain_ms)[0],
               "moved_pixels_64x64": moved}
        print(json.dumps(row), flush=True)
        rows_out.append(row)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "warm": WARM, "rows": rows_out}, fh, indent=1)


if __name__ == "__main__":
    main()
