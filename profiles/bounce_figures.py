"""Diffuse bounce on one MI355X, one GPU step.

1. Pass time.  1920x1056, depth 5, the demo scene and the Cornell box, 8 and 64 samples a pass, a pinhole, point lights (offsets
   of zero).  One rm_accumulate_bounce_device pass with all three outputs (n_before > 0: the sum is read) -- once with strength 0,
   once with strength 1 -- against one rm_accumulate_soft_device pass over the same table rows and buffers; and one
   rm_accumulate_converging_bounce_device pass that lists every pixel (tolerance < 0), strength 0 and 1, against one
   rm_accumulate_converging_device pass.  HIP events around each launch on one stream, WARM warm-up launches of each, then REPS
   launches of each, interleaved (soft, zero, bounce, soft, ...): median, minimum and maximum.  The soft pass's own (max - min) /
   median is the launch-to-launch spread the ratios stand beside.  A strength-0 pass casts the member's rays exactly: its
   ratio is the price of the rule's registers and branches; a strength-1 pass casts up to one subtree more a sample.
2. A whole converged Cornell view, 640x352, depth 5, tolerance 0.01, 8 samples a tick, at most 256 a pixel: the samples and the
   time the converging bounce tick takes to finish against the plain bounce tick run to the cap.

Before anything is timed the sides are checked on 64x64: a strength-0 pass is the soft pass byte for byte, and a strength-1
pass is another picture.

Usage: python profiles/bounce_figures.py [--reps 20] [--out profiles/raw/bounce_figures.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402
import workloads  # noqa: E402

WARM = 3
APERTURE, FOCUS = 0., 5.
WIDTH, HEIGHT, DEPTH = 1920, 1056, 5
VIEW_W, VIEW_H, TOLERANCE, TICK, CAP = 640, 352, 0.01, 8, 256


def event_ms(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return statistics.median(ms), min(ms), max(ms)


def spread(ms):
    return (max(ms) - min(ms)) / statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw", "bounce_figures.json"))
    args = ap.parse_args()
    pkg = G.load_package()
    K = pkg.backend
    ctx = K.Context(0)
    s = torch.cuda.current_stream()
    f64, u8, i32, dev = torch.float64, torch.uint8, torch.int32, "cuda:0"
    rows_out = []
    for scene in ("demo", "cornell"):
        ctx.orient(None)
        ctx.upload(workloads.product_scene(pkg, scene).flatten())
        n_lights = ctx.n_lights()

        # ---- the sides agree before either is timed (64 x 64)
        small = K.make_params(workloads.FOV, 64., 64., DEPTH)
        t8, b8, z8 = ctx.lens_sequence(0, 8), K.bounce_sequence(0, 8), np.zeros((8, n_lights, 3))
        soft, zero, lit = (torch.full((64, 64, 3), float("nan"), dtype=f64, device=dev) for _ in range(3))
        ctx.accumulate_soft_device(small, soft, APERTURE, FOCUS, t8, z8, 0)
        ctx.accumulate_bounce_device(small, zero, APERTURE, FOCUS, t8, z8, b8, 0., 0)
        ctx.accumulate_bounce_device(small, lit, APERTURE, FOCUS, t8, z8, b8, 1., 0)
        torch.cuda.synchronize()
        assert soft.cpu().numpy().tobytes() == zero.cpu().numpy().tobytes(), "a strength-0 pass is not the soft pass"
        bounced = int(((lit - soft).abs() > 0.05 * 8).any(dim=2).sum())
        assert bounced > 0, "strength 1 changed no pixel"

        p = K.make_params(workloads.FOV, float(HEIGHT), float(WIDTH), DEPTH)
        total, mean = torch.zeros((HEIGHT, WIDTH, 3), dtype=f64, device=dev), torch.zeros((HEIGHT, WIDTH, 3), dtype=f64, device=dev)
        rgb8 = torch.zeros((HEIGHT, WIDTH, 3), dtype=u8, device=dev)
        stat, count = torch.zeros((HEIGHT, WIDTH, 2), dtype=f64, device=dev), torch.zeros((HEIGHT, WIDTH), dtype=i32, device=dev)
        ws = torch.zeros((ctx.converge_workspace(p) // 4,), dtype=i32, device=dev)
        for n in (8, 64):
            table = torch.from_numpy(ctx.lens_sequence(0, 2 * n)).to(dev)       # rows n .. 2n - 1: the second pass of a frame
            bounce = torch.from_numpy(K.bounce_sequence(0, 2 * n)).to(dev)
            zeros = torch.zeros((n, n_lights, 3), dtype=f64, device=dev)
            tn, bn = table[n:].contiguous(), bounce[n:].contiguous()

            def run_soft():
                ctx.accumulate_soft_device(p, total, APERTURE, FOCUS, tn, zeros, n, mean=mean, rgb8=rgb8)

            def run_bounce(strength):
                ctx.accumulate_bounce_device(p, total, APERTURE, FOCUS, tn, zeros, bn, strength, n, mean=mean, rgb8=rgb8)

            def run_converge():
                count.fill_(n)                                                # every pixel holds the first pass: the second is timed
                return lambda: ctx.accumulate_converging_device(p, total, stat, count, APERTURE, FOCUS, n, table, -1., 0, 2 * n, False,
                                                                mean=mean, rgb8=rgb8, workspace=ws)

            def run_converge_bounce(strength):
                count.fill_(n)
                return lambda: ctx.accumulate_converging_bounce_device(p, total, stat, count, APERTURE, FOCUS, n, table, bounce, strength, -1., 0,
                                                                       2 * n, False, mean=mean, rgb8=rgb8, workspace=ws)

            sides = {"soft": lambda: run_soft, "bounce0": lambda: (lambda: run_bounce(0.)), "bounce1": lambda: (lambda: run_bounce(1.)),
                     "converge": run_converge, "converge_bounce0": lambda: run_converge_bounce(0.), "converge_bounce1": lambda: run_converge_bounce(1.)}
            for _ in range(WARM):
                for make in sides.values():
                    make()()
            torch.cuda.synchronize()
            ms = {k: [] for k in sides}
            for _ in range(args.reps):
                for k, make in sides.items():
                    fn = make()                                               # (the count's reset is outside the events)
                    torch.cuda.synchronize()
                    ms[k].append(event_ms(fn, s))
            med = {k: statistics.median(v) for k, v in ms.items()}
            row = {"what": "bounce_pass", "scene": scene, "width": WIDTH, "height": HEIGHT, "max_depth": DEPTH, "n_samples": n,
                   **{k + "_ms": stats(v) for k, v in ms.items()},
                   "bounce0_over_soft": med["bounce0"] / med["soft"], "bounce1_over_soft": med["bounce1"] / med["soft"],
                   "converge_bounce0_over_converge": med["converge_bounce0"] / med["converge"],
                   "converge_bounce1_over_converge": med["converge_bounce1"] / med["converge"],
                   "soft_spread": spread(ms["soft"]), "converge_spread": spread(ms["converge"]), "bounced_pixels_64x64": bounced}
            print(json.dumps(row), flush=True)
            rows_out.append(row)

    # ---- a whole converged Cornell view against the plain bounce frame ticked to the cap (the Cornell box is resident)
    v = K.make_params(workloads.FOV, float(VIEW_H), float(VIEW_W), DEPTH)
    t0, kernel, ticks, rep = time.perf_counter(), 0., 0, None
    while rep is None or rep.listed > 0:
        timing, rep = ctx.render_converging_bounce(v, APERTURE, FOCUS, TICK, TOLERANCE, 16, CAP, 1., restart=rep is None)
        kernel, ticks = kernel + timing.kernel_ms, ticks + 1
    converged = {"ticks": ticks, "samples_cast": int(rep.samples_cast), "kernel_ms": kernel, "wall_ms": (time.perf_counter() - t0) * 1e3}
    t0, kernel, total_n = time.perf_counter(), 0., 0
    while total_n < CAP:
        timing, total_n = ctx.render_progressive_bounce(v, APERTURE, FOCUS, TICK, 1., restart=total_n == 0)
        kernel += timing.kernel_ms
    plain = {"ticks": CAP // TICK, "samples_cast": CAP * VIEW_W * VIEW_H, "kernel_ms": kernel, "wall_ms": (time.perf_counter() - t0) * 1e3}
    row = {"what": "converged_view", "scene": "cornell", "width": VIEW_W, "height": VIEW_H, "max_depth": DEPTH, "tolerance": TOLERANCE,
           "n_samples": TICK, "max_samples": CAP, "converging": converged, "plain_to_the_cap": plain,
           "samples_ratio": converged["samples_cast"] / plain["samples_cast"], "kernel_ratio": converged["kernel_ms"] / plain["kernel_ms"]}
    print(json.dumps(row), flush=True)
    rows_out.append(row)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "warm": WARM, "rows": rows_out}, fh, indent=1)


if __name__ == "__main__":
    main()
