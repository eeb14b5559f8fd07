"""Converging frames on one MI355X, one GPU step.

1. The price of the machinery.  1920x1056, depth 5, the demo scene, aperture 0.4, 8 and 64 samples a pass: one
   rm_accumulate_converging_device pass with tolerance < 0 (every pixel listed) and all outputs, every count = n_samples -- so it
   casts rows n .. 2n - 1 for every pixel -- against one rm_accumulate_lens_device pass over the same rows with n_before =
   n_samples; and a pass whose cap leaves every pixel capped (the memset, the select launch and a shade launch that finds an empty
   list).  HIP events around each on one stream, WARM warm-up launches of each, then REPS of each, interleaved: median, minimum and
   maximum.  The counts are set back before every converging pass, outside the events.
2. The gain.  The same view ticked to the end by rm_render_converging (tolerance 0.01, min_samples 16, max_samples 1024, 8 samples
   a tick), with point lights and with radii of 1.5: per tick the listed pixels and kernel_ms, in total the milliseconds and the
   samples cast, against rm_render_progressive (rm_render_progressive_soft) ticked to 1024 samples a pixel.

Before anything is timed the sides are checked on 64x64: with tolerance < 0 a fresh and a continued converging pass are the plain
passes byte for byte.

Usage: python profiles/converge_figures.py [--reps 20] [--out profiles/raw/converge_figures.json]
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
TOLERANCE, MIN_SAMPLES, MAX_SAMPLES, TICK = 0.01, 16, 1024, 8


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw", "converge_figures.json"))
    args = ap.parse_args()
    pkg = G.load_package()
    ctx = pkg.backend.Context(0)
    s = torch.cuda.current_stream()
    f64, u8, i32, dev = torch.float64, torch.uint8, torch.int32, "cuda:0"
    ctx.orient(None)
    ctx.upload(workloads.product_scene(pkg, "demo").flatten())
    radii = (RADIUS,) * ctx.n_lights()

    # ---- the sides agree before either is timed (64 x 64)
    small = pkg.backend.make_params(workloads.FOV, 64., 64., DEPTH)
    t16 = torch.from_numpy(ctx.lens_sequence(0, 16)).to(dev)
    plain, conv = (torch.full((64, 64, 3), float("nan"), dtype=f64, device=dev) for _ in range(2))
    st, cnt = torch.zeros((64, 64, 2), dtype=f64, device=dev), torch.zeros((64, 64), dtype=i32, device=dev)
    for k in range(2):
        ctx.accumulate_lens_device(small, plain, APERTURE, FOCUS, t16[8 * k:8 * k + 8].contiguous(), 8 * k)
        ctx.accumulate_converging_device(small, conv, st, cnt, APERTURE, FOCUS, 8, t16, -1., 0, 16, k == 0)
        torch.cuda.synchronize()
        assert plain.cpu().numpy().tobytes() == conv.cpu().numpy().tobytes(), "pass %d with tolerance < 0 is not the plain pass" % (k + 1)
    assert bool((cnt == 16).all())

    p = pkg.backend.make_params(workloads.FOV, float(HEIGHT), float(WIDTH), DEPTH)
    total = torch.zeros((HEIGHT, WIDTH, 3), dtype=f64, device=dev)
    mean = torch.zeros((HEIGHT, WIDTH, 3), dtype=f64, device=dev)
    rgb8 = torch.zeros((HEIGHT, WIDTH, 3), dtype=u8, device=dev)
    stat = torch.zeros((HEIGHT, WIDTH, 2), dtype=f64, device=dev)
    count = torch.zeros((HEIGHT, WIDTH), dtype=i32, device=dev)
    mask = torch.zeros((HEIGHT, WIDTH), dtype=u8, device=dev)
    ws = torch.zeros((ctx.converge_workspace(p) // 4,), dtype=i32, device=dev)
    rows_out = []
    for n in (8, 64):
        whole = torch.from_numpy(ctx.lens_sequence(0, 2 * n)).to(dev)         # rows 0 .. 2n - 1; the passes cast n .. 2n - 1
        table = whole[n:].contiguous()

        def run_plain():
            ctx.accumulate_lens_device(p, total, APERTURE, FOCUS, table, n, mean=mean, rgb8=rgb8)

        def run_conv():
            ctx.accumulate_converging_device(p, total, stat, count, APERTURE, FOCUS, n, whole, -1., 0, 2 * n, False, mean=mean, rgb8=rgb8,
                                             mask=mask, workspace=ws)

        def run_capped():                                                  # n + n > 2 n - 1: every pixel capped, nothing listed
            ctx.accumulate_converging_device(p, total, stat, count, APERTURE, FOCUS, n, whole, -1., 0, 2 * n - 1, False, mean=mean, rgb8=rgb8,
                                             mask=mask, workspace=ws)

        def timed(fn):
            count.fill_(n)
            return event_ms(fn, s)

        for _ in range(WARM):
            timed(run_plain), timed(run_conv), timed(run_capped)
        torch.cuda.synchronize()
        assert int(ws[0]) == 0 and bool((count == n).all())                # (the capped pass ran last)
        plain_ms, conv_ms, capped_ms = [], [], []
        for _ in range(args.reps):
            plain_ms.append(timed(run_plain))
            conv_ms.append(timed(run_conv))
            assert int(ws[0]) == HEIGHT * WIDTH
            capped_ms.append(timed(run_capped))
        row = {"what": "converging_vs_plain_pass", "scene": "demo", "width": WIDTH, "height": HEIGHT, "max_depth": DEPTH, "n_samples": n,
               "plain_ms": stats(plain_ms), "converging_ms": stats(conv_ms), "capped_ms": stats(capped_ms),
               "converging_over_plain": stats(conv_ms)[0] / stats(plain_ms)[0], "plain_max_over_min": max(plain_ms) / min(plain_ms)}
        print(json.dumps(row), flush=True)
        rows_out.append(row)
    del total, mean, rgb8, stat, count, mask, ws

    # ---- the gain: the view ticked to the end
    for what, r in (("point lights", None), ("radii %g" % RADIUS, radii)):
        ticks, ms = [], 0.
        while True:
            timing, rep = ctx.render_converging(p, APERTURE, FOCUS, TICK, TOLERANCE, MIN_SAMPLES, MAX_SAMPLES, radii=r, restart=not ticks)
            if rep.listed == 0 and timing.kernel_ms == 0.:
                break
            ticks.append((rep.listed, timing.kernel_ms))
            ms += timing.kernel_ms
            assert len(ticks) <= 8 * (MAX_SAMPLES // TICK)                  # (a safety stop; a late neighbour can outlast max_samples / n_samples ticks)
        plain_ms, total_n = 0., 0
        while total_n < MAX_SAMPLES:
            if r is None:
                timing, total_n = ctx.render_progressive(p, APERTURE, FOCUS, TICK, restart=(total_n == 0))
            else:
                timing, total_n = ctx.render_progressive_soft(p, r, APERTURE, FOCUS, TICK, restart=(total_n == 0))
            plain_ms += timing.kernel_ms
        row = {"what": "converging_frame", "lights": what, "scene": "demo", "width": WIDTH, "height": HEIGHT, "max_depth": DEPTH,
               "tolerance": TOLERANCE, "min_samples": MIN_SAMPLES, "max_samples": MAX_SAMPLES, "n_samples": TICK,
               "ticks": len(ticks), "listed": [t[0] for t in ticks], "kernel_ms": [round(t[1], 4) for t in ticks],
               "total_ms": ms, "samples_cast": rep.samples_cast, "max_count": rep.max_count,
               "plain_ticks": MAX_SAMPLES // TICK, "plain_total_ms": plain_ms, "plain_samples": HEIGHT * WIDTH * MAX_SAMPLES}
        print(json.dumps(row), flush=True)
        rows_out.append(row)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "warm": WARM, "rows": rows_out}, fh, indent=1)


if __name__ == "__main__":
    main()
