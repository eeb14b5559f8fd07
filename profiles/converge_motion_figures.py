"""Converging frames with moving spheres on one MI355X, one GPU step.  Writes
profiles/converge_motion_figures.txt.

1. A pass that lists every pixel.  1920x1056, depth 5, the demo scene, 8 and 64 samples a pass, tolerance < 0, every count n_samples
   beforehand (so the sum and the stats are read and every pixel casts rows n_samples .. 2 n_samples - 1): one
   rm_accumulate_converging_device pass with light offsets of zero against one rm_accumulate_converging_motion_device pass over
   the same rows and buffers -- once with a shape offset table of zeros, once with the rows of rm_motion_sequence for the test
   velocities (sphere shape k: (2 cos(2 pi g k), 2 sin(2 pi g k), 0.5), g = 0.6180339887498949, shutter 1).  HIP events around the
   three steps of a pass (the memset, the select launch, the shade launch) on one stream; the counts are put back before the first
   event.  WARM warm-up passes of each, then REPS of each, interleaved (still, zero, motion, still, ...): median, minimum, maximum.
   The zero-velocity pass casts the still pass's rays exactly, so its ratio is the price of the rule itself; section 6n's ratios
   for the plain pass (rm_accumulate_motion_device over rm_accumulate_soft_device) are measured beside it in the same way.
2. The headline.  The same view at tolerance 0.01, min_samples 16, at most 1,024 samples, in ticks of 8 with the test velocities
   through rm_render_converging_motion until a tick lists nothing: ticks, the sum of the ticks' kernel_ms (HIP events inside the
   library) and samples cast -- against rm_render_progressive_motion ticked to 1,024 samples a pixel, and against
   rm_render_converging of the still scene.

Before anything is timed the sides are checked on 64x64: a zero-offset pass is the still pass byte for byte, and a pass with
velocities is another picture.

Usage: python profiles/converge_motion_figures.py [--reps 20] [--out profiles/converge_motion_figures.txt]
"""
import argparse
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
TOLERANCE, MIN_SAMPLES, MAX_SAMPLES, TICK = 0.01, 16, 1024, 8


def event_ms(before, fn, stream):
    before()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return statistics.median(ms), min(ms), max(ms)


def fmt(ms):
    return "median %8.3f ms (min %8.3f, max %8.3f)" % stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "converge_motion_figures.txt"))
    args = ap.parse_args()
    pkg = G.load_package()
    ctx = pkg.backend.Context(0)
    s = torch.cuda.current_stream()
    f64, u8, i32, dev = torch.float64, torch.uint8, torch.int32, "cuda:0"
    scene = workloads.product_scene(pkg, "demo")
    ctx.orient(None)
    ctx.upload(scene.flatten())
    n_lights, n_shapes = ctx.n_lights(), len(scene.shapes)
    velocities = np.zeros((n_shapes, 3))
    for k, shape in enumerate(scene.shapes):
        if isinstance(shape, pkg.sphere.Sphere):
            velocities[k] = (2. * np.cos(2. * np.pi * GOLDEN * k), 2. * np.sin(2. * np.pi * GOLDEN * k), 0.5)
    n_spheres = int((velocities != 0.).any(axis=1).sum())
    out = ["Converging frames with moving spheres on %s (profiles/converge_motion_figures.py, %d launches a side, %d warm-up)."
           % (torch.cuda.get_device_name(0), args.reps, WARM),
           "Demo scene, %d of its %d shapes are spheres and move; %dx%d, depth %d, aperture %g, focus %g, shutter %g." % (
               n_spheres, n_shapes, WIDTH, HEIGHT, DEPTH, APERTURE, FOCUS, SHUTTER), ""]

    def buffers(h, w, fill=0.):
        return dict(sum=torch.full((h, w, 3), fill, dtype=f64, device=dev), stats=torch.full((h, w, 2), fill, dtype=f64, device=dev),
                    count=torch.zeros((h, w), dtype=i32, device=dev), mean=torch.full((h, w, 3), fill, dtype=f64, device=dev),
                    rgb8=torch.zeros((h, w, 3), dtype=u8, device=dev))

    def tables(n_rows):
        return (torch.from_numpy(ctx.lens_sequence(0, n_rows)).to(dev), torch.zeros((n_rows, n_lights, 3), dtype=f64, device=dev),
                torch.zeros((n_rows, n_shapes, 3), dtype=f64, device=dev),
                torch.from_numpy(ctx.motion_sequence(0, n_rows, velocities, SHUTTER)).to(dev))

    # ---- the sides agree before either is timed (64 x 64, two passes of 8)
    small = pkg.backend.make_params(workloads.FOV, 64., 64., DEPTH)
    table, lights, zeros, offsets = tables(16)
    still, zero, motion = buffers(64, 64, float("nan")), buffers(64, 64, float("nan")), buffers(64, 64, float("nan"))
    for fresh in (True, False):
        ctx.accumulate_converging_device(small, still["sum"], still["stats"], still["count"], APERTURE, FOCUS, 8, table, -1., 0, 16, fresh,
                                         offsets=lights, mean=still["mean"], rgb8=still["rgb8"])
        for b, shapes in ((zero, zeros), (motion, offsets)):
            ctx.accumulate_converging_motion_device(small, b["sum"], b["stats"], b["count"], APERTURE, FOCUS, 8, table, lights, shapes, -1., 0, 16,
                                                    fresh, mean=b["mean"], rgb8=b["rgb8"])
    torch.cuda.synchronize()
    for key in still:
        assert still[key].cpu().numpy().tobytes() == zero[key].cpu().numpy().tobytes(), "a zero-offset pass is not the still pass: %s" % key
    moved = int(((motion["mean"] - still["mean"]).abs() > 0.05).any(dim=2).sum())
    assert moved > 0 and int(motion["count"].min()) == 16, "the velocities moved nothing"

    # ---- 1. a pass that lists every pixel
    p = pkg.backend.make_params(workloads.FOV, float(HEIGHT), float(WIDTH), DEPTH)
    b = buffers(HEIGHT, WIDTH)
    ws = torch.empty((ctx.converge_workspace(p) // 4,), dtype=i32, device=dev)
    out.append("1. A pass that lists every pixel (tolerance < 0, every count n_samples beforehand): memset + select + shade, HIP events.")
    for n in (8, 64):
        table, lights, zeros, offsets = tables(2 * n)

        def reset():
            b["count"].fill_(n)

        def run_still():
            ctx.accumulate_converging_device(p, b["sum"], b["stats"], b["count"], APERTURE, FOCUS, n, table, -1., 0, 2 * n, False, offsets=lights,
                                             mean=b["mean"], rgb8=b["rgb8"], workspace=ws)

        def run_zero():
            ctx.accumulate_converging_motion_device(p, b["sum"], b["stats"], b["count"], APERTURE, FOCUS, n, table, lights, zeros, -1., 0, 2 * n, False,
                                                    mean=b["mean"], rgb8=b["rgb8"], workspace=ws)

        def run_motion():
            ctx.accumulate_converging_motion_device(p, b["sum"], b["stats"], b["count"], APERTURE, FOCUS, n, table, lights, offsets, -1., 0, 2 * n,
                                                    False, mean=b["mean"], rgb8=b["rgb8"], workspace=ws)

        def run_soft():
            ctx.accumulate_soft_device(p, b["sum"], APERTURE, FOCUS, table[n:], lights[n:], n, mean=b["mean"], rgb8=b["rgb8"])

        def run_plain_zero():
            ctx.accumulate_motion_device(p, b["sum"], APERTURE, FOCUS, table[n:], lights[n:], zeros[n:], n, mean=b["mean"], rgb8=b["rgb8"])

        def run_plain_motion():
            ctx.accumulate_motion_device(p, b["sum"], APERTURE, FOCUS, table[n:], lights[n:], offsets[n:], n, mean=b["mean"], rgb8=b["rgb8"])

        sides = (("converging, still", run_still), ("converging, zero velocities", run_zero), ("converging, velocities", run_motion),
                 ("plain soft pass", run_soft), ("plain motion pass, zero velocities", run_plain_zero),
                 ("plain motion pass, velocities", run_plain_motion))
        for _ in range(WARM):
            for _, fn in sides:
                reset()
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in sides}
        for _ in range(args.reps):
            for name, fn in sides:
                ms[name].append(event_ms(reset, fn, s))
        assert int(ws[0]) == HEIGHT * WIDTH
        out.append("  %d samples a pass:" % n)
        for name, _ in sides:
            out.append("    %-36s %s" % (name, fmt(ms[name])))
        med = {name: stats(v)[0] for name, v in ms.items()}
        out.append("    ratios of medians: converging zero / still %.4f, velocities / still %.4f;  plain (section 6n's) zero / soft %.4f, velocities / soft %.4f"
                   % (med["converging, zero velocities"] / med["converging, still"], med["converging, velocities"] / med["converging, still"],
                      med["plain motion pass, zero velocities"] / med["plain soft pass"], med["plain motion pass, velocities"] / med["plain soft pass"]))
    out.append("")
    del b

    # ---- 2. the headline
    out.append("2. The headline: tolerance %g, min_samples %d, at most %d samples, ticks of %d; kernel ms are the library's own HIP events, summed." % (
        TOLERANCE, MIN_SAMPLES, MAX_SAMPLES, TICK))
    ticks, kernel_ms, report = 0, 0., None
    while report is None or report.listed > 0:
        timing, report = ctx.render_converging_motion(p, velocities, SHUTTER, APERTURE, FOCUS, TICK, TOLERANCE, MIN_SAMPLES, MAX_SAMPLES,
                                                      restart=report is None)
        ticks, kernel_ms = ticks + 1, kernel_ms + timing.kernel_ms
    out.append("  rm_render_converging_motion, test velocities:  %4d ticks, %9.1f kernel ms, %13d samples cast, largest count %d" % (
        ticks, kernel_ms, report.samples_cast, report.max_count))
    plain_ticks, plain_ms, total = 0, 0., 0
    while total < MAX_SAMPLES:
        timing, total = ctx.render_progressive_motion(p, velocities, SHUTTER, APERTURE, FOCUS, TICK, restart=plain_ticks == 0)
        plain_ticks, plain_ms = plain_ticks + 1, plain_ms + timing.kernel_ms
    plain_cast = HEIGHT * WIDTH * MAX_SAMPLES
    out.append("  rm_render_progressive_motion ticked to %d:     %4d ticks, %9.1f kernel ms, %13d samples cast" % (MAX_SAMPLES, plain_ticks, plain_ms, plain_cast))
    out.append("  converging / plain: %.4f of the kernel time, %.4f of the samples" % (kernel_ms / plain_ms, report.samples_cast / plain_cast))
    still_ticks, still_ms, report = 0, 0., None
    while report is None or report.listed > 0:
        timing, report = ctx.render_converging(p, APERTURE, FOCUS, TICK, TOLERANCE, MIN_SAMPLES, MAX_SAMPLES, restart=report is None)
        still_ticks, still_ms = still_ticks + 1, still_ms + timing.kernel_ms
    out.append("  rm_render_converging, the still scene:         %4d ticks, %9.1f kernel ms, %13d samples cast, largest count %d" % (
        still_ticks, still_ms, report.samples_cast, report.max_count))
    ctx.close()
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
