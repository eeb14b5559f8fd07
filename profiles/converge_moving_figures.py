"""Converging frames with moving shapes on one MI355X.  Two GPU steps, --part pass and --part view, each a
process of its own; run each under a time limit of its own and chain them with &&:

    timeout -k 10 300 python profiles/converge_moving_figures.py --part pass --out <file> &&
    timeout -k 10 600 python profiles/converge_moving_figures.py --part view --out <file>

pass.  A pass that lists every pixel.  1920x1056, depth 5, the demo scene and the Cornell box, 8 and 64 samples a pass, tolerance
   < 0, every count n_samples beforehand (so the sum and the stats are read and every pixel casts rows n_samples .. 2 n_samples - 1):
   one rm_accumulate_converging_motion_device pass with shape offsets of zero against one rm_accumulate_converging_moving_device
   pass over the same rows and buffers -- once with a shape offset table of zeros, once with the rows of rm_motion_sequence for the
   test velocities (spheres: (2 cos(2 pi g k), 2 sin(2 pi g k), 0.5); other shapes: speed x (cos(2 pi g k + 1), 0.5 sin(2 pi g k + 1),
   0.25), speed 6 in the demo and 150 in the Cornell box; g = 0.6180339887498949, shutter 1).  Light offsets of zero (point
   lights).  HIP events around the three steps of a pass (the memset, the select launch, the shade launch) on one stream; the
   counts are put back before the first event.  WARM warm-up passes of each, then REPS of each, interleaved (motion, zero,
   velocities, motion, ...): median, minimum, maximum.  The zero-offset pass casts the moving spheres' rays exactly, so its ratio
   is the price of the rule itself.
view.  The whole view at tolerance 0.01, min_samples 16, at most 1,024 samples, in ticks of 8 with the test velocities through
   rm_render_converging_moving until a tick lists nothing: ticks, the sum of the ticks' kernel_ms (HIP events inside the library)
   and samples cast -- against rm_render_progressive_moving ticked to 1,024 samples a pixel.

Before anything is timed the sides are checked on 64x64: a zero-offset pass is the moving spheres' pass byte for byte, and a pass
with velocities is another picture.

Usage: python profiles/converge_moving_figures.py --part pass|view [--reps 20] [--out profiles/raw/converge_moving_<part>.txt]
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

WARM = 3
WIDTH, HEIGHT, DEPTH = 1920, 1056, 5
GOLDEN, SHUTTER = 0.6180339887498949, 1.
TOLERANCE, MIN_SAMPLES, MAX_SAMPLES, TICK = 0.01, 16, 1024, 8
SCENES = {"demo": (0.4, 5., 6.), "cornell": (12., 500., 150.)}       # aperture, focus, speed of what is not a sphere


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


def test_velocities(pkg, scene, speed):
    v = np.zeros((len(scene.shapes), 3))
    for k, shape in enumerate(scene.shapes):
        if isinstance(shape, pkg.sphere.Sphere):
            v[k] = (2. * np.cos(2. * np.pi * GOLDEN * k), 2. * np.sin(2. * np.pi * GOLDEN * k), 0.5)
        else:
            a = 2. * np.pi * GOLDEN * k + 1.
            v[k] = (speed * np.cos(a), speed * 0.5 * np.sin(a), speed * 0.25)
    return v


def one_pass(pkg, ctx, name, reps, out):
    aperture, focus, speed = SCENES[name]
    s = torch.cuda.current_stream()
    f64, u8, i32, dev = torch.float64, torch.uint8, torch.int32, "cuda:0"
    scene = workloads.product_scene(pkg, name)
    ctx.orient(None)
    ctx.upload(scene.flatten())
    n_lights, n_shapes = ctx.n_lights(), len(scene.shapes)
    velocities = test_velocities(pkg, scene, speed)

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
    motion, zero, moving = buffers(64, 64, float("nan")), buffers(64, 64, float("nan")), buffers(64, 64, float("nan"))
    for fresh in (True, False):
        ctx.accumulate_converging_motion_device(small, motion["sum"], motion["stats"], motion["count"], aperture, focus, 8, table, lights, zeros,
                                                -1., 0, 16, fresh, mean=motion["mean"], rgb8=motion["rgb8"])
        for b, shapes in ((zero, zeros), (moving, offsets)):
            ctx.accumulate_converging_moving_device(small, b["sum"], b["stats"], b["count"], aperture, focus, 8, table, lights, shapes, -1., 0, 16,
                                                    fresh, mean=b["mean"], rgb8=b["rgb8"])
    torch.cuda.synchronize()
    for key in motion:
        assert motion[key].cpu().numpy().tobytes() == zero[key].cpu().numpy().tobytes(), "a zero-offset pass is not the moving spheres' pass: %s" % key
    moved = int(((moving["mean"] - motion["mean"]).abs() > 0.05).any(dim=2).sum())
    assert moved > 0 and int(moving["count"].min()) == 16, "the velocities moved nothing"

    p = pkg.backend.make_params(workloads.FOV, float(HEIGHT), float(WIDTH), DEPTH)
    b = buffers(HEIGHT, WIDTH)
    ws = torch.empty((ctx.converge_workspace(p) // 4,), dtype=i32, device=dev)
    out.append("%s (%d shapes, %d lights; aperture %g, focus %g, speed %g; %d of 4,096 pixels of the 64x64 check differ with the velocities):"
               % (name, n_shapes, n_lights, aperture, focus, speed, moved))
    for n in (8, 64):
        table, lights, zeros, offsets = tables(2 * n)

        def reset():
            b["count"].fill_(n)

        def run(call, shapes):
            getattr(ctx, call)(p, b["sum"], b["stats"], b["count"], aperture, focus, n, table, lights, shapes, -1., 0, 2 * n, False,
                               mean=b["mean"], rgb8=b["rgb8"], workspace=ws)

        sides = (("converging motion, zero", lambda: run("accumulate_converging_motion_device", zeros)),
                 ("converging moving, zero", lambda: run("accumulate_converging_moving_device", zeros)),
                 ("converging moving, velocities", lambda: run("accumulate_converging_moving_device", offsets)))
        for _ in range(WARM):
            for _, fn in sides:
                reset()
                fn()
        torch.cuda.synchronize()
        ms = {side: [] for side, _ in sides}
        for _ in range(reps):
            for side, fn in sides:
                ms[side].append(event_ms(reset, fn, s))
        assert int(ws[0]) == HEIGHT * WIDTH
        out.append("  %d samples a pass:" % n)
        for side, _ in sides:
            out.append("    %-32s %s" % (side, fmt(ms[side])))
        med = {side: stats(v)[0] for side, v in ms.items()}
        out.append("    ratios of medians: moving zero / motion zero %.4f, moving velocities / motion zero %.4f; motion's own max / min %.4f"
                   % (med["converging moving, zero"] / med["converging motion, zero"], med["converging moving, velocities"] / med["converging motion, zero"],
                      max(ms["converging motion, zero"]) / min(ms["converging motion, zero"])))
    out.append("")


def whole_view(pkg, ctx, name, out):
    aperture, focus, speed = SCENES[name]
    scene = workloads.product_scene(pkg, name)
    ctx.orient(None)
    ctx.upload(scene.flatten())
    velocities = test_velocities(pkg, scene, speed)
    p = pkg.backend.make_params(workloads.FOV, float(HEIGHT), float(WIDTH), DEPTH)
    ticks, kernel_ms, report = 0, 0., None
    while report is None or report.listed > 0:
        timing, report = ctx.render_converging_moving(p, velocities, SHUTTER, aperture, focus, TICK, TOLERANCE, MIN_SAMPLES, MAX_SAMPLES,
                                                      restart=report is None)
        ticks, kernel_ms = ticks + 1, kernel_ms + timing.kernel_ms
    out.append("%s:" % name)
    out.append("  rm_render_converging_moving, test velocities:  %4d ticks, %9.1f kernel ms, %13d samples cast, largest count %d" % (
        ticks, kernel_ms, report.samples_cast, report.max_count))
    plain_ticks, plain_ms, total = 0, 0., 0
    while total < MAX_SAMPLES:
        timing, total = ctx.render_progressive_moving(p, velocities, SHUTTER, aperture, focus, TICK, restart=plain_ticks == 0)
        plain_ticks, plain_ms = plain_ticks + 1, plain_ms + timing.kernel_ms
    plain_cast = HEIGHT * WIDTH * MAX_SAMPLES
    out.append("  rm_render_progressive_moving ticked to %d:     %4d ticks, %9.1f kernel ms, %13d samples cast" % (MAX_SAMPLES, plain_ticks, plain_ms, plain_cast))
    out.append("  converging / progressive: %.4f of the kernel time, %.4f of the samples" % (kernel_ms / plain_ms, report.samples_cast / plain_cast))
    out.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["pass", "view"], required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    path = args.out or os.path.join(ROOT, "profiles", "raw", "converge_moving_%s.txt" % args.part)
    pkg = G.load_package()
    ctx = pkg.backend.Context(0)
    out = []
    if args.part == "pass":
        out += ["Converging frames with moving shapes on %s (profiles/converge_moving_figures.py --part pass, %d passes a side, %d warm-up)."
                % (torch.cuda.get_device_name(0), args.reps, WARM),
                "A pass that lists every pixel (tolerance < 0, every count n_samples beforehand), %dx%d, depth %d, shutter %g: memset + select + shade, HIP events."
                % (WIDTH, HEIGHT, DEPTH, SHUTTER), ""]
        for name in SCENES:
            one_pass(pkg, ctx, name, args.reps, out)
    else:
        out += ["The whole view on %s (profiles/converge_moving_figures.py --part view): %dx%d, depth %d, tolerance %g, min_samples %d, at most %d samples,"
                % (torch.cuda.get_device_name(0), WIDTH, HEIGHT, DEPTH, TOLERANCE, MIN_SAMPLES, MAX_SAMPLES),
                "ticks of %d; kernel ms are the library's own HIP events, summed." % TICK, ""]
        for name in SCENES:
            whole_view(pkg, ctx, name, out)
    ctx.close()
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
