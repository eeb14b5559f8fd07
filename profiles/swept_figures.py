"""Swept hierarchies on one MI355X.  Two GPU steps, --part pass and --part converge, each a process of
its own; run each under a time limit of its own and chain them with &&:

    timeout -k 10 400 python profiles/swept_figures.py --part pass --out <file> &&
    timeout -k 10 400 python profiles/swept_figures.py --part converge --out <file>

pass.      One pass with all three outputs at 1920x1056, depth 5, n_before = n_samples, 8 and 64 samples, point lights:
           rm_accumulate_moving_device (the flat walk, the baseline) against rm_accumulate_swept_device over the same rows and
           buffers -- once with a shape offset table of zeros (the refit's boxes are the image's: the price or gain of the walk
           alone), once with the rows of rm_motion_sequence for the test velocities (spheres: (2 cos(2 pi g k), 2 sin(2 pi g k),
           0.5); other shapes: speed x (cos(2 pi g k + 1), 0.5 sin(2 pi g k + 1), 0.25); g = 0.6180339887498949, shutter 1).  The
           handle is built once a setting from rm_swept_extents of the rows, outside the timed region.
converge.  The same columns for a converging pass that lists every pixel (tolerance < 0, every count n_samples beforehand):
           rm_accumulate_converging_moving_device against rm_accumulate_converging_swept_device, memset + select + shade.

HIP events around each launch on one stream, WARM warm-up launches of each side, then REPS of each, interleaved (flat, swept,
flat, ...): median, minimum, maximum; the flat pass's own max / min is the spread a ratio has to leave to mean anything.

Scenes: the Cornell box (36 triangles, the smallest hierarchy in the suite), the 256 spheres, and two icospheres of
profiles/mk_icosphere.py (320 and 1,280 triangles, one mesh each).  Before anything is timed the sides are checked on 64x64: the
swept pass is the flat pass byte for byte, and the velocities are another picture.

Usage: python profiles/swept_figures.py --part pass|converge [--reps 20] [--out profiles/raw/swept_<part>.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402
import workloads  # noqa: E402

WARM = 3
WIDTH, HEIGHT, DEPTH = 1920, 1056, 5
GOLDEN, SHUTTER = 0.6180339887498949, 1.
# scene -> (aperture, focus, speed of what is not a sphere, subdivisions of the icosphere or None)
SCENES = {"cornell": (12., 500., 150., None), "synthetic256": (0.4, 5., 6., None), "icosphere320": (12., 250., 150., 2),
          "icosphere1280": (12., 250., 150., 3)}


def event_ms(before, fn, stream):
    before()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def test_velocities(pkg, scene, speed):
    v = np.zeros((len(scene.shapes), 3))
    for k, shape in enumerate(scene.shapes):
        if isinstance(shape, pkg.sphere.Sphere):
            v[k] = (2. * np.cos(2. * np.pi * GOLDEN * k), 2. * np.sin(2. * np.pi * GOLDEN * k), 0.5)
        else:
            a = 2. * np.pi * GOLDEN * k + 1.
            v[k] = (speed * np.cos(a), speed * 0.5 * np.sin(a), speed * 0.25)
    return v


def scene_of(pkg, name, tmp):
    sub = SCENES[name][3]
    if sub is None:
        return workloads.product_scene(pkg, name)
    path = os.path.join(tmp, name + ".obj")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "profiles", "mk_icosphere.py"), str(sub), path], stdout=subprocess.DEVNULL)
    return pkg.Scene.open_obj(path)


def measure(pkg, ctx, name, part, reps, out, tmp):
    aperture, focus, speed, _ = SCENES[name]
    s = torch.cuda.current_stream()
    f64, u8, i32, dev = torch.float64, torch.uint8, torch.int32, "cuda:0"
    scene = scene_of(pkg, name, tmp)
    ctx.orient(None)
    handle_desc = scene.flatten()
    ctx.upload(handle_desc)
    desc = handle_desc.desc()
    n_lights, n_shapes = ctx.n_lights(), len(scene.shapes)
    velocities = test_velocities(pkg, scene, speed)
    converge = part == "converge"

    def buffers(h, w, fill=0.):
        return dict(sum=torch.full((h, w, 3), fill, dtype=f64, device=dev), stats=torch.full((h, w, 2), fill, dtype=f64, device=dev),
                    count=torch.zeros((h, w), dtype=i32, device=dev), mean=torch.full((h, w, 3), fill, dtype=f64, device=dev),
                    rgb8=torch.zeros((h, w, 3), dtype=u8, device=dev))

    def tables(first, n_rows):
        rows = ctx.motion_sequence(first, n_rows, velocities, SHUTTER)
        return (torch.from_numpy(ctx.lens_sequence(first, n_rows)).to(dev), torch.zeros((n_rows, n_lights, 3), dtype=f64, device=dev),
                {"zero": torch.zeros((n_rows, n_shapes, 3), dtype=f64, device=dev), "velocities": torch.from_numpy(rows).to(dev)})

    def launch(p, b, n, first, table, lights, shapes, swept, ws=None):
        if converge:                                                    # (the tables hold rows [0, 2 n): a pixel with count n casts n .. 2 n - 1)
            call = ctx.accumulate_converging_swept_device if swept is not None else ctx.accumulate_converging_moving_device
            kw = dict(swept=swept) if swept is not None else {}
            call(p, b["sum"], b["stats"], b["count"], aperture, focus, n, table, lights, shapes, -1., 0, 2 * n, False, mean=b["mean"],
                 rgb8=b["rgb8"], workspace=ws, **kw)
        else:
            call = ctx.accumulate_swept_device if swept is not None else ctx.accumulate_moving_device
            kw = dict(swept=swept) if swept is not None else {}
            call(p, b["sum"], aperture, focus, table, lights, shapes, first, mean=b["mean"], rgb8=b["rgb8"], **kw)

    def handle_for(shapes):
        return ctx.swept(*pkg.backend.swept_extents(shapes.cpu().numpy()))

    # ---- the sides agree before either is timed (64 x 64, rows 8 .. 16 after 8)
    small = pkg.backend.make_params(workloads.FOV, 64., 64., DEPTH)
    first = 0 if converge else 8
    table, lights, both = tables(first, 16 if converge else 8)
    means = {}
    for setting, shapes in both.items():
        handle = handle_for(shapes)
        flat, swept = buffers(64, 64), buffers(64, 64)
        for b in (flat, swept):
            b["count"].fill_(8)
        launch(small, flat, 8, 8, table, lights, shapes, None)
        launch(small, swept, 8, 8, table, lights, shapes, handle)
        torch.cuda.synchronize()
        handle.close()
        for key in flat:
            assert flat[key].cpu().numpy().tobytes() == swept[key].cpu().numpy().tobytes(), "%s, %s: the swept pass is not the flat pass: %s" % (name, setting, key)
        means[setting] = flat["mean"]
    moved = int(((means["velocities"] - means["zero"]).abs() > 0.05).any(dim=2).sum())
    assert moved > 0, "the velocities moved nothing"

    H = desc
    out.append("%s (%d shapes, %d spheres, %d triangles, %d lights; aperture %g, focus %g, speed %g; %d of 4,096 pixels of the 64x64 check differ with the velocities):"
               % (name, n_shapes, H.n_spheres, H.n_triangles, n_lights, aperture, focus, speed, moved))
    p = pkg.backend.make_params(workloads.FOV, float(HEIGHT), float(WIDTH), DEPTH)
    b = buffers(HEIGHT, WIDTH)
    ws = torch.empty((ctx.converge_workspace(p) // 4,), dtype=i32, device=dev) if converge else None
    verdict = []
    for n in (8, 64):
        table, lights, both = tables(0 if converge else n, 2 * n if converge else n)
        for setting, shapes in both.items():
            handle = handle_for(shapes)

            def reset():
                if converge:
                    b["count"].fill_(n)

            sides = (("flat", lambda: launch(p, b, n, n, table, lights, shapes, None, ws)),
                     ("swept", lambda: launch(p, b, n, n, table, lights, shapes, handle, ws)))
            for _ in range(WARM):
                for _, fn in sides:
                    reset()
                    fn()
            torch.cuda.synchronize()
            ms = {side: [] for side, _ in sides}
            for _ in range(reps):
                for side, fn in sides:
                    ms[side].append(event_ms(reset, fn, s))
            torch.cuda.synchronize()
            handle.close()
            med = {side: statistics.median(v) for side, v in ms.items()}
            spread = max(ms["flat"]) / min(ms["flat"])
            ratio = med["swept"] / med["flat"]
            verdict.append(ratio <= spread)
            out.append("  %2d samples, %-10s  flat %9.3f (%9.3f .. %9.3f)   swept %9.3f (%9.3f .. %9.3f)   swept / flat %.4f   flat max / min %.4f"
                       % (n, setting, med["flat"], min(ms["flat"]), max(ms["flat"]), med["swept"], min(ms["swept"]), max(ms["swept"]), ratio, spread))
    out.append("  swept not slower than flat by more than flat's own spread in %d of %d rows" % (sum(verdict), len(verdict)))
    out.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["pass", "converge"], required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    path = args.out or os.path.join(ROOT, "profiles", "raw", "swept_%s.txt" % args.part)
    pkg = G.load_package()
    ctx = pkg.backend.Context(0)
    what = "rm_accumulate_moving_device (flat) against rm_accumulate_swept_device" if args.part == "pass" else \
        "rm_accumulate_converging_moving_device (flat) against rm_accumulate_converging_swept_device, every pixel listed"
    out = ["Swept hierarchies on %s (profiles/swept_figures.py --part %s, %d launches a side, %d warm-up, interleaved)." % (
               torch.cuda.get_device_name(0), args.part, args.reps, WARM),
           "%s; %dx%d, depth %d, shutter %g; median (min .. max) in ms, HIP events." % (what, WIDTH, HEIGHT, DEPTH, SHUTTER), ""]
    with tempfile.TemporaryDirectory() as tmp:
        for name in args.scenes.split(","):
            measure(pkg, ctx, name, args.part, args.reps, out, tmp)
            text = "\n".join(out) + "\n"
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:                                 # (after every scene: a step cut short keeps what it measured)
                fh.write(text)
    ctx.close()
    print(text)


if __name__ == "__main__":
    main()
