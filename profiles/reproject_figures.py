"""Temporal reprojection on one MI355X.  One GPU step; run it under a time limit of its own:

    timeout -k 10 500 python profiles/reproject_figures.py --out <file>

1. Launch times.  The demo scene at 1920x1056, depth 5, area lights of radius 1.5, a pinhole: the previous frame is two
   converging passes of 8 samples that list every pixel (tolerance < 0), with the hits of rm_primary_hits_device under it; the
   current hits are those of the same view, of the view a sideways step of 0.25 on and of the view a step back of 1.0 on.
   Timed, HIP events around each call on one stream, WARM warm-up calls of each side, then REPS of each, interleaved:
     (b)  the yardstick of cost: one more converging pass of 8 samples that lists every pixel (memset + select + shade) -- what
          one tick of a restarted frame costs;
     (r)  rm_reproject_device with both optional outputs, for each of the three views (the memset of the total and the launch);
     (h)  rm_primary_hits_device, which the tick launches in front of it;
     (a)  the HBM floor of the bytes the launch must move a pixel at ACHIEVABLE TB/s (what a streaming copy reaches on this
          chip): it reads the previous sum, stats and count (44 B), both hit records (2 x 72 B) and writes sum, stats, count
          and the mask (45 B).
2. The whole view.  The demo and the Cornell box (from inside the box) at 960x544, tolerance 0.01, 8 samples a tick, at least 16
   and at most 1,024 a pixel, radii 1.5: the view is ticked until a tick lists nothing, the camera steps sideways by 0.25, and
   the new view is ticked until a tick lists nothing -- with history (max_history 32) and without.  Ticks, samples cast and the
   sum of the ticks' kernel_ms after the step.
3. The gain the tests hold as an inequality (tests/test_gpu_reproject_tick.py): the demo at 64x64, settled to 64 samples, the
   step, then the mean absolute error of one tick of 8 against the progressive frame of the new view at 1,024 samples, from
   history and restarted, and the pixels the following tick lists.

Usage: python profiles/reproject_figures.py [--reps 20] [--out profiles/raw/reproject_figures.txt]
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
NS, RADIUS = 8, 1.5
ACHIEVABLE = 6.3e12                                                     # bytes a second a streaming kernel reaches
MOVED = 44 + 2 * 72 + 45                                                # bytes a pixel the launch must move
VIEWS = (("the same view", (0., 0., 0.)), ("a sideways step of 0.25", (.25, 0., 0.)), ("a step back of 1.0", (0., 0., 1.)))
CORNELL_EYE = (278., 273., 40.)


def event_ms(before, fn, stream):
    before()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def fmt(v):
    return "%8.3f (%8.3f .. %8.3f)" % (statistics.median(v), min(v), max(v))


def launch_times(pkg, reps, out):
    ctx = pkg.backend.Context(0)
    s = torch.cuda.current_stream()
    f64, u8, i32, dev = torch.float64, torch.uint8, torch.int32, "cuda:0"
    scene = workloads.product_scene(pkg, "demo")
    ctx.orient(None)
    ctx.upload(scene.flatten())
    eye = ctx.camera()[0]
    p = pkg.backend.make_params(workloads.FOV, float(HEIGHT), float(WIDTH), DEPTH)
    pixels = HEIGHT * WIDTH
    total, stats = torch.zeros((HEIGHT, WIDTH, 3), dtype=f64, device=dev), torch.zeros((HEIGHT, WIDTH, 2), dtype=f64, device=dev)
    count = torch.zeros((HEIGHT, WIDTH), dtype=i32, device=dev)
    table = torch.from_numpy(ctx.lens_sequence(0, 3 * NS)).to(dev)
    offsets = torch.from_numpy(ctx.light_sequence(0, 3 * NS, (RADIUS,) * len(scene.lights))).to(dev)
    ws = torch.empty((ctx.converge_workspace(p) // 4,), dtype=i32, device=dev)
    for fresh in (True, False):
        ctx.accumulate_converging_device(p, total, stats, count, 0., 5., NS, table, -1., 0, 3 * NS, fresh, offsets=offsets, workspace=ws)
    view = ctx.camera()
    prev_hits = ctx.primary_hits_device(p)
    cur = {}
    for name, step in VIEWS:
        ctx.set_camera(pkg.Vec3f(eye.x + step[0], eye.y + step[1], eye.z + step[2]))
        cur[name] = ctx.primary_hits_device(p)
    torch.cuda.synchronize()
    assert int(count.min()) == int(count.max()) == 2 * NS
    out += ["1. Launch times on %s (%d calls a side, %d warm-up, interleaved)." % (torch.cuda.get_device_name(0), reps, WARM),
            "Demo scene, %dx%d, depth %d, a pinhole, radii %g, every pixel 16 samples; median (min .. max) in ms, HIP events." % (
                WIDTH, HEIGHT, DEPTH, RADIUS), ""]
    total_b, stats_b, count_b = total.clone(), stats.clone(), count.clone()

    def reset_b():
        count_b.fill_(NS)

    def pass_b():
        ctx.accumulate_converging_device(p, total_b, stats_b, count_b, 0., 5., NS, table, -1., 0, 2 * NS, False, offsets=offsets, workspace=ws)

    o_sum, o_stats = torch.zeros((HEIGHT, WIDTH, 3), dtype=f64, device=dev), torch.zeros((HEIGHT, WIDTH, 2), dtype=f64, device=dev)
    o_count, o_mask = torch.zeros((HEIGHT, WIDTH), dtype=i32, device=dev), torch.zeros((HEIGHT, WIDTH), dtype=u8, device=dev)
    o_total = torch.zeros((1,), dtype=i32, device=dev)
    hits_out = torch.zeros((HEIGHT, WIDTH, 9), dtype=f64, device=dev)

    def reproject(name):
        ctx.reproject_device(p, total, stats, count, prev_hits, cur[name], view, o_sum, o_stats, o_count, carried=o_mask, carried_total=o_total)

    def hits():
        ctx.primary_hits_device(p, out=hits_out)

    sides = [("(b)", pass_b, reset_b), ("(h)", hits, lambda: None)] + [(name, (lambda n=name: reproject(n)), lambda: None) for name, _ in VIEWS]
    for _, fn, before in sides:
        for _ in range(WARM):
            before()
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in sides}
    for _ in range(reps):
        for name, fn, before in sides:
            ms[name].append(event_ms(before, fn, s))
    b_med = statistics.median(ms["(b)"])
    floor = MOVED * pixels / ACHIEVABLE * 1e3
    out += ["(b) converging pass, 8 samples, every pixel listed:  %s   max / min %.4f" % (fmt(ms["(b)"]), max(ms["(b)"]) / min(ms["(b)"])),
            "(h) rm_primary_hits_device:                          %s   = %.2f x (b)" % (fmt(ms["(h)"]), statistics.median(ms["(h)"]) / b_med),
            "(a) the HBM floor of a reprojection at %.1f TB/s: %.3f ms (%d B a pixel)" % (ACHIEVABLE / 1e12, floor, MOVED), ""]
    for name, _ in VIEWS:
        reproject(name)
        torch.cuda.synchronize()
        carried = int(o_total.cpu()[0])
        assert carried == int(o_mask.sum())
        med = statistics.median(ms[name])
        out.append("(r) rm_reproject_device, %-26s %s   max / min %.4f   = %.2f x (b), %.1f x the floor; %d of %d pixels carried" % (
            name + ":", fmt(ms[name]), max(ms[name]) / min(ms[name]), med / b_med, med / floor, carried, pixels))
    out.append("")
    ctx.close()


def whole_view(pkg, out):
    out += ["2. The whole view: 960x544, depth 3, tolerance 0.01, 8 samples a tick, 16 .. 1024 a pixel, radii %g; the view finished, then a" % RADIUS,
            "sideways step of 0.25 and ticks until a tick lists nothing.  After the step:", ""]
    w, h = 960, 544
    for name, eye in (("demo", None), ("cornell", CORNELL_EYE)):
        scene = workloads.product_scene(pkg, name)
        radii = (RADIUS,) * len(scene.lights)
        for history in (True, False):
            ctx = pkg.backend.Context(0)
            ctx.orient(None)
            ctx.upload(scene.flatten())
            e = ctx.camera()[0]
            e = (e.x, e.y, e.z) if eye is None else eye
            p = pkg.backend.make_params(workloads.FOV, float(h), float(w), 3)
            ctx.converge_history(dict(sigma_z=.1, min_normal_dot=.9, max_history=32) if history else None)

            def finish(restart):
                ticks, kernel, rep = 0, 0., None
                while rep is None or rep.listed > 0:
                    timing, rep = ctx.render_converging(p, 0., 5., NS, .01, 16, 1024, radii=radii, restart=restart and ticks == 0)
                    ticks, kernel = ticks + 1, kernel + timing.kernel_ms
                return ticks, kernel, rep

            ctx.set_camera(pkg.Vec3f(*e))
            t0, k0, r0 = finish(True)
            ctx.set_camera(pkg.Vec3f(e[0] + .25, e[1], e[2]))
            t1, k1, r1 = finish(False)
            info = ctx.history_info()
            out.append("%-8s %-16s %4d ticks, %11d samples cast, %9.3f ms of kernels   (the first view: %d ticks, %d samples, %.3f ms)%s" % (
                name, "with history:" if history else "without:", t1, r1.samples_cast, k1, t0, r0.samples_cast, k0,
                "   carried %d of %d pixels" % (info["carried"], info["carried"] + info["without"]) if history else ""))
            ctx.close()
    out.append("")


def gain(pkg, out):
    w = h = 64
    scene = workloads.product_scene(pkg, "demo")
    radii = (RADIUS,) * len(scene.lights)
    ctx = pkg.backend.Context(0)
    ctx.orient(None)
    ctx.upload(scene.flatten())
    e = ctx.camera()[0]
    e = (e.x, e.y, e.z)
    p = pkg.backend.make_params(workloads.FOV, float(h), float(w), 3)
    out += ["3. The gain at 64x64 (demo, radii %g, a pinhole, the view settled to 64 samples a pixel, then a sideways step): mean absolute" % RADIUS,
            "error of one tick of 8 against the progressive frame of the new view at 1,024 samples; pixels listed by the tick after it.", ""]
    for step in (.25, 1.):
        ctx.set_camera(pkg.Vec3f(e[0] + step, e[1], e[2]))
        truth = np.zeros((h, w, 3))
        for k in range(16):
            ctx.render_progressive_soft(p, radii, 0., 5., 64, restart=(k == 0), host_rgb=truth)
        res = {}
        for history in (True, False):
            ctx.converge_history(dict(sigma_z=.1, min_normal_dot=.9, max_history=32) if history else None)
            ctx.set_camera(pkg.Vec3f(*e))
            for k in range(8):
                ctx.render_converging(p, 0., 5., NS, -1., 8, 64, radii=radii, restart=(k == 0))
            ctx.set_camera(pkg.Vec3f(e[0] + step, e[1], e[2]))
            mean = np.zeros((h, w, 3))
            ctx.render_converging(p, 0., 5., NS, .02, 8, 1024, radii=radii, host_rgb=mean)
            res[history] = (float(np.abs(mean - truth).mean()), ctx.render_converging(p, 0., 5., NS, .02, 8, 1024, radii=radii)[1].listed)
        out.append("step %-5g with history: error %.6f, %4d pixels listed;   restarted: error %.6f, %4d pixels listed" % (
            step, res[True][0], res[True][1], res[False][0], res[False][1]))
    out.append("")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    path = args.out or os.path.join(ROOT, "profiles", "raw", "reproject_figures.txt")
    pkg = G.load_package()
    out = ["Temporal reprojection (profiles/reproject_figures.py).", ""]
    for part in (lambda: launch_times(pkg, args.reps, out), lambda: whole_view(pkg, out), lambda: gain(pkg, out)):
        part()
        text = "\n".join(out) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:                                     # (after every part: a step cut short keeps what it measured)
            fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
