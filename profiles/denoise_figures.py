"""The variance-guided filter on one MI355X.  One GPU step; run it under a time limit of its own:

    timeout -k 10 500 python profiles/denoise_figures.py --out <file>

The frame: the demo scene at 1920x1056, depth 5, two converging passes of 8 samples that list every pixel (tolerance < 0), and
the hits of rm_primary_hits_device under it.  Timed on it, HIP events around each call on one stream, WARM warm-up calls of each
side, then REPS of each, interleaved (side A, side B, ..., side A, ...): median, minimum, maximum.

  (b)  the yardstick of cost: one more converging pass of 8 samples that lists every pixel (memset + select + shade), every
       count 8 beforehand -- measured in the same session.
  T(k) rm_denoise_device with iterations = k, k = 0 .. 5, all three outputs, guided and unguided, for every setting of
       RM_DENOISE_TILED (0: every step gathers from global memory; 1, 2, 3: step 1, step 2, both stage their tile in LDS).  A
       call is the prepare launch and k iteration launches, so the cost of step 1 << (k - 1) is T(k) - T(k - 1) of the medians --
       taken between calls whose earlier steps took the same path -- and T(0) is the prepare launch (which with k = 0 writes
       the outputs instead of the plane and the guide).
  (a)  the HBM floor of each launch from the bytes it must move a pixel, at ACHIEVABLE TB/s (what a streaming copy reaches on
       this chip; the data sheet says 8.0): prepare reads sum, stats, count (44 B) and the rm_hit (72 B) and writes the plane
       (32 B) and the guide (64 B); an iteration reads the plane, the count and the guide (32 + 4 + 64 B) and writes the plane (32 B),
       the last one the three outputs (35 B) instead.

A path is chosen over the gather for a step only where it wins by more than the gather's own max / min spread in this session.
Before anything is timed the settings are checked against each other on the whole frame: the same bytes in all three outputs.

Usage: python profiles/denoise_figures.py [--reps 20] [--out profiles/raw/denoise_figures.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402
import workloads  # noqa: E402

WARM = 3
WIDTH, HEIGHT, DEPTH = 1920, 1056, 5
APERTURE, FOCUS, NS = 0.4, 5., 8
ACHIEVABLE = 6.3e12                                                     # bytes a second a streaming kernel reaches
KNOB = "RM_DENOISE_TILED"


def event_ms(before, fn, stream):
    before()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def floor_ms(pixels, k, guided, step_index):
    """The HBM floor of launch `step_index` (0: prepare, i: iteration i) of a call with k iterations."""
    last = step_index == k
    if step_index == 0:
        moved = 44 + (35 if last else 32) + ((72 + 64) if guided and not last else 0)
    else:
        moved = 36 + (64 if guided else 0) + (35 if last else 32)
    return moved * pixels / ACHIEVABLE * 1e3, moved


def fmt(v):
    return "%8.3f (%8.3f .. %8.3f)" % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    path = args.out or os.path.join(ROOT, "profiles", "raw", "denoise_figures.txt")
    pkg = G.load_package()
    ctx = pkg.backend.Context(0)
    s = torch.cuda.current_stream()
    f64, u8, i32, dev = torch.float64, torch.uint8, torch.int32, "cuda:0"
    ctx.orient(None)
    ctx.upload(workloads.product_scene(pkg, "demo").flatten())
    p = pkg.backend.make_params(workloads.FOV, float(HEIGHT), float(WIDTH), DEPTH)
    pixels = HEIGHT * WIDTH
    total, stats = torch.zeros((HEIGHT, WIDTH, 3), dtype=f64, device=dev), torch.zeros((HEIGHT, WIDTH, 2), dtype=f64, device=dev)
    count = torch.zeros((HEIGHT, WIDTH), dtype=i32, device=dev)
    table = torch.from_numpy(ctx.lens_sequence(0, 3 * NS)).to(dev)
    ws = torch.empty((ctx.converge_workspace(p) // 4,), dtype=i32, device=dev)

    def converge_pass(fresh, most):
        ctx.accumulate_converging_device(p, total, stats, count, APERTURE, FOCUS, NS, table, -1., 0, most, fresh, workspace=ws)

    converge_pass(True, 3 * NS)
    converge_pass(False, 3 * NS)
    hits = ctx.primary_hits_device(p)
    torch.cuda.synchronize()
    assert int(count.min()) == int(count.max()) == 2 * NS
    out = ["The variance-guided filter on %s (profiles/denoise_figures.py, %d calls a side, %d warm-up, interleaved)." % (
               torch.cuda.get_device_name(0), args.reps, WARM),
           "Demo scene, %dx%d, depth %d, aperture %g, focus %g, every pixel 16 samples; median (min .. max) in ms, HIP events." % (
               WIDTH, HEIGHT, DEPTH, APERTURE, FOCUS), ""]

    # ---- (b) the converging pass that lists every pixel, on buffers of its own
    total_b, stats_b, count_b = total.clone(), stats.clone(), count.clone()

    def reset_b():
        count_b.fill_(NS)

    def pass_b():
        ctx.accumulate_converging_device(p, total_b, stats_b, count_b, APERTURE, FOCUS, NS, table, -1., 0, 2 * NS, False, workspace=ws)

    for _ in range(WARM):
        reset_b()
        pass_b()
    torch.cuda.synchronize()
    b_ms = [event_ms(reset_b, pass_b, s) for _ in range(args.reps)]
    b_med = statistics.median(b_ms)
    out += ["(b) converging pass, 8 samples, every pixel listed:  %s   max / min %.4f" % (fmt(b_ms), max(b_ms) / min(b_ms)), ""]

    res, var, rgb8 = torch.zeros((HEIGHT, WIDTH, 3), dtype=f64, device=dev), torch.zeros((HEIGHT, WIDTH), dtype=f64, device=dev), \
        torch.zeros((HEIGHT, WIDTH, 3), dtype=u8, device=dev)
    dws = torch.empty((ctx.denoise_workspace(p),), dtype=u8, device=dev)

    def call(k, guided, knob):
        os.environ[KNOB] = knob
        ctx.denoise_device(p, total, stats, count, res, iterations=k, hits=hits if guided else None, variance=var, rgb8=rgb8, workspace=dws)

    # ---- the settings write the same bytes
    for guided in (True, False):
        seen = None
        for knob in "0123":
            call(5, guided, knob)
            torch.cuda.synchronize()
            now = (res.cpu().numpy().tobytes(), var.cpu().numpy().tobytes(), rgb8.cpu().numpy().tobytes())
            assert seen is None or now == seen, "RM_DENOISE_TILED=%s writes other bytes (guided: %s)" % (knob, guided)
            seen = now
    out += ["RM_DENOISE_TILED = 0, 1, 2, 3 write the same bytes in all three outputs, guided and unguided (5 iterations, the whole frame).", ""]

    # ---- T(k): the sides of one k interleaved
    for guided in (True, False):
        out.append("%s:" % ("guided (hits of rm_primary_hits_device)" if guided else "unguided"))
        T = {}
        for k in range(6):
            knobs = {0: ["0"], 1: ["0", "1"], 2: ["0", "2", "3"]}.get(k, ["0", "3"])
            for knob in knobs:
                for _ in range(WARM):
                    call(k, guided, knob)
            torch.cuda.synchronize()
            ms = {knob: [] for knob in knobs}
            for _ in range(args.reps):
                for knob in knobs:
                    ms[knob].append(event_ms(lambda: None, lambda: call(k, guided, knob), s))
            for knob in knobs:
                T[(k, knob)] = ms[knob]
                out.append("  T(%d) iterations = %d, RM_DENOISE_TILED=%s   %s   max / min %.4f   = %.2f x (b)" % (
                    k, k, knob, fmt(ms[knob]), max(ms[knob]) / min(ms[knob]), statistics.median(ms[knob]) / b_med))
        med = {key: statistics.median(v) for key, v in T.items()}
        out.append("  launch by launch, beside the HBM floor at %.1f TB/s:" % (ACHIEVABLE / 1e12))
        line = "    %-44s %8.3f ms   floor %6.3f ms (%3d B a pixel)   %5.1f x the floor"
        fl, moved = floor_ms(pixels, 0, guided, 0)
        out.append(line % ("prepare, writing the outputs: T(0)", med[(0, "0")], fl, moved, med[(0, "0")] / fl))
        (f0, m0), (f1, m1) = floor_ms(pixels, 1, guided, 0), floor_ms(pixels, 1, guided, 1)
        out.append(line % ("prepare + step 1, gather: T(1)", med[(1, "0")], f0 + f1, m0 + m1, med[(1, "0")] / (f0 + f1)))
        out.append(line % ("prepare + step 1, tiled: T(1)", med[(1, "1")], f0 + f1, m0 + m1, med[(1, "1")] / (f0 + f1)))
        steps = [("step 2, gather: T(2) - T(1)", med[(2, "0")] - med[(1, "0")]), ("step 2, tiled: T(2) - T(1)", med[(2, "2")] - med[(1, "0")]),
                 ("step 2, tiled behind a tiled step 1", med[(2, "3")] - med[(1, "1")]),
                 ("step 4, gather: T(3) - T(2)", med[(3, "0")] - med[(2, "0")]), ("step 8, gather: T(4) - T(3)", med[(4, "0")] - med[(3, "0")]),
                 ("step 16, gather: T(5) - T(4)", med[(5, "0")] - med[(4, "0")])]
        fl, moved = floor_ms(pixels, 6, guided, 2)                       # (an iteration that is not the last: it writes the plane)
        for name, ms_ in steps:
            out.append(line % (name, ms_, fl, moved, ms_ / fl))
        out.append("  the whole filter, 5 iterations: gather %.3f ms = %.2f x (b); steps 1 and 2 tiled %.3f ms = %.2f x (b)" % (
            med[(5, "0")], med[(5, "0")] / b_med, med[(5, "3")], med[(5, "3")] / b_med))
        # the choice: the step's own cost where a difference gives it (step 2), the call's where not (step 1: the prepare launch
        # is in both sides, which only makes the test harder to pass)
        for k, knob, what, base in ((1, "1", "step 1", 0.), (2, "2", "step 2", med[(1, "0")])):
            spread = max(T[(k, "0")]) / min(T[(k, "0")])
            tiled, gather = med[(k, knob)] - base, med[(k, "0")] - base
            wins = tiled * spread < gather
            out.append("  %s: tiled / gather = %.3f / %.3f ms = %.4f, the gather's max / min of T(%d) %.4f -> %s" % (
                what, tiled, gather, tiled / gather, k, spread, "the tiled path wins" if wins else "the gather stays"))
        out.append("")
        text = "\n".join(out) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:                                     # (after every half: a step cut short keeps what it measured)
            fh.write(text)
    os.environ.pop(KNOB, None)
    ctx.close()
    print(text)


if __name__ == "__main__":
    main()
