"""Progressive frames on one MI355X, one GPU step.

  1. Kernel against the lens kernel.  1920x1080, depth 5, C2 (demo) and C3 (Cornell), 4 and 16 samples a pass: one
     rm_accumulate_lens_device pass with all three outputs (n_before > 0: the sum is read) against rm_render_lens_device of the
     same table -- the kernel of the parent commit, unchanged here.  HIP events around each launch on one stream, WARM warm-up
     launches of each, then REPS launches of each, interleaved (lens, pass, lens, pass, ...): median, minimum and maximum.
     A pass casts the same rays and moves 24 B (sum read) + 24 B (mean) + 3 B (bytes) a pixel more than the lens launch.
  2. Against torch.  64 samples a pixel as 16 ticks of 4 through rm_render_progressive (blocking, the bytes copied to the host
     every tick, as a viewer would) against 16 rm_render_lens_device launches of the same rows of the sequence summed in torch,
     divided and quantised there and copied once a tick too.  Wall clock around the 16 ticks, median of 5.

Before anything is timed the two sides are checked on 64x64: a pass with n_before = 0 is the lens frame byte for byte, and the
16 ticks agree with the torch average within 1e-9.

Usage: python profiles/progressive_figures.py [--reps 20] [--out profiles/raw/progressive_figures.json]
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

TIGHT = 1e-9
WARM = 5
LENS = {"demo": (0.4, 5.), "cornell": (12., 500.)}                  # (aperture, focus)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw", "progressive_figures.json"))
    args = ap.parse_args()
    pkg = G.load_package()
    ctx = pkg.backend.Context(0)
    s = torch.cuda.current_stream()
    f64, u8, dev = torch.float64, torch.uint8, "cuda:0"

    def torch_ticks(p, h, w, aperture, focus, host8):
        """16 lens launches of 4 rows of the sequence, summed, averaged and quantised in torch, the bytes copied every tick."""
        acc = torch.zeros((h, w, 3), dtype=f64, device=dev)
        frame = torch.zeros((h, w, 3), dtype=f64, device=dev)
        mean = None
        for k in range(16):
            ctx.render_lens_device(p, frame, aperture, focus, tables[k])
            acc += frame
            mean = acc / float(k + 1)                                   # (every frame is a mean of 4 already)
            host8.copy_((255. * mean.clamp(0., 1.)).to(u8))
        return mean

    def library_ticks(p, aperture, focus, host8, host=None):
        for k in range(16):
            ctx.render_progressive(p, aperture, focus, 4, restart=(k == 0), host_rgb=host, host_rgb8=host8)

    rows_out = []
    for cfg in ("C2", "C3"):
        c = workloads.CONFIGS[cfg]
        ctx.orient(None)
        ctx.upload(workloads.product_scene(pkg, c["scene"]).flatten())
        depth = c["max_depth"]
        aperture, focus = LENS[c["scene"]]
        w, h = c["width"], c["height"]
        p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)
        small = pkg.backend.make_params(workloads.FOV, 64., 64., depth)
        tables = [torch.from_numpy(ctx.lens_sequence(4 * k, 4)).to(dev) for k in range(16)]

        # ---- the two sides agree before either is timed (64 x 64)
        t16 = torch.from_numpy(ctx.lens_sequence(0, 16)).to(dev)
        a, b, m = (torch.full((64, 64, 3), float("nan"), dtype=f64, device=dev) for _ in range(3))
        ctx.render_lens_device(small, a, aperture, focus, t16)
        ctx.accumulate_lens_device(small, b, aperture, focus, t16, 0, mean=m)
        torch.cuda.synchronize()
        assert a.cpu().numpy().tobytes() == m.cpu().numpy().tobytes(), (cfg, "a pass from nothing is not the lens frame")
        host, host8 = np.zeros((64, 64, 3)), np.zeros((64, 64, 3), np.uint8)
        library_ticks(small, aperture, focus, host8, host)
        pinned8 = torch.zeros((64, 64, 3), dtype=u8).pin_memory()
        ref = torch_ticks(small, 64, 64, aperture, focus, pinned8)
        torch.cuda.synchronize()
        delta = float((torch.from_numpy(host).to(dev) - ref).abs().max())
        assert delta < TIGHT, (cfg, delta)

        # ---- 1. one pass against one lens launch
        frame = torch.zeros((h, w, 3), dtype=f64, device=dev)
        total = torch.zeros((h, w, 3), dtype=f64, device=dev)
        mean = torch.zeros((h, w, 3), dtype=f64, device=dev)
        rgb8 = torch.zeros((h, w, 3), dtype=u8, device=dev)
        for n in (4, 16):
            table = torch.from_numpy(ctx.lens_sequence(n, n)).to(dev)       # rows n .. 2n - 1: the second pass of a frame

            def lens():
                ctx.render_lens_device(p, frame, aperture, focus, table)

            def accum():
                ctx.accumulate_lens_device(p, total, aperture, focus, table, n, mean=mean, rgb8=rgb8)

            for _ in range(WARM):
                lens()
                accum()
            torch.cuda.synchronize()
            lens_ms, accum_ms = [], []
            for _ in range(args.reps):
                lens_ms.append(event_ms(lens, s))
                accum_ms.append(event_ms(accum, s))
            row = {"what": "pass_vs_lens", "config": cfg, "scene": c["scene"], "width": w, "height": h, "max_depth": depth, "n_samples": n,
                   "lens_ms": stats(lens_ms), "accumulate_ms": stats(accum_ms), "accumulate_over_lens": stats(accum_ms)[0] / stats(lens_ms)[0],
                   "extra_bytes": (h // 32) * 32 * w * 51}
            print(json.dumps(row), flush=True)
            rows_out.append(row)

        # ---- 2. 64 samples as 16 ticks of 4: the library against lens launches averaged in torch
        del frame, total, mean, rgb8
        torch.cuda.empty_cache()
        host8 = np.zeros((h, w, 3), np.uint8)
        pinned8 = torch.zeros((h, w, 3), dtype=u8).pin_memory()
        lib_ms, torch_ms = [], []
        for rep in range(1 + 5):                                            # (the first round warms both up)
            t0 = time.perf_counter()
            library_ticks(p, aperture, focus, host8)
            t1 = time.perf_counter()
            torch_ticks(p, h, w, aperture, focus, pinned8)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if rep:
                lib_ms.append((t1 - t0) * 1e3)
                torch_ms.append((t2 - t1) * 1e3)
        row = {"what": "16_ticks_of_4", "config": cfg, "scene": c["scene"], "width": w, "height": h, "max_depth": depth,
               "agree_64x64": delta, "progressive_ms": stats(lib_ms), "torch_ms": stats(torch_ms),
               "progressive_over_torch": stats(lib_ms)[0] / stats(torch_ms)[0]}
        print(json.dumps(row), flush=True)
        rows_out.append(row)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "warm": WARM, "rows": rows_out}, fh, indent=1)


if __name__ == "__main__":
    main()
