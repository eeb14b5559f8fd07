"""Adaptive anti-aliasing on one MI355X: HIP events around each step on one stream, 3 warm-up
runs, median and minimum of REPS runs, at C2 (demo, depth 5) and C3 (Cornell, depth 5), 1920x1080.

  (a) rm_render_device alone: the 1-sample frame, the floor;
  (b) (a) + rm_refine_device for n in 2, 3, 4 at threshold 0.125, with the share of pixels refined (and rm_refine_device
      alone at threshold +inf: memset, mark and a shade launch that finds an empty list -- the refine's floor);
  (c) the way to the same picture without the refine: rm_radiance_samples_device over all n * n positions of every
      pixel + the torch mean, as Renderer.render_supersampled does it.

Before anything is timed, (b) at threshold -1 and (c) are checked to agree within 1e-9 on a 64x64 frame.  Reported per
row: (b) against (c), and (b) - (a) against share refined x n * n x (c)'s cost per sample -- what grouping a pixel's samples
into neighbouring lanes bought, or did not.

Usage: python profiles/antialias_figures.py [--reps 25] [--out profiles/raw/antialias_figures.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import __graft_entry__ as G  # noqa: E402
import workloads  # noqa: E402
from query_figures import timed  # noqa: E402

TIGHT = 1e-9
THRESHOLD = 0.125


def positions(w, rows, n):
    """[y][x][j][i] pairs (x + i / n, y + j / n) on the device, as Renderer.render_supersampled builds them."""
    f64, dev = torch.float64, "cuda:0"
    sub = torch.arange(n, dtype=f64, device=dev) / n
    sx = torch.arange(w, dtype=f64, device=dev)[:, None] + sub[None, :]
    sy = torch.arange(rows, dtype=f64, device=dev)[:, None] + sub[None, :]
    xy = torch.empty((rows, w, n, n, 2), dtype=f64, device=dev)
    xy[..., 0] = sx[None, :, None, :]
    xy[..., 1] = sy[:, None, :, None]
    return xy.view(-1, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw", "antialias_figures.json"))
    args = ap.parse_args()
    pkg = G.load_package()
    L, B = pkg.lib(), pkg._lib
    ctx = pkg.backend.Context(0)
    stream = torch.cuda.current_stream().cuda_stream

    def refine(p, frame, ws, n, threshold):
        r = B.rm_refine(n, 0, threshold)
        B.check(L.rm_refine_device(ctx.ptr, C.byref(p), C.byref(r), C.c_void_p(frame.data_ptr()), C.c_void_p(ws.data_ptr()), None,
                                   C.c_void_p(stream)), ctx.ptr)

    def supersampled(p, xy, rows, w, n):
        rgb = ctx.radiance_samples_device(p, xy, stream=stream)
        return rgb.view(rows, w, n * n, 3).sum(dim=2) / float(n * n)

    rows_out = []
    for cfg in ("C2", "C3"):
        c = workloads.CONFIGS[cfg]
        ctx.upload(workloads.product_scene(pkg, c["scene"]).flatten())
        depth = c["max_depth"]
        # ---- the two ways agree before either is timed
        small = pkg.backend.make_params(workloads.FOV, 64., 64., depth)
        f = torch.zeros((64, 64, 3), dtype=torch.float64, device="cuda:0")
        ws = torch.zeros((ctx.refine_workspace(small) // 4,), dtype=torch.int32, device="cuda:0")
        for n in (2, 3, 4):
            ctx.render_device(small, f.data_ptr(), stream)
            refine(small, f, ws, n, -1.)
            delta = float((f - supersampled(small, positions(64, 64, n), 64, 64, n)).abs().max())
            assert int(ws[0]) == 64 * 64 and delta < TIGHT, (cfg, n, int(ws[0]), delta)
        # ---- the frame of the config
        w, h = c["width"], c["height"]
        rows = (h // 32) * 32
        p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)
        frame = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
        ws = torch.zeros((ctx.refine_workspace(p) // 4,), dtype=torch.int32, device="cuda:0")
        ren_ms = timed(lambda: ctx.render_device(p, frame.data_ptr(), stream), args.reps)
        # the refine's own floor: at threshold +inf the memset, the mark launch and a shade launch that finds an empty list
        ctx.render_device(p, frame.data_ptr(), stream)
        floor_ms = timed(lambda: refine(p, frame, ws, 2, float("inf")), args.reps)
        assert int(ws[0]) == 0
        for n in (2, 3, 4):
            def both():
                ctx.render_device(p, frame.data_ptr(), stream)
                refine(p, frame, ws, n, THRESHOLD)
            aa_ms = timed(both, args.reps)
            share = int(ws[0]) / float(rows * w)
            xy = positions(w, rows, n)
            ss_ms = timed(lambda: supersampled(p, xy, rows, w, n), args.reps)
            per_sample_ms = ss_ms[0] / (rows * w * n * n)
            row = {"config": cfg, "scene": c["scene"], "width": w, "height": h, "max_depth": depth, "n": n, "threshold": THRESHOLD,
                   "render_ms": ren_ms, "refine_nothing_ms": floor_ms, "antialiased_ms": aa_ms, "supersampled_ms": ss_ms, "share_refined": share,
                   "refined_pixels": int(ws[0]), "antialiased_over_supersampled": aa_ms[0] / ss_ms[0],
                   "refine_ms": aa_ms[0] - ren_ms[0], "same_samples_at_supersampled_cost_ms": share * rows * w * n * n * per_sample_ms}
            print(json.dumps(row), flush=True)
            rows_out.append(row)
            del xy
            torch.cuda.empty_cache()
        del frame, ws
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows_out}, fh, indent=1)


if __name__ == "__main__":
    main()
