"""Radiance-query throughput on one MI355X: HIP events around each launch on one stream, 3 warm-up
launches, median and minimum of REPS launches.

  samples at the integer positions of a 1920x1080 frame (rm_radiance_samples_device) at C2 (demo, depth 5) and C3
  (Cornell, depth 5), beside the render kernel (rm_render_device) with the same params on the same stream: the same
  rays, once through the tiled, classified, culled render launch and once through the query;
  16 M incoherent random rays per scene (origins uniform in the scene's padded bounds, directions normalised
  Gaussians) through rm_radiance_rays_device at the config's depth cap.

Usage: python profiles/radiance_figures.py [--reps 25] [--rays 16777216] [--out profiles/raw/radiance_figures.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import __graft_entry__ as G  # noqa: E402
import workloads  # noqa: E402
from query_figures import scene_bounds, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--rays", type=int, default=16 * 1024 * 1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw", "radiance_figures.json"))
    args = ap.parse_args()
    pkg = G.load_package()
    ctx = pkg.backend.Context(0)
    stream = torch.cuda.current_stream().cuda_stream
    rows_out = []
    for cfg in ("C2", "C3"):
        c = workloads.CONFIGS[cfg]
        w, h, depth = c["width"], c["height"], c["max_depth"]
        handle = workloads.product_scene(pkg, c["scene"]).flatten()
        ctx.upload(handle)
        desc = handle.desc()
        p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)
        rows = (h // 32) * 32
        frame = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
        ys, xs = torch.meshgrid(torch.arange(rows, dtype=torch.float64, device="cuda:0"),
                                torch.arange(w, dtype=torch.float64, device="cuda:0"), indexing="ij")
        xy = torch.stack([xs.reshape(-1), ys.reshape(-1)], dim=1).contiguous()
        ren_ms = timed(lambda: ctx.render_device(p, frame.data_ptr(), stream), args.reps)
        sam_ms = timed(lambda: ctx.radiance_samples_device(p, xy, stream=stream), args.reps)
        # the two launches computed the same picture
        delta = float((ctx.radiance_samples_device(p, xy, stream=stream).view(rows, w, 3) - frame[:rows]).abs().max())
        rng = np.random.default_rng(1)
        lo, hi = scene_bounds(desc)
        o = torch.from_numpy(rng.uniform(lo, hi, size=(args.rays, 3))).to("cuda:0")
        d = torch.from_numpy(rng.normal(size=(args.rays, 3))).to("cuda:0")
        d /= torch.linalg.norm(d, dim=1, keepdim=True)
        ray_ms = timed(lambda: ctx.radiance_device(o, d, max_depth=depth, stream=stream), args.reps)
        n_px = w * rows
        row = {"config": cfg, "scene": c["scene"], "width": w, "height": h, "max_depth": depth,
               "render_ms": ren_ms, "samples_ms": sam_ms, "samples_over_render": sam_ms[0] / ren_ms[0],
               "samples_per_s": n_px / (sam_ms[0] * 1e-3), "samples_bytes": n_px * (16 + 24),
               "samples_vs_render_max_delta": delta,
               "random_rays": args.rays, "rays_ms": ray_ms, "rays_per_s": args.rays / (ray_ms[0] * 1e-3)}
        print(json.dumps(row), flush=True)
        rows_out.append(row)
        del o, d, xy, frame
        torch.cuda.empty_cache()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows_out}, f, indent=1)


if __name__ == "__main__":
    main()
