"""Ranged ray-query throughput on one MI355X: HIP events around each launch on one stream, 3 warm-up
launches, median AND minimum of REPS launches (section 6b saw medians move by 2x between runs).

For one scene (--scene demo | cornell | synthetic256: plain walk, triangle hierarchy, sphere hierarchy) and --rays
incoherent random rays (origins uniform in the scene's padded bounds, directions normalised Gaussians):

  unranged   rm_intersect_rays_device / rm_occluded_rays_device: the parent's kernels, the baseline
  full       the ranged kernels with {0, +inf} on every ray
  mean40     the ranged kernels with {0, L}, L exponential of mean 40
  mean5      ... of mean 5
  and rm_visible_segments_device from each origin to origin + L direction (skin 1e-3) for the two lengths.

One scene per process, so that a caller can give each its own time limit.

Usage: python profiles/ranged_figures.py --scene demo [--reps 25] [--rays 16777216] [--out profiles/raw/ranged_demo.json]
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
    ap.add_argument("--scene", required=True, choices=["demo", "cornell", "synthetic256"])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--rays", type=int, default=16 * 1024 * 1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = G.load_package()
    ctx = pkg.backend.Context(0)
    stream = torch.cuda.current_stream().cuda_stream
    handle = workloads.product_scene(pkg, args.scene).flatten()
    ctx.upload(handle)
    n = args.rays
    rng = np.random.default_rng(1)
    lo, hi = scene_bounds(handle.desc())
    o = torch.from_numpy(rng.uniform(lo, hi, size=(n, 3))).to("cuda:0")
    d = torch.from_numpy(rng.normal(size=(n, 3))).to("cuda:0")
    d /= torch.linalg.norm(d, dim=1, keepdim=True)

    def row(what, kind, ms, extra=None):
        r = {"scene": args.scene, "rays": n, "query": what, "kind": kind, "median_ms": ms[0], "min_ms": ms[1], "max_ms": ms[2],
             "rays_per_s_median": n / (ms[0] * 1e-3), "rays_per_s_best": n / (ms[1] * 1e-3)}
        r.update(extra or {})
        print(json.dumps(r), flush=True)
        return r

    rows = [row("unranged", "closest", timed(lambda: ctx.intersect_device(o, d, stream=stream), args.reps)),
            row("unranged", "occluded", timed(lambda: ctx.occluded_device(o, d, stream=stream), args.reps))]
    ranges = torch.empty((n, 2), dtype=torch.float64, device="cuda:0")
    for what, mean in (("full", None), ("mean40", 40.), ("mean5", 5.)):
        ranges[:, 0] = 0.
        if mean is None:
            ranges[:, 1] = float("inf")
        else:
            ranges[:, 1] = torch.from_numpy(rng.exponential(mean, n)).to("cuda:0")
        hits = ctx.intersect_device(o, d, stream=stream, ranges=ranges)
        occ = ctx.occluded_device(o, d, stream=stream, ranges=ranges)
        torch.cuda.synchronize()
        extra = {"hit_fraction": float(hits.hit.to(torch.float64).mean()), "occluded_fraction": float(occ.to(torch.float64).mean())}
        del hits, occ
        rows.append(row(what, "closest", timed(lambda: ctx.intersect_device(o, d, stream=stream, ranges=ranges), args.reps), extra))
        rows.append(row(what, "occluded", timed(lambda: ctx.occluded_device(o, d, stream=stream, ranges=ranges), args.reps), extra))
        if mean is not None:
            to = o + d * ranges[:, 1:2]
            rows.append(row(what, "segments", timed(lambda: ctx.visible_device(o, to, 1e-3, stream=stream), args.reps)))
            del to
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
