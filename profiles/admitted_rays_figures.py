"""Closest hits of 1 M unit rays on the 256 spheres (the hierarchy kernel of rm_intersect_rays_device), timed with HIP events
around each launch after warm-up: what the unit-length vote of rm_query.hip (a dot product and a ballot a ray, DESIGN.md
section 6b) costs the rays that pass it.  Prints one JSON line: median / min / max of REPS launches in microseconds and a
SHA-256 of the hit records, so that two builds can be told apart or found equal on the same seeded rays.

Two builds are compared by running this file once per build (RM_LIB_PATH names the other library), alternating, in one
session on one GPU.

--stretch E times the same rays stretched to d.d = 1 + E instead: with E beyond 1e-14 every wave takes the complete walk.

Usage: python profiles/admitted_rays_figures.py [--reps 50] [--rays 1048576] [--stretch 9e-5]
"""
import argparse
import hashlib
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
from profiles.query_figures import scene_bounds, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--stretch", type=float, default=0., help="d.d - 1 of every ray: what the complete walk costs a wave that fails the vote")
    args = ap.parse_args()
    pkg = G.load_package()
    ctx = pkg.backend.Context(0)
    handle = workloads.product_scene(pkg, "synthetic256").flatten()
    ctx.upload(handle)
    rng = np.random.default_rng(1)
    lo, hi = scene_bounds(handle.desc())
    o = torch.from_numpy(rng.uniform(lo, hi, size=(args.rays, 3))).to("cuda:0")
    d = torch.from_numpy(rng.normal(size=(args.rays, 3))).to("cuda:0")
    d /= torch.linalg.norm(d, dim=1, keepdim=True)
    d *= (1. + args.stretch) ** 0.5
    stream = torch.cuda.current_stream().cuda_stream
    med, low, high = timed(lambda: ctx.intersect_device(o, d, stream=stream), args.reps, warm=5)
    hits = ctx.intersect_device(o, d, stream=stream).raw.cpu().numpy()
    print(json.dumps({"library": pkg._lib.LIB_PATH, "rays": args.rays, "stretch": args.stretch, "reps": args.reps, "closest_us": [round(1e3 * x, 2) for x in (med, low, high)],
                      "hit": int(hits.view(pkg.backend.HIT_DTYPE)["hit"].sum()), "sha256": hashlib.sha256(hits.tobytes()).hexdigest()}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
