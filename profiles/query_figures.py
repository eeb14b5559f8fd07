"""Ray-query throughput on one MI355X (DESIGN.md "Ray queries"): HIP events around each launch on one stream, after
warm-up, median of REPS launches.

  primary-hit buffer (rm_primary_hits_device) at C2 (demo 1920x1080), C3 (Cornell 1920x1080), C5 (256 spheres
  4096x4096), beside the render kernel (rm_render_device, the config's depth cap) at the same geometry;
  16 M incoherent random rays (origins uniform in the scene's padded bounds, directions normalised Gaussians),
  closest hit and occlusion launched separately (rm_*_rays_device).

Usage: python profiles/query_figures.py [--reps 25] [--rays 16777216] [--out profiles/raw/query_figures.json]
"""
import argparse
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


def timed(fn, reps, warm=3):
    s = torch.cuda.current_stream()
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def scene_bounds(desc):
    pts = [[desc.spheres[i].center.x, desc.spheres[i].center.y, desc.spheres[i].center.z] for i in range(desc.n_spheres)]
    pts += [[desc.polygon_vertices[i].x, desc.polygon_vertices[i].y, desc.polygon_vertices[i].z] for i in range(desc.n_polygon_vertices)]
    for i in range(desc.n_triangles):
        pts += [[v.x, v.y, v.z] for v in desc.triangles[i].vertices]
    p = np.array(pts)
    lo, hi = p.min(axis=0), p.max(axis=0)
    pad = 0.25 * (hi - lo) + 1.
    return lo - pad, hi + pad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--rays", type=int, default=16 * 1024 * 1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw", "query_figures.json"))
    args = ap.parse_args()
    pkg = G.load_package()
    ctx = pkg.backend.Context(0)
    stream = torch.cuda.current_stream().cuda_stream
    rows_out = []
    for cfg in ("C2", "C3", "C5"):
        c = workloads.CONFIGS[cfg]
        w, h, depth = c["width"], c["height"], c["max_depth"]
        handle = workloads.product_scene(pkg, c["scene"]).flatten()
        ctx.upload(handle)
        desc = handle.desc()
        p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)
        rows = (h // 32) * 32
        hits = torch.zeros((h, w, 9), dtype=torch.float64, device="cuda:0")
        frame = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
        buf_ms = timed(lambda: ctx.primary_hits_device(p, out=hits, stream=stream), args.reps)
        ren_ms = timed(lambda: ctx.render_device(p, frame.data_ptr(), stream), args.reps)
        rng = np.random.default_rng(1)
        lo, hi = scene_bounds(desc)
        o = torch.from_numpy(rng.uniform(lo, hi, size=(args.rays, 3))).to("cuda:0")
        d = torch.from_numpy(rng.normal(size=(args.rays, 3))).to("cuda:0")
        d /= torch.linalg.norm(d, dim=1, keepdim=True)
        ch_ms = timed(lambda: ctx.intersect_device(o, d, stream=stream), args.reps)
        oc_ms = timed(lambda: ctx.occluded_device(o, d, stream=stream), args.reps)
        n_px = w * rows
        row = {"config": cfg, "scene": c["scene"], "width": w, "height": h, "max_depth": depth,
               "primary_hits_ms": buf_ms, "primary_rays_per_s": n_px / (buf_ms[0] * 1e-3),
               "render_ms": ren_ms, "buffer_bytes": n_px * 72,
               "buffer_write_floor_us_at_8TBps": n_px * 72 / 8e12 * 1e6,
               "random_rays": args.rays, "closest_ms": ch_ms, "closest_rays_per_s": args.rays / (ch_ms[0] * 1e-3),
               "occluded_ms": oc_ms, "occluded_rays_per_s": args.rays / (oc_ms[0] * 1e-3)}
        print(json.dumps(row), flush=True)
        rows_out.append(row)
        del o, d, hits, frame
        torch.cuda.empty_cache()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows_out}, f, indent=1)


if __name__ == "__main__":
    main()
