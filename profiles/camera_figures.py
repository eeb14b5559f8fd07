"""What a turned view costs on one MI355X: HIP events on one stream, after warm-up.

  C2 (demo 1920x1080, depth 5), rm_render_device: the fixed view (its own kernels) against the fixed view yawed by
  1e-3 rad (practically the same picture through the oriented kernels) -- standing views, median of REPS launches each,
  the two measured in alternating blocks so that a drift of the machine shows in both;
  a lap of workloads.camera_walk (244 positions, a press of the reference's buttons between frames) without a turn and
  with 3 degrees of yaw added per frame: events around the whole lap, LAPS laps each, alternating, median lap.

Usage: python profiles/camera_figures.py [--reps 200] [--laps 7] [--out profiles/raw/camera_figures.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402
import workloads  # noqa: E402


def launches(fn, reps):
    s = torch.cuda.current_stream()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def summary(ms):
    return {"median_us": statistics.median(ms) * 1e3, "min_us": min(ms) * 1e3, "max_us": max(ms) * 1e3, "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--laps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw", "camera_figures.json"))
    args = ap.parse_args()
    pkg = G.load_package()
    B = pkg.backend
    ctx = B.Context(0)
    stream = torch.cuda.current_stream().cuda_stream
    c = workloads.CONFIGS["C2"]
    w, h, depth = c["width"], c["height"], c["max_depth"]
    ctx.upload(workloads.product_scene(pkg, c["scene"]).flatten())
    p = B.make_params(workloads.FOV, float(h), float(w), depth)
    frame = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    render = lambda: ctx.render_device(p, frame.data_ptr(), stream)
    out = {"device": torch.cuda.get_device_name(0), "config": "C2", "reps": args.reps, "laps": args.laps}

    # ---- standing views: fixed against yawed by 1e-3 rad, in alternating blocks
    yawed = B.basis_turn(B.FIXED_VIEW, 1e-3, 0., 0.)
    views = {"fixed": None, "yawed_1e-3": yawed}
    names = {}
    ms = {k: [] for k in views}
    blocks = 4
    for _ in range(blocks):
        for k, b in views.items():
            ctx.orient(b)
            names[k] = ctx.kernel_name(p)
            for _ in range(20):                               # (the view's order and frozen launches settle)
                render()
            torch.cuda.synchronize()
            ms[k] += launches(render, args.reps // blocks)
    ctx.orient(None)
    out["standing"] = {k: dict(summary(v), kernel=names[k]) for k, v in ms.items()}
    f, y = out["standing"]["fixed"]["median_us"], out["standing"]["yawed_1e-3"]["median_us"]
    out["standing"]["yawed_over_fixed"] = y / f
    print(json.dumps({"standing": out["standing"]}), flush=True)

    # ---- the walk: a lap without a turn, a lap with 3 degrees of yaw per frame
    walk = workloads.camera_walk()
    s = torch.cuda.current_stream()

    def lap(turn_deg):
        basis = B.basis_turn(B.FIXED_VIEW, 0., 0., 0.)
        ctx.orient(None)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        for pos in walk:
            ctx.set_camera(pos)
            if turn_deg:
                basis = B.basis_turn(basis, math.radians(turn_deg), 0., 0.)
                ctx.orient(basis)
            render()
        b.record(s)
        b.synchronize()
        return a.elapsed_time(b)

    laps = {"no_turn": [], "yaw_3deg_per_frame": []}
    for k in (0., 3.):
        lap(k)                                                # warm-up: both sets of kernels loaded, lists allocated
    for _ in range(args.laps):
        laps["no_turn"].append(lap(0.))
        laps["yaw_3deg_per_frame"].append(lap(3.))
    ctx.orient(None)
    out["walk"] = {"frames_per_lap": len(walk)}
    for k, v in laps.items():
        med = statistics.median(v)
        out["walk"][k] = {"median_lap_ms": med, "min_lap_ms": min(v), "max_lap_ms": max(v), "us_per_frame": med / len(walk) * 1e3,
                          "frames_per_s": len(walk) / (med * 1e-3)}
    print(json.dumps({"walk": out["walk"]}), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(out, fo, indent=1)


if __name__ == "__main__":
    main()
