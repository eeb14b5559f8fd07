"""The thin-lens camera on one MI355X: HIP events around each way on one stream, 3 warm-up runs,
median and minimum of REPS runs, at C2 (demo, depth 5) and C3 (Cornell, depth 5), 1920x1080, for 4 and 16 rays a pixel.

  (a) rm_render_lens_device: the lens rays formed, shaded and resolved in one launch;
  (b) the way to the same picture without it: the same rays formed in torch on the device (origins and directions, 48 bytes
      a ray), rm_radiance_rays_device over them (24 bytes a ray back) and the torch mean.

Before anything is timed, (a) and (b) are checked to agree within 1e-9 on a 64x64 frame.  The table is the library's
(rm_lens_table); aperture and focus put something of the scene into the plane in focus.

Usage: python profiles/lens_figures.py [--reps 25] [--out profiles/raw/lens_figures.json]
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
LENS = {"demo": (0.4, 5.), "cornell": (12., 500.)}                  # (aperture, focus)


def lens_rays(p, rows, w, cam, aperture, focus, table):
    """Origins and unit directions of every lens ray of the rows [0, rows), [y][x][s], on the device: the header's steps 1-4
    under the fixed view, every operation a torch operation of its own (rounded once; no fused multiply-add)."""
    f64, dev = torch.float64, "cuda:0"
    n = table.shape[0]
    sx = torch.arange(w, dtype=f64, device=dev)[None, :, None] + table[:, 0][None, None, :]        # [1][x][s]
    sy = torch.arange(rows, dtype=f64, device=dev)[:, None, None] + table[:, 1][None, None, :]     # [y][1][s]
    bx = (2. * (sx / p.width - 0.5) * p.half_fov * p.ratio).expand(rows, w, n)
    by = (-2. * (sy / p.height - 0.5) * p.half_fov).expand(rows, w, n)
    d = torch.empty((rows, w, n, 3), dtype=f64, device=dev)
    o = torch.empty((rows, w, n, 3), dtype=f64, device=dev)
    au, av = aperture * table[:, 2], aperture * table[:, 3]
    o[..., 0] = cam[0] + au                                            # right (1, 0, 0), up (0, 1, 0)
    o[..., 1] = cam[1] + av
    o[..., 2] = cam[2]
    d[..., 0] = (cam[0] + bx * focus) - o[..., 0]
    d[..., 1] = (cam[1] + by * focus) - o[..., 1]
    d[..., 2] = (cam[2] + -1. * focus) - o[..., 2]
    inv = 1. / torch.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    d *= inv[..., None]
    return o.view(-1, 3), d.view(-1, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw", "lens_figures.json"))
    args = ap.parse_args()
    pkg = G.load_package()
    L, B = pkg.lib(), pkg._lib
    ctx = pkg.backend.Context(0)
    stream = torch.cuda.current_stream().cuda_stream

    def lens(p, frame, table, aperture, focus):
        ln = B.rm_lens(aperture, focus, table.shape[0], 0)
        B.check(L.rm_render_lens_device(ctx.ptr, C.byref(p), C.byref(ln), C.c_void_p(table.data_ptr()), C.c_void_p(frame.data_ptr()),
                                        C.c_void_p(stream)), ctx.ptr)

    def by_rays(p, rows, w, cam, table, aperture, focus, depth):
        o, d = lens_rays(p, rows, w, cam, aperture, focus, table)
        rgb = ctx.radiance_device(o, d, max_depth=depth, stream=stream)
        n = table.shape[0]
        return rgb.view(rows, w, n, 3).sum(dim=2) / float(n)

    rows_out = []
    for cfg in ("C2", "C3"):
        c = workloads.CONFIGS[cfg]
        ctx.orient(None)
        ctx.upload(workloads.product_scene(pkg, c["scene"]).flatten())
        pos, _, _ = ctx.camera()
        cam = (pos.x, pos.y, pos.z)
        depth = c["max_depth"]
        aperture, focus = LENS[c["scene"]]
        w, h = c["width"], c["height"]
        rows = (h // 32) * 32
        p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)
        small = pkg.backend.make_params(workloads.FOV, 64., 64., depth)
        for n in (4, 16):
            table = torch.from_numpy(ctx.lens_table(n)).to("cuda:0")
            # ---- the two ways agree before either is timed
            f = torch.zeros((64, 64, 3), dtype=torch.float64, device="cuda:0")
            lens(small, f, table, aperture, focus)
            delta = float((f - by_rays(small, 64, 64, cam, table, aperture, focus, depth)).abs().max())
            assert delta < TIGHT, (cfg, n, delta)
            # ---- the frame of the config
            frame = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
            lens_ms = timed(lambda: lens(p, frame, table, aperture, focus), args.reps)
            rays_ms = timed(lambda: by_rays(p, rows, w, cam, table, aperture, focus, depth), args.reps)
            o, d = lens_rays(p, rows, w, cam, aperture, focus, table)
            cast_ms = timed(lambda: ctx.radiance_device(o, d, max_depth=depth, stream=stream), args.reps)
            row = {"config": cfg, "scene": c["scene"], "width": w, "height": h, "max_depth": depth, "n_samples": n, "aperture": aperture,
                   "focus": focus, "agree_64x64": delta, "lens_ms": lens_ms, "rays_ms": rays_ms, "rays_cast_only_ms": cast_ms,
                   "lens_over_rays": lens_ms[0] / rays_ms[0], "rays": rows * w * n}
            print(json.dumps(row), flush=True)
            rows_out.append(row)
            del frame, o, d
            torch.cuda.empty_cache()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows_out}, fh, indent=1)


if __name__ == "__main__":
    main()
