"""The moving camera on one MI355X, one GPU step.  (profiles/camera_figures.py is the oriented camera's.)

Kernels against the kernels they are built over, of the same build (their code is the parent's, instruction for instruction:
profiles/camera_resource_usage.txt).  1920x1056, depth 5, 8 and 64 samples a pass, all three outputs, n_before > 0, point
lights (light offsets of zero), an oriented context (the fixed view turned by 1e-3 rad):
  static family   rm_accumulate_camera_device without a shape table against rm_accumulate_soft_device, on the demo, the Cornell
                  box and the 256 spheres -- with standing rows (the base pass's rays exactly: the ratio is the price of the
                  rule, twelve loads and three additions a group) and with the test motion;
  moving family   the same with a shape table against rm_accumulate_moving_device, on the demo and the Cornell box, the shapes
                  at moving_figures.py's velocities;
  converging      a fresh pass that lists every pixel (tolerance < 0), standing rows, against rm_accumulate_converging_device
                  with offsets and rm_accumulate_converging_moving_device.
HIP events around each launch on one stream, WARM warm-up launches of each, then REPS launches of each, interleaved: median,
minimum and maximum; each ratio is to be judged against the base pass's own spread between launches (max over min).

Before anything is timed the sides are checked on 64x64: a standing-rows pass is the base pass byte for byte.

Usage: python profiles/camera_motion_figures.py [--reps 20] [--out profiles/raw/camera_motion_figures.json]
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

WARM = 3
WIDTH, HEIGHT, DEPTH = 1920, 1056, 5
GOLDEN, SHUTTER = 0.6180339887498949, 1.
# aperture, focus, speed of what is not a sphere, camera velocity, (yaw, pitch, roll) a shutter, moving family too
SCENES = {"demo": (0.4, 5., 6., (4., 0., -2.), (0.2, 0.1, 0.), True), "cornell": (12., 500., 150., (150., 40., 0.), (0.1, 0., 0.), True),
          "synthetic256": (0.4, 5., 6., (6., 2., 0.), (0.15, 0., 0.1), False)}


def event_ms(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return statistics.median(ms), min(ms), max(ms)


def timed(sides, reps, stream):
    """sides: name -> launch.  -> name -> (median, min, max) of `reps` launches each, interleaved."""
    for _ in range(WARM):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            ms[k].append(event_ms(fn, stream))
    return {k: stats(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw", "camera_motion_figures.json"))
    args = ap.parse_args()
    pkg = G.load_package()
    K = pkg.backend
    ctx = K.Context(0)
    s = torch.cuda.current_stream()
    f64, u8, i32, dev = torch.float64, torch.uint8, torch.int32, "cuda:0"
    rows_out = []
    for name, (aperture, focus, speed, cam_v, cam_turn, with_shapes) in SCENES.items():
        scene = workloads.product_scene(pkg, name)
        ctx.upload(scene.flatten())
        ctx.orient(K.basis_turn(K.FIXED_VIEW, 1e-3, 0., 0.))
        basis = ctx.camera()[1]
        n_lights, n_shapes = ctx.n_lights(), len(scene.shapes)
        velocities = np.zeros((n_shapes, 3))
        for k, shape in enumerate(scene.shapes):
            if isinstance(shape, pkg.sphere.Sphere):
                velocities[k] = (2. * np.cos(2. * np.pi * GOLDEN * k), 2. * np.sin(2. * np.pi * GOLDEN * k), 0.5)
            else:
                a = 2. * np.pi * GOLDEN * k + 1.
                velocities[k] = (speed * np.cos(a), speed * 0.5 * np.sin(a), speed * 0.25)

        def standing(first, n):
            return K.camera_sequence(first, n, (0., 0., 0.), SHUTTER, (0., 0., 0.), basis)

        # ---- the sides agree before either is timed (64 x 64)
        small = K.make_params(workloads.FOV, 64., 64., DEPTH)
        t8 = torch.from_numpy(ctx.lens_sequence(0, 8)).to(dev)
        l8, g8 = np.zeros((8, n_lights, 3)), ctx.motion_sequence(0, 8, velocities, SHUTTER)
        soft, still, moving, both = (torch.full((64, 64, 3), float("nan"), dtype=f64, device=dev) for _ in range(4))
        ctx.accumulate_soft_device(small, soft, aperture, focus, t8, l8, 0)
        ctx.accumulate_camera_device(small, still, aperture, focus, t8, standing(0, 8), l8, None, 0)
        ctx.accumulate_moving_device(small, moving, aperture, focus, t8, l8, g8, 0)
        ctx.accumulate_camera_device(small, both, aperture, focus, t8, standing(0, 8), l8, g8, 0)
        torch.cuda.synchronize()
        assert soft.cpu().numpy().tobytes() == still.cpu().numpy().tobytes(), "a standing-rows pass is not the soft pass"
        assert moving.cpu().numpy().tobytes() == both.cpu().numpy().tobytes(), "a standing-rows pass is not the moving shapes' pass"

        p = K.make_params(workloads.FOV, float(HEIGHT), float(WIDTH), DEPTH)
        total = torch.zeros((HEIGHT, WIDTH, 3), dtype=f64, device=dev)
        mean = torch.zeros((HEIGHT, WIDTH, 3), dtype=f64, device=dev)
        rgb8 = torch.zeros((HEIGHT, WIDTH, 3), dtype=u8, device=dev)
        stat = torch.zeros((HEIGHT, WIDTH, 2), dtype=f64, device=dev)
        count = torch.zeros((HEIGHT, WIDTH), dtype=i32, device=dev)
        ws = torch.zeros((ctx.converge_workspace(p) // 4,), dtype=i32, device=dev)
        for n in (8, 64):
            table = torch.from_numpy(ctx.lens_sequence(n, n)).to(dev)           # rows n .. 2n - 1: the second pass of a frame
            lights = torch.zeros((n, n_lights, 3), dtype=f64, device=dev)
            shapes = torch.from_numpy(ctx.motion_sequence(n, n, velocities, SHUTTER)).to(dev)
            stand = torch.from_numpy(standing(n, n)).to(dev)
            moves = torch.from_numpy(K.camera_sequence(n, n, cam_v, SHUTTER, cam_turn, basis)).to(dev)
            sides = {"soft": lambda: ctx.accumulate_soft_device(p, total, aperture, focus, table, lights, n, mean=mean, rgb8=rgb8),
                     "camera_standing": lambda: ctx.accumulate_camera_device(p, total, aperture, focus, table, stand, lights, None, n, mean=mean, rgb8=rgb8),
                     "camera_moving": lambda: ctx.accumulate_camera_device(p, total, aperture, focus, table, moves, lights, None, n, mean=mean, rgb8=rgb8)}
            if with_shapes:
                sides.update({
                    "shapes": lambda: ctx.accumulate_moving_device(p, total, aperture, focus, table, lights, shapes, n, mean=mean, rgb8=rgb8),
                    "camera_shapes_standing": lambda: ctx.accumulate_camera_device(p, total, aperture, focus, table, stand, lights, shapes, n, mean=mean, rgb8=rgb8),
                    "camera_shapes_moving": lambda: ctx.accumulate_camera_device(p, total, aperture, focus, table, moves, lights, shapes, n, mean=mean, rgb8=rgb8)})
            # the converging pass that lists every pixel: fresh, tolerance < 0, tables of n rows
            conv = (-1., n, n, True)
            sides["converge"] = lambda: ctx.accumulate_converging_device(p, total, stat, count, aperture, focus, n, table, *conv, offsets=lights,
                                                                         mean=mean, rgb8=rgb8, workspace=ws)
            sides["converge_camera_standing"] = lambda: ctx.accumulate_converging_camera_device(
                p, total, stat, count, aperture, focus, n, table, stand, lights, None, *conv, mean=mean, rgb8=rgb8, workspace=ws)
            if with_shapes:
                sides["converge_shapes"] = lambda: ctx.accumulate_converging_moving_device(
                    p, total, stat, count, aperture, focus, n, table, lights, shapes, *conv, mean=mean, rgb8=rgb8, workspace=ws)
                sides["converge_camera_shapes_standing"] = lambda: ctx.accumulate_converging_camera_device(
                    p, total, stat, count, aperture, focus, n, table, stand, lights, shapes, *conv, mean=mean, rgb8=rgb8, workspace=ws)
            ms = timed(sides, args.reps, s)
            ratios = {"camera_standing/soft": ms["camera_standing"][0] / ms["soft"][0], "camera_moving/soft": ms["camera_moving"][0] / ms["soft"][0],
                      "soft max/min": ms["soft"][2] / ms["soft"][1],
                      "converge_camera_standing/converge": ms["converge_camera_standing"][0] / ms["converge"][0],
                      "converge max/min": ms["converge"][2] / ms["converge"][1]}
            if with_shapes:
                ratios.update({"camera_shapes_standing/shapes": ms["camera_shapes_standing"][0] / ms["shapes"][0],
                               "camera_shapes_moving/shapes": ms["camera_shapes_moving"][0] / ms["shapes"][0],
                               "shapes max/min": ms["shapes"][2] / ms["shapes"][1],
                               "converge_camera_shapes_standing/converge_shapes": ms["converge_camera_shapes_standing"][0] / ms["converge_shapes"][0],
                               "converge_shapes max/min": ms["converge_shapes"][2] / ms["converge_shapes"][1]})
            row = {"what": "camera_vs_base_pass", "scene": name, "width": WIDTH, "height": HEIGHT, "max_depth": DEPTH, "n_samples": n,
                   "ms (median, min, max)": ms, "ratios": ratios}
            print(json.dumps(row), flush=True)
            rows_out.append(row)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "warm": WARM, "rows": rows_out}, fh, indent=1)


if __name__ == "__main__":
    main()
