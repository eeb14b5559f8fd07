"""What the plain-walk kernels' generic tile body costs now that it lives beside a body compiled for the default scene's
counts ("scene signatures"): no bench config runs it any more.  The default scene plus one sphere -- five
spheres: no signature, same kernel -- at 1920x1080, depth cap 5, kernel time by the library's own events:
    python profiles/near_miss_time.py [frames]            (RM_LIB_PATH names another build's library)
-> one line: kernel us median / min / max over the frames, after as many warm-up frames as it takes the order to settle."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry   # noqa: E402
import workloads                  # noqa: E402

W, H, DEPTH, WARMUP = 1920, 1080, 5, 20


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    pkg = entry.load_package()
    scene = pkg.Scene.create_default()
    scene.shapes.append(pkg.sphere.create(pkg.Vec3f(3., 3., -12.), 1.5, pkg.Reflectance(diffuse_color=(0.8, 0., 0.), specular_exponent=100.)))
    ctx = pkg.backend.Context(0)
    try:
        ctx.upload(scene.flatten())
        p = pkg.backend.make_params(workloads.FOV, float(H), float(W), DEPTH)
        out = np.zeros((H, W, 3), dtype=np.float64)
        us = [ctx.render(p, out).kernel_ms * 1e3 for _ in range(WARMUP + frames)][WARMUP:]
    finally:
        ctx.close()
    lit = int((out.sum(axis=2) > 0).sum())
    print("near miss (default scene + 1 sphere) %dx%d depth %d, %d frames: kernel us median %.2f min %.2f max %.2f | lit px %d | %s"
          % (W, H, DEPTH, frames, float(np.median(us)), min(us), max(us), lit, os.environ.get("RM_LIB_PATH", "this tree's library")))


if __name__ == "__main__":
    main()
