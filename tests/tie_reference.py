"""The tie certificate of the fast flavour (RM_FLAG_FAST_FP), and the one rule every fast frame of the suite is held to.

The fast flavour may differ from the reference only where the reference itself cannot decide.  What "cannot decide" means is
fixed here, on the oracle alone (no GPU, no product code):

  the family of a primary ray   its unit direction d as orc_normalized returns it (member 0), and d with the magnitudes of its
                                non-zero components moved by +-1, +-4 and +-16 ulps of the binary64 representation, over the 26
                                sign patterns: 78 neighbours.  A component that is exactly 0 stays 0 -- the fast flavour maps
                                exact zeros to exact zeros, so a decision on a symmetry axis is no tie.  (16 ulps move d.d by
                                1e-14 at the most: inside orc_cast_ray's |d.d - 1| < 1e-4.)
  outcomes                      orc_cast_ray along every member: (N, 79, 3) colours
  unstable                      a pixel one of whose members differs from member 0 by TIGHT or more on a channel
  certified                     a pixel that is unstable AND whose GPU colour is within TIGHT, on every channel, of a member's

compare_fast is the rule: every pixel outside the differing set within TIGHT of the reference, the differing set no larger than
FAST_TIE_PIXELS, and every differing pixel certified -- by the `tie=` the call site passes; a call site that passes none admits
no differing pixel at all.  tests/test_tie_reference.py pins member 0 to orc_render, freezes where unstable pixels are, and
shows that the certificate has teeth; tests/test_gpu_fast_ties.py renders the frames where ties exist."""
import atexit
import shutil
import tempfile
from pathlib import Path

import numpy as np

import radiance_reference as RR
import workloads

TIGHT = RR.TIGHT
# the recipe tests/test_radiance_abi.py pins to orc_render bit for bit (test_casting_the_sample_directions_is_orc_render):
# cast(eye, orc_normalized(direction), scene, BACKGROUND, 1, max_depth)
BACKGROUND = RR.BACKGROUND
ULPS = (1, 4, 16)
SIGNS = np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)], dtype=np.int64)
MEMBERS = 1 + len(ULPS) * len(SIGNS)                                 # 79
MAX_UNSTABLE_SHARE = 0.005           # a frame a GPU test certifies on has at most this share of unstable pixels: a condition
# the differing pixels a fast frame may have at the most -- all of them certified
FAST_TIE_PIXELS = lambda n_px: max(8, n_px // 50000)

_ORC = {}


def oracle_radiance():
    """The OracleRadiance of this process (radiance_reference.compile_helper), compiled once into a directory of its own."""
    if "orc" not in _ORC:
        import __graft_entry__ as G
        d = tempfile.mkdtemp(prefix="orc_tie_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        _ORC["orc"] = RR.compile_helper(G.load_oracle(), G, Path(d))
    return _ORC["orc"]


# ---------------------------------------------------------------- the family
def family(d):
    """(N, 3) unit directions -> (N, 79, 3): member 0 is d; member 1 + 26 * i + j moves the magnitude of every non-zero
    component c by SIGNS[j][c] * ULPS[i] ulps.  Exact zeros stay zeros, and no component becomes one."""
    d = np.ascontiguousarray(d, dtype=np.float64).reshape(-1, 3)
    bits = d.view(np.uint64)
    sign, mag = bits & np.uint64(1 << 63), (bits & np.uint64((1 << 63) - 1)).astype(np.int64)
    out = np.empty((d.shape[0], MEMBERS, 3))
    out[:, 0] = d
    for i, k in enumerate(ULPS):
        moved = np.maximum(mag[:, None, :] + k * SIGNS[None, :, :], 1)                      # (N, 26, 3)
        moved = np.where(mag[:, None, :] == 0, 0, moved)
        out[:, 1 + 26 * i:1 + 26 * (i + 1)] = (moved.astype(np.uint64) | sign[:, None, :]).view(np.float64)
    return out


def outcomes(oscene, eye, dirs, depth, orc=None):
    """orc_cast_ray from `eye` ((3,) or (N, 3)) along every member of the families of the unit directions `dirs` -> (N, 79, 3)."""
    orc = orc or oracle_radiance()
    fam = family(dirs)
    n = fam.shape[0]
    o = np.broadcast_to(np.asarray(eye, dtype=np.float64).reshape(-1, 1, 3), fam.shape)
    return orc.cast(oscene, o.reshape(-1, 3), fam.reshape(-1, 3), depth, background=BACKGROUND).reshape(n, MEMBERS, 3)


def unstable(out):
    """(N, 79, 3) outcomes -> (N,) bool: a member differs from member 0 by TIGHT or more on a channel."""
    return (np.abs(out[:, 1:] - out[:, :1]) >= TIGHT).any(axis=(1, 2))


# ---------------------------------------------------------------- primary rays
class Tie:
    """What the certificate needs of a call site: the oracle's scene, the Renderer's width and height (backproject's, which
    need not be the frame's), the depth cap, the eye (the scene's camera unless given), the field of view, the basis ((right,
    up, forward) as tuples, None: the fixed view) and, where the compared array is a band of the frame, `rows`: the frame row
    of each of its rows."""

    def __init__(self, oscene, w, h, depth, eye=None, fov=workloads.FOV, basis=None, rows=None, orc=None):
        self.oscene, self.w, self.h, self.depth, self.fov, self.basis = oscene, int(w), int(h), int(depth), fov, basis
        self.eye = tuple(oscene.c.camera.tup()) if eye is None else tuple(float(c) for c in eye)
        self.rows = None if rows is None else np.asarray(rows, dtype=np.int64)
        self.orc = orc or oracle_radiance()

    def directions(self, pixels, cols):
        """Unit primary directions of the pixels (flat indices into an array `cols` wide): backproject's two numbers per
        pixel, through the basis where there is one (radiance_reference.sample_directions -- tests/test_gpu_camera.py's
        OracleCamera.directions operation for operation), normalised by orc_normalized."""
        pixels = np.asarray(pixels, dtype=np.int64)
        y, x = pixels // cols, pixels % cols
        if self.rows is not None:
            y = self.rows[y]
        xy = np.stack([x, y], axis=1).astype(np.float64)
        return self.orc.normalized(RR.sample_directions(xy, self.orc.renderer(self.w, self.h, self.fov), self.basis))

    def outcomes(self, pixels, cols):
        return outcomes(self.oscene, self.eye, self.directions(pixels, cols), self.depth, self.orc)


def frame_map(tie, cols=None, n_rows=None):
    """-> (the unstable mask (n_rows, cols), the outcomes (n_rows, cols, 79, 3)) of a whole small frame: by default the rows
    the renderer writes, [0, h - h % 32), or the rows of tie.rows."""
    cols = tie.w if cols is None else cols
    if n_rows is None:
        n_rows = len(tie.rows) if tie.rows is not None else tie.h - tie.h % 32
    out = tie.outcomes(np.arange(n_rows * cols), cols)
    return unstable(out).reshape(n_rows, cols), out.reshape(n_rows, cols, MEMBERS, 3)


# ---------------------------------------------------------------- the certificate
def certify(gpu, ref, pixels, tie):
    """gpu, ref: (rows, cols, 3); pixels: flat indices of the differing ones -> (certified (n,) bool, outcomes (n, 79, 3)).
    Member 0 must be the reference's own colour bit for bit, or the call site's recipe is not the reference's."""
    cols = gpu.shape[1]
    pixels = np.asarray(pixels, dtype=np.int64)
    out = tie.outcomes(pixels, cols)
    want = np.ascontiguousarray(ref.reshape(-1, 3)[pixels])
    assert out[:, 0].tobytes() == want.tobytes(), "tie=: member 0 is not the reference's colour at %d of %d pixels" % (
        int((out[:, 0] != want).any(axis=1).sum()), len(pixels))
    got = gpu.reshape(-1, 3)[pixels]
    with np.errstate(invalid="ignore"):
        shown = (np.abs(out - got[:, None, :]) < TIGHT).all(axis=2).any(axis=1)              # (a NaN is within nothing)
    return unstable(out) & shown, out


def compare_fast(gpu, ref, tol=TIGHT, tie=None, label=None):
    """The fast flavour's rule -> (largest deviation among the pixels held to the bound, differing pixels)."""
    if label is None:
        label = "frame" if tie is None else "%dx%d frame from %s, depth %d" % (tie.w, tie.h, tie.eye, tie.depth)
    d = np.abs(np.asarray(gpu) - ref).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        bad = ~(d.max(axis=1) < tol)                                 # (a NaN differs)
    n_bad, allowed, cols = int(bad.sum()), FAST_TIE_PIXELS(bad.size), gpu.shape[-2]
    where = [(int(i) % cols, int(i) // cols) for i in np.flatnonzero(bad)[:32]]
    assert n_bad <= allowed, "%s: %d pixels differ (the fast flavour may differ at %d certified ties): %s" % (label, n_bad, allowed, where)
    if n_bad:
        assert tie is not None, "%s: %d pixels differ and the call site names no ties: %s" % (label, n_bad, where)
        ok, out = certify(np.asarray(gpu).reshape(-1, cols, 3), np.asarray(ref).reshape(-1, cols, 3), np.flatnonzero(bad), tie)
        un = unstable(out)
        refused = [(int(i) % cols, int(i) // cols, "unstable" if u else "stable") for i, k, u in zip(np.flatnonzero(bad), ok, un) if not k]
        print("%s: fast flavour, %d differing pixels, %d certified" % (label, n_bad, int(ok.sum())))
        assert not refused, "%s: differing pixels without a certificate (stable: the oracle decides them; unstable: the colour is none of the family's): %s" % (
            label, refused[:32])
    return (float(d[~bad].max()) if (~bad).any() else 0.), n_bad
