"""The render matrix on the GPU (-m gpu): every instantiation of rm_render_static (csrc/rm_kernels.hip), 368 kernels, renders
a frame whose ray trees fill its per-lane stack, against the oracle.  The recipes are tests/render_matrix.py's; that a cell
takes the kernel it claims, that the stacks fill and that the oracle alone tells the variants apart is pinned on the CPU by
tests/test_render_matrix.py.

A case is a row (flavour, camera, group, edges, order) and loops over the seven depths and the two powerings: 14 launches
through rm_render_device into a caller-owned buffer that holds a sentinel beforehand.  Before each launch rm_kernel_name
must name the instantiation the cell claims.  Strict flavour: every channel of every pixel within TIGHT = 1e-9 of the
oracle.  Fast flavour: the rule of tests/tie_reference.py's compare_fast -- the same bound but at certified ties, and these
frames name none: no pixel may differ.  Two launches that differ only in a knob no answer may depend on (the dispatch order, the cull's edge
test, the tile-level feedback), within one flavour and camera, must be equal bit for bit.  The contexts are made under the
rows' environments (the knobs are read at rm_init), each once, in this one process."""
import os
import time

import numpy as np
import pytest

import radiance_reference as RR
import render_matrix as RM
import test_gpu_parity as GP
import tie_reference as TR

pytestmark = pytest.mark.gpu

TIGHT = GP.TIGHT
SENTINEL = -1.
CLOCK = {}                           # "t0": when the module's first context was asked for
NAMES = set()                        # the kernel names met, over the module
FIRST = {}                           # (flavour, camera, scene, kernel group but for the feedback, depth, generic) -> the first frame
WORST = {}                           # (group, flavour) -> [largest deviation among the pixels held to the bound, tie pixels at the most]


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_gpu_render_matrix"))


@pytest.fixture(scope="module")
def frames(pkg, O, orc):
    return RM.Frames(pkg, O, orc)


@pytest.fixture(scope="module")
def contexts(pkg):
    """contexts(env) -> the context made under exactly these knobs of RM.KNOB_NAMES, made once."""
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    made = {}
    CLOCK["t0"] = time.time()

    def get(env):
        key = tuple(sorted(env.items()))
        if key not in made:
            before = {k: os.environ.get(k) for k in RM.KNOB_NAMES}
            for k in RM.KNOB_NAMES:
                os.environ.pop(k, None)
            os.environ.update(env)
            try:
                made[key] = pkg.backend.Context(0)
            finally:
                for k, v in before.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
        return made[key]

    yield get
    for c in made.values():
        c.close()


def parse(name):
    """rm_kernel_name's text -> ((fast, stack, pow_mode, staged, bvh, cull, edges, order, feedback), oriented), the template
    arguments taken apart as test_config_c5_synthetic_bands does."""
    space = name.split("::")[0]
    targs = [x.strip() for x in name.split("<", 1)[1].rstrip(">").split(",")]
    assert space in ("rmdev_strict", "rmdev_fast", "rmdev_strict_o", "rmdev_fast_o") and len(targs) == 10 and targs[2:4] == ["1", "1"], name
    flags = [{"true": 1, "false": 0}[t] for t in targs[4:]]
    return (int(space.startswith("rmdev_fast")), int(targs[0]), int(targs[1])) + tuple(flags), space.endswith("_o")


def device_frame(ctx, p):
    """One frame into a device buffer of the caller's that holds SENTINEL everywhere beforehand."""
    import torch
    dev = torch.full((RM.H, RM.W, 3), SENTINEL, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.render_device(p, dev.data_ptr())
    torch.cuda.synchronize()
    return dev.cpu().numpy()


def compare(gpu, ref, fast, label, tie=None):
    """-> (largest deviation among the pixels held to the bound, differing pixels); fast: tests/tie_reference.py compare_fast,
    the differing pixels certified by `tie` (a tie_reference.Tie; None: none may differ)."""
    d = np.abs(gpu - ref)
    if fast:
        return TR.compare_fast(gpu, ref, TIGHT, tie, label)
    worst = float(d.max())
    assert worst < TIGHT, "%s: max |delta| %.3e (channels above 1e-12: %d)" % (label, worst, int((d > 1e-12).sum()))
    return worst, 0


def run_row(pkg, frames, ctx, row, name, depths, powerings=(False, True)):
    flavour, camera, group, edges, order = row
    fast = flavour == "fast"
    for generic in powerings:
        ctx.upload(frames.pair(name, generic)[0].flatten())
        ctx.set_camera(RM.EYE)
        ctx.orient(RM.basis_of(camera))
        for depth in depths:
            label = "%s %s depth %d %s" % (RM.row_id(row), name, depth, "generic" if generic else "integer")
            p = pkg.backend.make_params(RM.FOV, float(RM.H), float(RM.W), depth)
            p.flags = GP.RM_FLAG_FAST_FP if fast else 0
            claimed = RM.claim(row, depth, generic)
            named = ctx.kernel_name(p)
            assert parse(named) == claimed and named == RM.kernel_text(*claimed), (label, named)
            NAMES.add(named)
            got = device_frame(ctx, p)
            assert not (got == SENTINEL).any(), "%s: %d pixels never written" % (label, int((got == SENTINEL).all(axis=2).sum()))
            worst, ties = compare(got, frames.frame(name, camera, depth, generic), fast, label)
            w = WORST.setdefault((name if name in ("mesh", "staged-12") else "g%d" % group, flavour), [0., 0])
            w[0], w[1] = max(w[0], worst), max(w[1], ties)
            # the knobs no answer may depend on: the first launch of these facts gave this very frame
            key = (flavour, camera, name, min(group, 3), depth, generic)
            if key in FIRST:
                assert np.array_equal(got, FIRST[key][1]), "%s differs from %s" % (label, FIRST[key][0])
            else:
                FIRST[key] = (label, got)


@pytest.mark.parametrize("row", RM.rows(), ids=RM.row_id)
def test_row(pkg, frames, contexts, row):
    flavour, camera, group, edges, order = row
    run_row(pkg, frames, contexts(RM.knobs(group, edges, order)), row, RM.SCENE_OF_GROUP[group], RM.DEPTHS)


@pytest.mark.parametrize("camera", RM.CAMERAS)
@pytest.mark.parametrize("flavour", RM.FLAVOURS)
def test_the_triangle_hierarchy_meets_a_full_stack(pkg, frames, contexts, flavour, camera):
    """Group 3's extra row: the 14-triangle mesh in place of the 20 small spheres."""
    row = (flavour, camera, 3, True, True)
    run_row(pkg, frames, contexts(RM.knobs(3, True, True)), row, "mesh", RM.DEPTHS)


@pytest.mark.parametrize("edges", [True, False], ids=["edges", "noedges"])
@pytest.mark.parametrize("camera", RM.CAMERAS)
@pytest.mark.parametrize("flavour", RM.FLAVOURS)
def test_twelve_primitives_in_the_staged_budget(pkg, frames, contexts, flavour, camera, edges):
    """Group 1's extra row: what takes its kernels with no RM_CULL_MIN set -- five panes and seven spheres; stack 4 fills."""
    row = (flavour, camera, 1, edges, True)
    run_row(pkg, frames, contexts(RM.knobs(2, edges, True)), row, "staged-12", RM.DEPTHS)


def test_every_instantiation_was_launched():
    """Last: the names collected over the module are the 368 kernels of the table."""
    for (group, flavour), (worst, ties) in sorted(WORST.items()):
        print("%s %s: max |delta| %.3e among the pixels held to the bound, %d tie pixels a frame at the most" % (group, flavour, worst, ties))
    print("knob pairs compared bit for bit: %d frames stand for %d launches" % (len(FIRST), len(RM.cells()) + 12 * 14))
    print("the module took %.1f s up to here" % (time.time() - CLOCK["t0"]))
    assert NAMES == {RM.kernel_text(*t) for t in RM.table()} and len(NAMES) == 368
