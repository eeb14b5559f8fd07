"""CPU pins of tests/hierarchy_reference.py, the premises of tests/test_gpu_hierarchy_walk.py, by the host-only scene image
and the oracle alone:

1. on the rays the suite already holds to the oracle (unit to rounding) the model's unpruned walk reaches every primitive
   the oracle names as the closest hit: the model and the boxes are sound;
2. the admitted-direction sets pass the host's check (|d.d - 1| < 1e-4 with d.d = (x x + y y) + z z), the numpy restatement
   used for the elements is the oracle's on them, and they have teeth: at d.d = 1 + 9e-5 the oracle's closest hit lies on a
   sphere the box walk never reaches on at least 32 rays of the 256 spheres and 16 of the variant matrix's 25, on none at
   |d.d - 1| <= 1e-6, and at 1 - 9e-5 at least 16 rays pass through the overlap of two spheres whose distances differ by
   less than 1e-4 relative (where the pruning distance of the one must not cut off the other);
3. the chain scenes are as deep as they claim -- spheres: more than the 24 levels of surface-area splits, at most the 60
   the builder allows; mesh: 16 or more over leaves of 2 --, whole groups of 64 consecutive rays of the query set and of
   the frame's primary rays park depth - 1 entries or more, and a depth-6 ray tree sees more than a depth-3 one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hierarchy_reference as HR
import radiance_reference as RR
import ranged_reference
import test_gpu_query as GQ
import variant_matrix as VM


@pytest.fixture(scope="module")
def batch(O, entry, tmp_path_factory):
    d = tmp_path_factory.mktemp("orc_batch_hierarchy")
    src, so = d / "orc_batch.c", d / "orc_batch.so"
    src.write_text(GQ.BATCH_C)
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-shared", "-fPIC",
                           "-I", os.path.join(entry.ROOT, "oracle"), str(src), "-o", str(so)])
    return GQ.OracleBatch(O, C.CDLL(str(so)))


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_hierarchy"))


def closest_primitives(batch, oscene, desc, img, o, d):
    """The oracle's closest hit of every ray as a device primitive id (-1: none): the element comes from the numpy
    restatement, which must agree with the oracle's own decision and shape on every ray."""
    ref = ranged_reference.Scene(desc).closest(o, d, (0., np.inf))
    hit, shape, _, _ = batch.closest(oscene, o, d)
    assert np.array_equal(ref["hit"], hit) and np.array_equal(ref["shape"][hit == 1] % 256, shape[hit == 1])
    return HR.pid_of(img, ref["shape"], ref["element"]), ref


# ---------------------------------------------------------------- 1. unit rays: the model is sound
@pytest.mark.parametrize("name", ["synthetic256", "cornell", "matrix-spheres", "matrix-mesh"])
def test_unit_rays_reach_what_the_oracle_hits(pkg, O, batch, name):
    scene, oscene = HR.scene_pair(pkg, O, name)
    desc, img = HR.image_of(pkg, scene)
    assert img["H"]["off_bvh_spheres"] or img["H"]["off_bvh_triangles"]
    o, d = HR.unit_rays(name, desc)
    assert np.abs(HR.length_squared(d) - 1.).max() < 1e-15
    pid, _ = closest_primitives(batch, oscene, desc, img, o, d)
    n = img["H"]["n_spheres"] + img["H"]["n_polygons"]
    walked = (pid >= 0) & ((pid < img["H"]["n_spheres"]) if img["H"]["off_bvh_spheres"] else (pid >= n))
    missed = HR.unreached(img, o, d, pid)
    print("%s: %d unit rays, %d closest hits on a primitive of a hierarchy, %d of them not reached" % (name, len(o), int(walked.sum()), int(missed.sum())))
    assert walked.sum() >= 1 and not missed.any()                      # (the matrix's rays mostly meet its panes first)
    # ... and every primitive of a hierarchy that the reference's rule lets the ray hit AT ALL, closest or not
    met = 0
    lo, hi = np.zeros(len(o)), np.full(len(o), np.inf)
    for kind, si, el, _, ok, _, _ in ranged_reference.Scene(desc)._accepted(o, d, lo, hi):
        if ok.any():
            p = np.full(int(ok.sum()), HR.pid_of(img, [si], [el])[0])
            lost = HR.unreached(img, o[ok], d[ok], p)
            assert not lost.any(), (kind, si, el)
            in_tree = (p[0] < img["H"]["n_spheres"]) if img["H"]["off_bvh_spheres"] else (p[0] >= n)
            met += int(ok.sum()) if in_tree else 0
    print("%s: %d incidences of a ray with a primitive of a hierarchy, all reached" % (name, met))
    assert met >= 32


# ---------------------------------------------------------------- 2. admitted directions: the sets have teeth
LEAST_UNREACHED = {"synthetic256": 32, "matrix-spheres": 16}


@pytest.mark.parametrize("name", HR.SCENES)
def test_admitted_directions_have_teeth(pkg, O, batch, name):
    scene, oscene = HR.scene_pair(pkg, O, name)
    desc, img = HR.image_of(pkg, scene)
    o, d, e, kind = HR.admitted_set(name, desc)
    dd = HR.length_squared(d)
    assert len(o) <= 20000 and np.isfinite(o).all() and (np.abs(dd - 1.) < HR.ADMITTED).all()
    assert kind[-1] == HR.QUERY and (kind[:-1] != HR.QUERY).all() and tuple(d[-1]) == HR.QUERY_TEST_RAY and not o[-1].any()
    for c in HR.CLASSES:                                               # every class is what it says, to the rounding of the stretch
        assert (e == c).sum() >= 1200 and np.abs(dd[e == c] - 1. - c).max() < 1e-15
    pid, ref = closest_primitives(batch, oscene, desc, img, o, d)
    missed = HR.unreached(img, o, d, pid)
    counts = {c: int(missed[e == c].sum()) for c in HR.CLASSES}
    print("%s: %d rays, %d hit; closest hit on a primitive the box walk never reaches, by d.d - 1: %s" % (name, len(o), int(ref["hit"].sum()), counts))
    assert 0.3 * len(o) < ref["hit"].sum() < len(o)
    assert all(counts[c] == 0 for c in HR.CLASSES if abs(c) <= 1e-6)
    assert counts[9e-5] >= LEAST_UNREACHED.get(name, 0)
    if name in LEAST_UNREACHED:                                        # the pruning case
        m = kind == HR.OVERLAP
        assert (e[m] == -9e-5).all()
        lo, hi = np.zeros(int(m.sum())), np.full(int(m.sum()), np.inf)
        ts = np.array([np.where(ok, t, np.inf) for _, _, _, _, ok, t, _ in ranged_reference.Scene(desc)._accepted(o[m], d[m], lo, hi)])
        ts.sort(axis=0)
        with np.errstate(invalid="ignore"):
            close = np.isfinite(ts[1]) & (ts[1] - ts[0] < 1e-4 * ts[0])
        print("%s: %d rays through an overlap, the two nearest distances within 1e-4 relative on %d" % (name, int(m.sum()), int(close.sum())))
        assert close.sum() >= 16


# ---------------------------------------------------------------- 3. the chain scenes are deep and the rays go deep
def frame_directions(pkg):
    p = pkg.backend.make_params(HR.CHAIN_FOV, float(HR.CHAIN_H), float(HR.CHAIN_W), 3)
    return ranged_reference.normalized(RR.sample_directions(RR.pixel_positions(HR.CHAIN_W, HR.CHAIN_H), p))[0]


@pytest.mark.parametrize("which", ["spheres", "mesh"])
def test_chain_scenes_are_deep(pkg, O, orc, which):
    scene, oscene = HR.chain_pair(pkg, O, which)
    desc, img = HR.image_of(pkg, scene)
    if which == "spheres":
        tree = HR.Tree(img, "spheres")
        assert 24 < tree.depth <= 60 and tree.leaf_size == 4 and not img["H"]["off_bvh_triangles"]
    else:
        tree = HR.Tree(img, "triangles")
        assert tree.depth >= 16 and tree.leaf_size == 2 and not img["H"]["off_bvh_spheres"]
    o, d = HR.chain_rays()
    dirs = frame_directions(pkg)
    rays, frame = tree.stack_height(o, d), tree.stack_height(np.zeros_like(dirs), dirs)
    print("%s chain: depth %d, %d nodes; stack heights of the query rays up to %d (%d whole groups of 64 at depth - 1 or more), of the "
          "frame's up to %d (%d whole groups)" % (which, tree.depth, len(tree.nodes), rays.max(), HR.whole_groups(rays, tree.depth - 1),
                                                  frame.max(), HR.whole_groups(frame, tree.depth - 1)))
    assert rays.max() == frame.max() == tree.depth
    assert HR.whole_groups(rays, tree.depth - 1) >= 1 and HR.whole_groups(frame, tree.depth - 1) >= 1
    # the tiles of the render kernels (8 x 8 pixels): some hold depth - 1 or more on every pixel too
    tiles = frame.reshape(HR.CHAIN_H // 8, 8, HR.CHAIN_W // 8, 8).min(axis=(1, 3))
    assert (tiles >= tree.depth - 1).any()
    # ... and the rays see many links, some none; six levels of glass show more than three
    ref = ranged_reference.Scene(desc).closest(o, d, (0., np.inf))
    seen = {(int(s), int(t)) for s, t in zip(ref["shape"][ref["hit"] == 1], ref["element"][ref["hit"] == 1])}
    assert len(seen) >= 20 and 0.3 < ref["hit"].mean() < 0.9
    o, d = HR.chain_rays(top=HR.CHAIN_SHADED_TOP)                      # the rays that are shaded
    assert HR.whole_groups(tree.stack_height(o, d), tree.depth - 1) >= 1
    deep, shallow = orc.cast(oscene, o, d, 6), orc.cast(oscene, o, d, 3)
    assert np.isfinite(deep).all() and VM.told_apart(deep, shallow) >= VM.SHARE
