"""CPU pins of the variant matrix (tests/variant_matrix.py), the premises of tests/test_gpu_variant_matrix.py and
tests/test_gpu_structured_rays.py, by the host-only scene image and the oracle alone:

1. every cell's scene image carries the hierarchies and the integer_exponents verdict the cell claims, and its depth lies on
   the side of the stack rule it claims -- by the rule as written here and by the library's own (rmi_shading_launch, asked
   with the image's header, verdict and the depth): a recipe that drifts into another kernel fails here;
2. the oracle tells the variants apart: with 12.5 replaced by 12, and one level less deep, more than 1e-6 changes in some
   channel on at least 5 % of the rays and of the pixels (the shares are printed);
3. some ray of the list holds exactly max_depth - 1 live siblings at once (cast_ray's tree replayed for 64 rays);
4. the refine threshold refines a proper subset with no contrast near it, and no select decision of a converging cell is close;
   the light the diffuse bounce brings back tells the depths and the exponents apart by itself, with no bounce ray on a boundary;
5. the structured rays hold the exact incidences they are there for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import antialias_reference as AR
import bounce_reference as BR
import converge_reference as CR
import progressive_reference as PR
import radiance_reference as RR
import ranged_reference
import soft_reference as SR
import test_gpu_query as GQ
import test_launch_plan as LP
import test_scene_image as SI
import variant_matrix as VM


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_variant_matrix"))


@pytest.fixture(scope="module")
def matrix(pkg, O, orc):
    return VM.Matrix(pkg, O, orc)


@pytest.fixture(scope="module")
def batch(O, entry, tmp_path_factory):
    d = tmp_path_factory.mktemp("orc_batch_structured")
    src, so = d / "orc_batch.c", d / "orc_batch.so"
    src.write_text(GQ.BATCH_C)
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-shared", "-fPIC",
                           "-I", os.path.join(entry.ROOT, "oracle"), str(src), "-o", str(so)])
    return GQ.OracleBatch(O, C.CDLL(str(so)))


# ---------------------------------------------------------------- 1. the launcher's facts
@pytest.mark.parametrize("cell", VM.CELLS, ids=VM.cell_id)
def test_a_cell_takes_the_kernel_it_claims(pkg, matrix, cell):
    bvh, generic, depth = cell
    handle = matrix.pair(bvh, generic)[0].flatten()
    st, img = SI.scene_image(pkg, handle.desc(), 1, 1)
    assert st == 0
    spheres, triangles, integer, shallow = VM.claims(cell)
    assert (img["H"]["off_bvh_spheres"] != 0) == spheres and (img["H"]["off_bvh_triangles"] != 0) == triangles, img["H"]
    assert bool(img["verdicts"][1]) == integer
    assert (depth <= 5) == shallow and depth in (5, 6)                 # the two sides of `max_depth <= 5u ? 4 : 32`
    # ... and the library says so itself: the variant its launchers take for this header, verdict and depth
    header = [img["H"][name] for name in SI.HEADER_FIELDS]
    assert LP.shading_variant(pkg, header, bool(img["verdicts"][1]), depth) == (spheres or triangles, 1 if integer else 0, 4 if shallow else 32)
    assert img["H"]["n_lights"] == len(VM.LIGHTS) == len(VM.RADII)
    # the exponents the integer cells keep at the ends of the binary powering
    exponents = {m["specular_exponent"] for m in VM.materials(generic).values()}
    assert {0., 1000.} <= exponents and ({12.5, 0.5} <= exponents) == generic
    assert len(matrix.o) == VM.N_RAYS and VM.N_RAYS % 64 and (VM.W * VM.H) % (64 // VM.LENS_SAMPLES)


# ---------------------------------------------------------------- 2. resolving power
@pytest.mark.parametrize("cell", VM.CELLS, ids=VM.cell_id)
def test_the_oracle_tells_the_variants_apart(matrix, cell):
    bvh, generic, depth = cell
    for what, answers in (("rays", matrix.rays), ("pixels", matrix.pixels)):
        true = answers(bvh, generic, depth)
        assert np.isfinite(true).all()
        shallower = VM.told_apart(true, answers(bvh, generic, depth - 1))
        print("%s, %s: depth %d against %d differs on %.1f %%" % (VM.cell_id(cell), what, depth, depth - 1, 100. * shallower))
        assert shallower >= VM.SHARE
        if generic:
            rounded = VM.told_apart(true, answers(bvh, generic, depth, half=12.))
            print("%s, %s: exponent 12.5 against 12 differs on %.1f %%" % (VM.cell_id(cell), what, 100. * rounded))
            assert rounded >= VM.SHARE
        # some go into the sky (exactly +0) and most do not
        gone = ~(true != 0.).any(axis=1)
        assert 0.02 < gone.mean() < 0.5, gone.mean()
    if bvh != "flat":                                                  # what makes the hierarchy is seen
        flat = matrix.rays("flat", generic, depth)
        assert VM.told_apart(matrix.rays(bvh, generic, depth), flat) >= VM.SHARE


# ---------------------------------------------------------------- 3. depth of parking
@pytest.mark.parametrize("cell", VM.CELLS, ids=VM.cell_id)
def test_a_ray_parks_max_depth_less_one_siblings(O, matrix, cell):
    bvh, generic, depth = cell
    oscene = matrix.pair(bvh, generic)[1]
    k = VM.N_RAYS // 4                                                 # (behind the random rays and the sky's)
    parked = np.array([VM.parked_at_once(O, oscene, matrix.o[i], matrix.d[i], depth) for i in range(k, k + 64)])
    print("%s: live siblings at once over 64 rays: %s" % (VM.cell_id(cell), np.bincount(parked, minlength=depth).tolist()))
    assert parked.max() == depth - 1 and (parked == depth - 1).sum() >= 8
    # ... and under the primary rays of the frame's middle
    d = RR.sample_directions(np.array([[16., 16.], [15., 17.], [17., 14.]]), matrix.orc.renderer(VM.W, VM.H))
    assert max(VM.parked_at_once(O, oscene, VM.EYE, v, depth) for v in matrix.orc.normalized(d)) == depth - 1


# ---------------------------------------------------------------- 4. decisions with room
@pytest.mark.parametrize("cell", VM.CELLS, ids=VM.cell_id)
def test_the_refine_threshold_decides_with_room(matrix, cell):
    bvh, generic, depth = cell
    frame = matrix.pixels(bvh, generic, depth).reshape(VM.H, VM.W, 3)
    refined = int(AR.mask(frame, VM.H, VM.REFINE_THRESHOLD).sum())
    near = AR.nearest_to(frame, VM.H, VM.REFINE_THRESHOLD)
    print("%s: %d of %d pixels refined, nearest contrast %.3e off the threshold" % (VM.cell_id(cell), refined, VM.W * VM.H, near))
    assert 64 < refined < VM.W * VM.H - 64 and near > AR.MARGIN


@pytest.fixture(scope="module")
def Y(pkg, O, orc):
    return CR.Yardstick(pkg, O, orc)


@pytest.mark.parametrize("offsets", [False, True], ids=["stored", "offsets"])
@pytest.mark.parametrize("cell", VM.CELLS, ids=VM.cell_id)
def test_no_select_decision_of_a_converging_cell_is_close(matrix, Y, cell, offsets):
    bvh, generic, depth = cell
    ns, tol, lo, hi = VM.CONVERGE
    name = VM.register(Y, matrix.name(bvh, generic), matrix.pair(bvh, generic))
    s = Y.samples(name, VM.W, VM.H, depth, VM.APERTURE, VM.FOCUS, hi, VM.RADII if offsets else None)
    recs, nearest = CR.run(s, VM.W, VM.H, ns, tol, lo, hi)             # (asserts every free decision's margin)
    counts = recs[-1][1].n
    print("%s, %s lights: %d passes, %d samples cast, counts %d .. %d, nearest decision %.3g x its margin"
          % (VM.cell_id(cell), "offset" if offsets else "stored", len(recs), sum(int(l.sum()) for l, _ in recs) * ns,
             counts.min(), counts.max(), nearest))
    assert nearest > 1. and not recs[-1][0].any()
    assert counts.min() == lo and counts.max() == hi and len(np.unique(counts)) >= 4     # some settle at once, some run into the cap
    listed = [int(l.sum()) for l, _ in recs]
    assert any(0 < n < VM.W * VM.H and n % 16 for n in listed)         # a list that fills no whole number of waves


# ---------------------------------------------------------------- 4b. the bounce cells
@pytest.fixture(scope="module")
def B(pkg, O, entry, orc, tmp_path_factory):
    return BR.Yardstick(pkg, O, orc, BR.compile_helper(O, entry, tmp_path_factory.mktemp("orb_variant_matrix")))


def bounce_share(B, matrix, bvh, generic, depth, half=VM.HALF):
    """What the bounce adds to the cell's frame (tests/test_gpu_variant_matrix.py test_bounce's inputs): the yardstick's mean at
    strength 1 less its mean at strength 0, [pixel][3] -> (the share, the scene's name in B)."""
    n = VM.BOUNCE_ROWS
    name = VM.register(B, matrix.name(bvh, generic) + ("" if half == VM.HALF else "-%g" % half), matrix.pair(bvh, generic, half))
    table, offsets = PR.lens_sequence(VM.BOUNCE_FIRST, n), SR.light_sequence(VM.BOUNCE_FIRST, n, VM.RADII)
    bounce = BR.bounce_sequence(VM.BOUNCE_FIRST, n)
    lit, plain = (B.bounce(name, VM.W, VM.H, depth, VM.APERTURE, VM.FOCUS, table, offsets, bounce, strength, (n,))[1] for strength in (1., 0.))
    return (lit - plain).reshape(-1, 3), name


@pytest.mark.parametrize("cell", VM.CELLS, ids=VM.cell_id)
def test_the_bounce_share_tells_the_variants_apart(O, matrix, B, cell):
    """The bounce launchers pick their instantiation as the others do (test_a_cell_takes_the_kernel_it_claims asks the
    library's own rule).  Here: the light the bounce brings back -- not the frame underneath it -- depends on the depth and, in
    the generic cells, on the exponent, on the committed numbers of pixels; and no sample's bounce ray lies on a hit / miss
    boundary."""
    bvh, generic, depth = cell
    share, name = bounce_share(B, matrix, bvh, generic, depth)
    differ = lambda a, b: int((np.abs(a - b) > VM.RESOLVE).any(axis=1).sum())
    lit, shallower = differ(share, 0.), differ(share, bounce_share(B, matrix, bvh, generic, depth - 1)[0])
    rounded = differ(share, bounce_share(B, matrix, bvh, generic, depth, 12.)[0]) if generic else None
    print("%s bounce share: %d pixels, depth %d against %d on %d, exponent 12.5 against 12 on %s; more than 0.05 on %d" % (
        VM.cell_id(cell), lit, depth, depth - 1, shallower, rounded, int((np.abs(share) > 0.05).any(axis=1).sum())))
    want = VM.BOUNCE_SHARE[bvh]
    assert lit == want[0] >= 50 and shallower == want[depth - 4] >= 1
    assert not generic or rounded == want[3] >= 10
    assert (share >= 0.).all()                                         # light is only added
    n = VM.BOUNCE_ROWS
    table, offsets = PR.lens_sequence(VM.BOUNCE_FIRST, n), SR.light_sequence(VM.BOUNCE_FIRST, n, VM.RADII)
    assert BR.boundary_rays(O, B.orb, B.scene(name)[1], VM.EYE, None, VM.W, VM.H, depth, VM.APERTURE, VM.FOCUS, table, offsets,
                            BR.bounce_sequence(VM.BOUNCE_FIRST, n), 1.) == 0
    c = B.counters(name, VM.W, VM.H, depth, VM.APERTURE, VM.FOCUS, table, offsets, BR.bounce_sequence(VM.BOUNCE_FIRST, n), 1.)
    assert c["bouncing"] > 500 and c["below"] > 10, c                 # (spheres in front of the panes: both halves of the basis)


# ---------------------------------------------------------------- 5. the structured rays
def test_the_structured_rays_hold_the_incidences_they_are_there_for(pkg, O, batch):
    scene, oscene = GQ.build_pair(pkg, O, VM.lattice_shapes())
    handle = scene.flatten()
    desc = handle.desc()
    st, img = SI.scene_image(pkg, desc, 1, 1)
    assert st == 0 and img["H"]["off_bvh_spheres"] and img["H"]["off_bvh_triangles"]
    assert (img["H"]["n_spheres"], img["H"]["n_triangles"]) == (65, 16)
    ref = ranged_reference.Scene(desc)
    for shift in (0., 1e-160):
        o, d = VM.structured_rays(shift)
        assert np.isfinite(o).all() and np.isfinite(d).all() and np.abs((d * d).sum(axis=1) - 1.).max() < 1e-4
        zero = (d == 0.).any(axis=1)
        assert zero.all() if not shift else (np.abs(d) == shift).any(axis=1).all()
        tangent, tie, hit, shape = VM.incidences(ref, o, d)
        # the numpy restatement is the oracle's: decisions and shapes
        o_hit, o_shape, _, _ = batch.closest(oscene, o, d)
        assert np.array_equal(o_hit.astype(bool), hit) and np.array_equal(o_shape[hit], shape[hit])
        lo, hi = GQ.bounds_of(desc)
        outside, centre = ((o < lo) | (o > hi)).any(axis=1), (o[:, None, :] == np.array(VM.LATTICE)[None]).all(axis=2).any(axis=1)
        inside = (((o[:, None, :] - np.array(VM.LATTICE)[None]) ** 2).sum(axis=2) < 1.).any(axis=1)
        in_plane = np.isin(o[:, 2], (-12., -2.5)) & (np.abs(d[:, 2]) <= shift)
        signs = np.signbit(d[zero & (np.abs(d) == 0.).any(axis=1)]).any() if not shift else True
        print("structured rays, shift %g: %d rays, %d hit, %d exactly tangent, %d exact ties (%d not with the sphere listed twice), "
              "%d from outside the bounds, %d from a centre, %d from inside a sphere, %d in a triangle's plane"
              % (shift, len(o), int(hit.sum()), int(tangent.sum()), int(tie.sum()), int((tie & (shape != 0)).sum()), int(outside.sum()),
                 int(centre.sum()), int(inside.sum()), int(in_plane.sum())))
        assert signs and tangent.sum() >= 50 and (tie & (shape != 0)).sum() >= 50
        assert (hit & zero).sum() >= 200 if not shift else hit.sum() >= 200
        assert (tie & (shape == 0)).sum() >= 10                        # the sphere listed twice is met
        assert outside.sum() >= 100 and centre.sum() >= 48 and inside.sum() > centre.sum() and in_plane.sum() >= 100
        assert hit.mean() < 0.9                                        # ... and misses are among them
