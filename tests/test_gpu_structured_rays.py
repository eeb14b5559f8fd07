"""Structured rays for the hierarchy walks (-m gpu): axis-parallel and diagonal rays -- exact zeros of both signs in their
directions -- from an integer and half-integer lattice of origins at a lattice of touching unit spheres, a mesh of triangles
in two planes z = const and a sphere listed twice (tests/variant_matrix.py).  Both hierarchies are built, so the slab test's
reciprocal meets 0., -0. and, in the shifted set, +-1e-160; rays run through sphere centres, exactly tangent to spheres
(d2 == r2: the root of a zero discriminant), through the points where two spheres touch (exact ties, which go to the first in
list order) and in the triangles' planes.  tests/test_variant_matrix.py counts these incidences with the oracle alone.

rm_intersect_rays and rm_occluded_rays against the oracle's find_closest_intersect and intersect_shape_set, decisions exact and
points and normals within TIGHT = 1e-9; their ranged forms byte for byte over [0, inf] and, over finite ranges, against
tests/ranged_reference.py (decisions, shape, element and ray parameter exactly); rm_radiance_rays at depth 3 against
orc_cast_ray within TIGHT, apart from the rays that start on the very surface they hit (see there)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import radiance_reference as RR
import ranged_reference
import test_gpu_query as GQ
import test_gpu_ranged_queries as GRQ
import variant_matrix as VM

pytestmark = pytest.mark.gpu

TIGHT = GQ.TIGHT
SHIFTS = [0., 1e-160]
RANGES = [(0.3, 2.7), (1.1, 5.3), (0.05, 0.9), (3.3, np.inf)]             # no end at a distance the lattice makes


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batch(O, entry, tmp_path_factory):
    d = tmp_path_factory.mktemp("orc_batch_structured_gpu")
    src, so = d / "orc_batch.c", d / "orc_batch.so"
    src.write_text(GQ.BATCH_C)
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-shared", "-fPIC",
                           "-I", os.path.join(entry.ROOT, "oracle"), str(src), "-o", str(so)])
    return GQ.OracleBatch(O, C.CDLL(str(so)))


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_structured_gpu"))


class Lattice:
    def __init__(self, pkg, O):
        self.scene, self.oscene = GQ.build_pair(pkg, O, VM.lattice_shapes())
        self.handle = self.scene.flatten()
        self.desc = self.handle.desc()
        self.ref = ranged_reference.Scene(self.desc)
        self.rays = {shift: VM.structured_rays(shift) for shift in SHIFTS}


@pytest.fixture(scope="module")
def lattice(pkg, O):
    return Lattice(pkg, O)


@pytest.mark.parametrize("shift", SHIFTS)
def test_closest_hits_and_occlusion_match_the_oracle(ctx, batch, lattice, shift):
    ctx.upload(lattice.handle)
    o, d = lattice.rays[shift]
    label = "structured rays, shift %g" % shift
    g, worst = GQ.check_closest(batch, ctx, lattice.oscene, o, d, label=label)
    occ = GQ.check_occluded(batch, ctx, lattice.oscene, o, d, label=label)
    m = g["hit"] == 1
    assert np.array_equal(occ[m], np.ones(int(m.sum()), bool))
    assert not (g["shape"][m] == len(VM.LATTICE) + 1).any(), "the sphere listed twice won a tie against itself"
    assert (g["shape"][m] == 0).any() and (g["shape"][m] == len(VM.LATTICE)).any()      # the first sphere and the mesh are met
    print("%s: %d of %d hit, %d occluded, max |point / normal delta| %.3e" % (label, int(m.sum()), len(o), int(occ.sum()), worst))
    # the ranged forms over [0, inf]: byte for byte
    assert ctx.intersect(o, d, ranges=GRQ.FULL).tobytes() == g.tobytes()
    assert ctx.occluded(o, d, ranges=GRQ.FULL).tobytes() == occ.tobytes()


@pytest.mark.parametrize("shift", SHIFTS)
def test_finite_ranges_match_the_helper(ctx, lattice, shift):
    ctx.upload(lattice.handle)
    o, d = lattice.rays[shift]
    for r in RANGES:
        label = "structured rays, shift %g, range %s" % (shift, r)
        ref = lattice.ref.closest(o, d, r)
        ref_occ, near_occ = lattice.ref.occluded(o, d, r)
        keep = GRQ.kept(ref["near_end"] | near_occ, label)
        g, occ = ctx.intersect(o, d, ranges=r), ctx.occluded(o, d, ranges=r)
        assert np.array_equal(g["hit"][keep], ref["hit"][keep]), "%s: %d hit / miss decisions differ" % (label, int((g["hit"] != ref["hit"])[keep].sum()))
        assert np.array_equal(occ[keep], ref_occ[keep]), "%s: %d occlusion decisions differ" % (label, int((occ != ref_occ)[keep].sum()))
        m = keep & (ref["hit"] == 1)
        assert m.sum() > 500
        for f in ("shape", "element", "t"):
            assert np.array_equal(g[f][m], ref[f][m]), "%s: %d rays differ in %s" % (label, int((g[f][m] != ref[f][m]).sum()), f)
        assert np.abs(g["point"][m] - ref["point"][m]).max() < TIGHT and np.abs(g["normal"][m] - ref["normal"][m]).max() < TIGHT


@pytest.mark.parametrize("shift", SHIFTS)
def test_radiance_matches_the_oracle(ctx, orc, lattice, shift):
    ctx.upload(lattice.handle)
    o, d = lattice.rays[shift]
    got = ctx.radiance(o, d, max_depth=3)
    ref = orc.cast(lattice.oscene, o, d, 3)
    # A ray that starts on the surface it hits (t == 0: the point is the origin): the reference's dir_to_viewer,
    # normalize(origin - point), is the zero vector there and its specular term falls to 0.  The radiance step forms that
    # vector as the reference does ("radiance queries", Viewer direction), so these rays are held to the same
    # bound as all the others -- and are still counted apart, lit and finite.
    first = lattice.ref.closest(o, d, GRQ.FULL)
    at_origin = (first["hit"] == 1) & (first["t"] == 0.)
    delta = np.abs(got - ref).max(axis=1)
    gone = ~(ref != 0.).any(axis=1)
    print("structured rays, shift %g: radiance max |delta| %.3e over %d rays (%d lit), %.3e over the %d that start on the surface they hit"
          % (shift, delta[~at_origin].max(), int((~at_origin).sum()), int((~gone & ~at_origin).sum()), delta[at_origin].max(), int(at_origin.sum())))
    assert not np.isnan(got).any() and delta[~at_origin].max() < TIGHT, "%d rays differ" % int((delta[~at_origin] >= TIGHT).sum())
    assert (got[at_origin] >= 0.1).all() and at_origin.sum() < 0.1 * len(o)
    assert at_origin.sum() > 0 and delta[at_origin].max() < TIGHT, "%d rays that start on the surface they hit differ" % int((delta[at_origin] >= TIGHT).sum())
    assert gone.any() and (~gone & ~at_origin).sum() > 1000 and not got[gone].view(np.uint64).any()
