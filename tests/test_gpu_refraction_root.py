"""GPU: the refraction's root in the checked tile body (rm_trace.inc refract_ray: sqrt_discriminant, the compiler's
iteration without its scaling, the select for 0 kept) gives __builtin_sqrt's bits for everything a cos_theta_2 can be.
cos_theta_2 = 1 - x with x >= 0, so a value that is not zero is a multiple of 2^-53 up to 1: every such multiple near
zero and near 1, the powers of two and the all-ones significands of every binade between, and 10^6 seeded values are put
through the probe (rmi_numerics_probe's bit for the discriminant's root).  Frames: views that refract a great deal -- the
demo scene from inside its glass sphere, a floor of index 0.7 whose rays towards the horizon pass the critical angle --
are bit-equal with RM_CHECKED_NUMERICS=0, and no tile is rendered again."""
import numpy as np
import pytest

import test_gpu_child_fate as fate
import test_gpu_dead_children as scenes
from test_gpu_checked_numerics import THC_DIFF, both, pair, probe   # noqa: F401  (`pair`: the module's fixture)

pytestmark = pytest.mark.gpu

U = 2. ** -53


def check(pkg, x, label):
    x = np.ascontiguousarray(x, dtype=np.float64)
    bad = (probe(pkg, x) & THC_DIFF) != 0
    assert not bad.any(), "%s: %d arguments differ from __builtin_sqrt, first %r" % (label, int(bad.sum()), x[bad][0].hex())
    return x.size


def test_every_small_multiple_of_the_unit(pkg):
    k = np.arange(0, 1 << 16, dtype=np.float64)
    n = check(pkg, k * U, "k 2^-53") + check(pkg, 1. - k * U, "1 - k 2^-53") + check(pkg, [0., -0., 1., U, 2. * U], "ends")
    print("multiples of 2^-53: %d arguments, all bit-equal" % n)


def test_hard_significands_between_the_unit_and_one(pkg):
    sig = np.array([0, 1, 2, 3, (1 << 52) - 1, (1 << 52) - 2, (1 << 52) - 3, (1 << 52) - 4], dtype=np.uint64)
    e = np.arange(1023 - 53, 1023, dtype=np.uint64)
    x = ((e[:, None] << np.uint64(52)) | sig[None, :]).view(np.float64).ravel()
    x = x[(x >= U) & (x <= 1.)]
    s = ((np.arange(1023 - 27, 1023, dtype=np.uint64)[:, None] << np.uint64(52)) | sig[None, :]).view(np.float64).ravel().astype(np.longdouble)
    sq = (s * s).astype(np.float64)                                   # arguments whose root has those significands
    near = np.concatenate([sq, np.nextafter(sq, 0.), np.nextafter(sq, np.inf)])
    near = near[(near >= U) & (near <= 1.)]
    print("hard significands: %d arguments, all bit-equal" % (check(pkg, x, "significands") + check(pkg, near, "roots")))


def test_random_cos_theta_2(pkg):
    rng = np.random.default_rng(0xC052)
    x = np.concatenate([1. - rng.uniform(0., 1., 500_000), 2. ** rng.uniform(-53., 0., 500_000)])
    x = x[x > 0.]
    print("random: %d arguments, all bit-equal" % check(pkg, x, "random"))
    assert x.size >= 999_000


@pytest.mark.parametrize("name", ["inside_blue_d5", "thin_from_above_d5", "thin_from_below_d5", "above_d5"])
def test_refracting_views_bit_equal_and_nothing_redone(pkg, O, pair, name):
    what, depth, _ = fate.CASES[name]
    scene, _ = scenes.build(pkg, O, what)
    frame, redone, exact = both(pair, scene, fate.W, fate.H, depth, camera=what["camera"], label=name)
    assert frame.any() and redone == 0 and not exact
