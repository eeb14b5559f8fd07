"""CPU: the certificate behind the early fate of a refracted child (csrc/rm_trace.inc refract_fate / refract_ray,
render_tile).  The refracted direction's dot with the surface normal is -sqrt(cos_theta_2) without
the flip and +sqrt(cos_theta_2) with it, so from RM_FATE_COS2_MIN on (and for r up to RM_FATE_R_MAX) the kernels take the
side the child leaves into from `flip` alone and never form the ray.  Here the strict kernels' sequence is restated in
numpy float64 -- the reference's operation order, every operation rounded once, no fused multiply-add -- and the sign of
the COMPUTED dot is compared with the predicted one: over a million seeded cases with unit vectors as the kernels form
them (sqrt, then 1 / norm), both sides, indices from 1.0001 to 3; normals that are unit only to 1e-6, which is what the
upload admits for a flagged primitive; cases at and around the critical angle, cos_theta_2 from T / 4 to 4 T and down to
the smallest positive values there are; grazing incidence; normals along an axis."""
import os
import re

import numpy as np
import pytest

TRACE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rusty-marcher_amd", "csrc", "rm_trace.inc")


def _define(name):
    m = re.search(r"^#define %s (\S+)$" % name, open(TRACE).read(), re.M)
    assert m, "%s is not defined in rm_trace.inc" % name
    return float.fromhex(m.group(1)) if "x" in m.group(1) else float(m.group(1))


T = _define("RM_FATE_COS2_MIN")
R_MAX = _define("RM_FATE_R_MAX")


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]                  # geometry.rs:180-182


def normalized(v):
    norm = np.sqrt(dot(v, v))                                         # geometry.rs:104-109
    inv = 1. / norm
    return [v[0] * inv, v[1] * inv, v[2] * inv]


def refract(i, n, ri):
    """-> (flip, r, cos_theta_2, computed d . n, v . n of the direction before it is normalised) as refract_fate and
    refract_ray compute them, per case."""
    with np.errstate(invalid="ignore"):
        c0 = -dot(n, i)
        flip = c0 < 0.
        r = np.where(flip, ri, 1. / ri)
        c = np.where(flip, -c0, c0)
        cos2 = 1. - r * r * (1. - c * c)
        k = r * c - np.sqrt(cos2)
        ks = np.where(flip, -k, k)
        v = [i[0] * r + n[0] * ks, i[1] * r + n[1] * ks, i[2] * r + n[2] * ks]
        return flip, r, cos2, dot(normalized(v), n), dot(v, n)


def unit(rng, n):
    return normalized(list(rng.normal(size=(3, n))))


def tangent(rng, nrm):
    t = unit(rng, len(nrm[0]))
    h = dot(t, nrm)
    return normalized([t[0] - h * nrm[0], t[1] - h * nrm[1], t[2] - h * nrm[2]])


def random_cases(rng, n):
    return unit(rng, n), unit(rng, n), rng.uniform(1.0001, 3., n)


def loose_normal_cases(rng, n):
    """Normals whose length is 1 +- 1e-6 at the most: a flagged primitive's may be that far from unit."""
    i, nrm, ri = random_cases(rng, n)
    s = 1. + rng.choice([-1., 1.], n) * 1e-6 * rng.uniform(0., 1., n) ** 0.25 * (1. - 1e-9)
    return i, [nrm[0] * s, nrm[1] * s, nrm[2] * s], ri


def critical_cases(rng, n, targets):
    """Incident rays that run along the normal (the flip: r = ri > 1) at the angle where cos_theta_2 is `targets`."""
    nrm, ri = unit(rng, n), rng.uniform(1.0001, 3., n)
    t = tangent(rng, nrm)
    c = np.sqrt(1. - (1. - targets) / (ri * ri))
    s = np.sqrt(1. - c * c)
    return normalized([c * nrm[0] + s * t[0], c * nrm[1] + s * t[1], c * nrm[2] + s * t[2]]), nrm, ri


def grazing_cases(rng, n):
    nrm, ri = unit(rng, n), rng.uniform(1.0001, 3., n)
    t = tangent(rng, nrm)
    e = rng.choice([-1., 1.], n) * 10. ** rng.uniform(-17., -1., n)
    e[: n // 16] = 0.
    return normalized([t[0] + e * nrm[0], t[1] + e * nrm[1], t[2] + e * nrm[2]]), nrm, ri


def axis_cases(rng, n):
    i, _, ri = random_cases(rng, n)
    axis, sign = rng.integers(0, 3, n), rng.choice([-1., 1.], n)
    return i, [np.where(axis == j, sign, 0.) for j in range(3)], ri


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(20260808)
    n = 200_000
    sets = {
        "random": random_cases(rng, 1_000_000),
        "normal unit to 1e-6": loose_normal_cases(rng, n),
        "around T": critical_cases(rng, n, T * 2. ** rng.uniform(-2., 2., n)),
        "towards zero": critical_cases(rng, n, 10. ** rng.uniform(-17., -4., n)),
        "critical angle": critical_cases(rng, n, np.zeros(n)),
        "grazing": grazing_cases(rng, n),
        "axis normals": axis_cases(rng, n),
    }
    out = {}
    for name, (i, nrm, ri) in sets.items():
        res = tuple(np.asarray(a) for a in refract(i, nrm, ri))
        for a in res:
            a.setflags(write=False)
        out[name] = res
    return out


def test_constants_leave_a_margin():
    # |v . normal -+ sqrt(cos_theta_2)| <= (r + 1) x (2.1e-6 + 40 x 2^-53) for a normal unit to 1e-6
    bound = (R_MAX + 1.) * 2.1e-6 + 40. * 2. ** -53 * (R_MAX + 1.)
    assert np.sqrt(T) >= 100. * bound                                 # T is four orders of magnitude above the bound's square
    assert R_MAX >= 3.


@pytest.mark.parametrize("name", ["random", "normal unit to 1e-6", "around T", "towards zero", "critical angle", "grazing", "axis normals"])
def test_sign_of_the_computed_dot_is_the_predicted_one(cases, name):
    flip, r, cos2, dn, _ = cases[name]
    sure = (cos2 >= T) & (r <= R_MAX)
    predicted = np.where(flip, 1., -1.)
    wrong = sure & (np.sign(dn) != predicted)                         # (a zero or a NaN is wrong too)
    below = (cos2 >= 0.) & (cos2 < T)
    off = np.abs(dn - predicted * np.sqrt(np.where(cos2 >= 0., cos2, 0.)))[cos2 >= 0.]
    print("%s: %d cases, %d certified (flip %d / no flip %d), %d with 0 <= cos_theta_2 < T, %d total reflections; "
          "max |dot -+ sqrt(cos_theta_2)| %.3e; smallest positive cos_theta_2 %.3e"
          % (name, len(dn), int(sure.sum()), int((sure & flip).sum()), int((sure & ~flip).sum()), int(below.sum()),
             int((cos2 < 0.).sum()), float(off.max()) if len(off) else 0., float(cos2[cos2 > 0.].min())))
    assert not wrong.any(), "%s: %d certified cases with another sign, the first at cos_theta_2 = %r" % (
        name, int(wrong.sum()), float(cos2[wrong][0]))
    assert sure.any() or name in ("towards zero", "critical angle")   # (those two lie below T altogether: the fallback's range)


def test_both_sides_are_certified(cases):
    flip, r, cos2, dn, _ = cases["random"]
    sure = (cos2 >= T) & (r <= R_MAX)
    assert (sure & flip).sum() > 100_000 and (sure & ~flip).sum() > 100_000


def test_the_fallback_range_is_sampled(cases):
    """Below T the kernels form the ray and decide on its computed dot as before: the structured cases do reach that range,
    down to the smallest positive cos_theta_2 there is (an ulp of 1 - x near 1), and the total reflections beyond it."""
    for name in ("around T", "towards zero", "critical angle"):
        flip, r, cos2, dn, _ = cases[name]
        below = (cos2 >= 0.) & (cos2 < T)
        assert below.sum() > 1000, name
    _, _, cos2, _, _ = cases["around T"]
    assert (cos2 >= T).sum() > 1000 and ((cos2 >= T / 4.) & (cos2 < T)).sum() > 1000 and (cos2 <= 4.001 * T).all()
    _, _, cos2, dn, _ = cases["critical angle"]
    assert (cos2 < 0.).any() and (cos2 == 0.).any()
    assert ((cos2 > 0.) & (cos2 <= 2. ** -52)).any()
    # ... and there the sign is NOT always the predicted one (or is zero): the reason the certificate has a threshold
    flip, r, cos2, dn, _ = cases["towards zero"]
    tiny = (cos2 >= 0.) & (cos2 < 1e-12)
    assert tiny.sum() > 1000


def test_the_bound_holds_for_the_dot_before_the_normalisation(cases):
    """What the proof derives: v . normal, v the direction before it is normalised (a division by a positive number, which
    keeps the sign), lies within (r + 1) x (2.1e-6 + 40 ulp) of -+sqrt(cos_theta_2)."""
    for name, (flip, r, cos2, dn, vn) in cases.items():
        ok = (cos2 >= 0.) & (r <= R_MAX)
        err = np.abs(vn - np.where(flip, 1., -1.) * np.sqrt(np.where(ok, cos2, 0.)))[ok]
        lim = ((r + 1.) * (2.1e-6 + 40. * 2. ** -53))[ok]
        assert (err <= lim).all(), name
