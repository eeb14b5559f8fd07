"""CPU part of tests/test_gpu_grazing.py: the probe builder (tests/grazing_probes.py) against the oracle alone.

A GPU frame that equals the oracle's says nothing about a bound unless the frame holds something at the bound's edge.  So
every probe list the GPU tests render is built here and checked: each probe changes its own pixel of the oracle's frame
(one dead probe fails the list as vacuous), and nothing but its pixel and that pixel's 8 neighbours."""
import pytest

import grazing_probes as GP


@pytest.fixture(scope="module")
def cam(O, tmp_path_factory):
    return GP.oracle_camera(O, tmp_path_factory.mktemp("orc_camera"))


def test_probe_pixels_are_tile_corners_apart_from_each_other():
    for w, h in GP.SMALL_FRAMES + [GP.BIG_FRAME]:
        for n in (12, 14, 70):
            px = GP.probe_pixels(w, h, n, seed=n)
            assert len(set(px)) == n and px == GP.probe_pixels(w, h, n, seed=n)          # seeded: the same list every time
            rows = h // 32 * 32
            assert all(x % 16 in (0, 15) and y % 4 in (0, 3) and 0 <= x < w and 0 <= y < rows for x, y in px)
            assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) >= 3 for i, a in enumerate(px) for b in px[:i])
            # the four frame corners (they are patch corners too), the centre pixel, the centre column and the centre row
            assert set(px[:4]) == {(0, 0), (w - 1, 0), (0, rows - 1), (w - 1, rows - 1)} and px[4] == (w // 2, h // 2)
            assert sum(x == w // 2 for x, _ in px) >= 2 and sum(y == h // 2 for _, y in px) >= 2
            assert sum(x % 32 in (0, 31) and y % 32 in (0, 31) for x, y in px) >= 6


def test_every_probe_list_of_the_gpu_tests_is_live(O, pkg, cam):
    counts = GP.check_every_list(O, pkg, cam)
    for name, c in counts.items():
        print(name, c)
        assert all(v >= 4 for v in c.values()), (name, c)             # every kind is there, in every list
    # both kinds at every t in every primary list, read off the lists as built
    for name in GP.PRIMARY_SCENES:
        for w, h in GP.frames_for(name):
            _, _, probes = GP.primary_case(O, name, w, h)
            seen = {(kind, t) for _, _, kind, t in probes}
            assert seen == {(k, t) for k in ("centred", "tangent") for t in GP.T_VALUES}, (name, w, h, seen)


def test_the_shadow_probes_sit_on_rows_of_the_mask_table_that_clear_bits(O, pkg):
    """A receiver whose bounding sphere holds a light has every bit set, and a probe on its shadow rays tests nothing of
    the masks' bounds.  Here neither receiver's row is full, every probe's bit is set in its receiver's row for its own
    light -- and, since a row names little else, clear for the other light: the bit is the bound's decision."""
    from test_shadow_masks import masks
    view = GP.View(O, *GP.SHADOW_FRAME)
    recipe, probes = GP.shadow_recipe(O, view, GP.SHADOW_PROBES, 3)
    occ, shape_of = masks(pkg, GP.product_scene(pkg, recipe, lights=GP.SHADOW_LIGHTS))
    assert occ is not None and len(occ) == len(recipe) <= 64
    pid_of = {shape: pid for pid, shape in enumerate(shape_of)}
    full = (1 << len(recipe)) - 1
    for receiver in (0, 1):
        for light in (0, 1):
            row = occ[pid_of[receiver]][light]
            assert row != full and bin(row).count("1") <= len(recipe) // 2 + 2, (receiver, light, bin(row))
    assert {(kind, light, receiver) for _, _, kind, _, light, receiver in probes} == \
        {(k, l, r) for k in GP.SHADOW_KINDS for l in (0, 1) for r in (0, 1)}
    for x, y, kind, index, light, receiver in probes:
        assert occ[pid_of[receiver]][light] >> pid_of[index] & 1, "the %s probe of pixel (%d, %d) is not in its receiver's mask" % (kind, x, y)
        assert not occ[pid_of[receiver]][1 - light] >> pid_of[index] & 1


def test_a_probe_moved_off_its_ray_is_reported_dead(O):
    """The check itself: the same list with its tangent probes one radius further out no longer passes."""
    view, recipe, probes = GP.primary_case(O, "s14", *GP.SMALL_FRAMES[0], eps=-1.)     # r (1 - eps) = 2 r off the ray
    with pytest.raises(AssertionError, match="dead tangent probe"):
        GP.live_primary(O, recipe, probes, view)
