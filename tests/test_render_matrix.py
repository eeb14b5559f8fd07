"""CPU pins of the render matrix (tests/render_matrix.py), the premises of tests/test_gpu_render_matrix.py, by the host-only
scene image, the CPU planner and the oracle alone:

1. every cell takes the kernel it claims: the planner (rmi_plan_launches), asked under the cell's environment with the
   cell's scene-image header and integer_exponents verdict, answers with exactly the claimed
   (fast, stack, pow_mode, staged, bvh, cull, edges, order, feedback);
2. the cells are the picker's whole table (rm_kernels.hip): 184 instantiations a flavour, 368 in all;
3. the stacks fill: cast_ray's tree replayed under primary rays of the frame's middle, fixed and rolled, holds max_depth - 1
   live siblings at once at the last depth of every stack size, and one more than the smaller stack has entries at the first
   depth of the next -- as far as the scene's panes go (the staged scenes': STAGED_MOST);
4. the oracle tells the variants apart: one level less deep, and 12.5 replaced by 12, change more than 1e-6 in some channel
   on at least 5 % of the pixels (3 % between depths 32 and 31).  The shares are printed."""
import numpy as np
import pytest

import radiance_reference as RR
import render_matrix as RM
import test_launch_plan as LP
import test_scene_image as SI
import variant_matrix as VM

RM_FLAG_FAST_FP = 2
LDS_SCENE_LIMIT_WORDS = 512          # RM_LDS_SCENE_LIMIT_WORDS: 4 KB
# The most live siblings a ray of the staged scenes (groups 0 and 1) can hold: one a pane.  It is no more because 4 KB of
# scene image hold no more panes: 90 words without a primitive (three lights, the tail the batch loads may read), 52 to 54 a
# triangular pane, 18 to 20 a sphere -- eight panes and nothing else are 510 of the 512 words, a ninth makes 564
# (test_the_staged_budget_holds_eight_panes).  So stacks 4 and 8 fill to the brim there and 16 and 32 hold eight entries.
STAGED_MOST = RM.N_STAGED
assert STAGED_MOST >= 8
MIN_PIXELS = 8
SCENE_NAMES = ("staged", "staged-12", "global", "spheres", "mesh")


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_render_matrix"))


@pytest.fixture(scope="module")
def frames(pkg, O, orc):
    return RM.Frames(pkg, O, orc)


@pytest.fixture(scope="module")
def images(pkg, frames):
    """(scene, generic) -> the host-only scene image, hierarchies and occluder masks on as an upload has them."""
    out = {}
    for name in SCENE_NAMES:
        for generic in (False, True):
            st, img = SI.scene_image(pkg, frames.pair(name, generic)[0].flatten().desc(), 1, 1)
            assert st == 0
            out[name, generic] = img
    return out


def plan_scene(img):
    """The scene of a tests/test_launch_plan.py launch, from an image's header."""
    H = img["H"]
    return dict(n_spheres=H["n_spheres"], n_polygons=H["n_polygons"], n_triangles=H["n_triangles"], total_words=H["total_words"],
                bvh=H["off_bvh_spheres"] or H["off_bvh_triangles"])


def set_knobs(monkeypatch, env):
    for k in RM.KNOB_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        assert k in RM.KNOB_NAMES
        monkeypatch.setenv(k, v)


def planned(pkg, img, row, depth):
    flavour, camera, group, edges, order = row
    l = LP.launch(scene=plan_scene(img), cam=RM.EYE, w=RM.W, h=RM.H, depth=depth, basis=RM.basis_of(camera))
    l["flags"] = RM_FLAG_FAST_FP if flavour == "fast" else 0
    r = LP.plan(pkg, [l], integer_exponents=int(img["verdicts"][1]))[0]
    assert (r.waves, r.per_wave, r.n_tiles) == (1, 1, (RM.W // 32) * (RM.H // 32) * 16)
    return (r.fast, r.stack, r.pow_mode, r.staged, r.bvh, r.cull, r.edges, r.order, r.feedback)


# ---------------------------------------------------------------- 1. the launcher's facts
def test_the_scenes_are_sized_by_the_kernel_choices_rules(images):
    """rm_plan.cpp choose_kernel: staged = at most 4 KB and no hierarchy; cull = RM_CULL_MIN primitives or not staged; the edge
    test from four planar primitives on; POW_INTEGER by the image's verdict."""
    for (name, generic), img in images.items():
        H = img["H"]
        n = H["n_spheres"] + H["n_polygons"] + H["n_triangles"]
        n_panes, _, _, core, small, mesh = RM.SCENES[name]
        print("%s%s: %d primitives, %d words" % (name, " generic" if generic else "", n, H["total_words"]))
        assert bool(img["verdicts"][1]) == (not generic)
        assert H["n_polygons"] == n_panes >= 4 and H["n_lights"] == len(VM.LIGHTS)
        assert (H["off_bvh_spheres"] != 0) == (small == 20) and (H["off_bvh_triangles"] != 0) == mesh
        if name == "staged":
            assert H["total_words"] <= LDS_SCENE_LIMIT_WORDS and RM.CULL_MIN_G1 <= n < 12       # (12: RM_CULL_MIN_PRIMS)
        elif name == "staged-12":
            assert H["total_words"] <= LDS_SCENE_LIMIT_WORDS and n == 12
        else:
            assert H["total_words"] > LDS_SCENE_LIMIT_WORDS and n >= 12
        # the exponents at the ends of the binary powering in every scene, the fractional ones in the generic rows alone
        M = RM.materials(generic)
        used = set(RM.SCENES[name][2]) | ({"back", "right", "left", "below", "marble"} if core else set()) | ({"marble", "small"} if small else set())
        exponents = {M[m]["specular_exponent"] for m in used}
        assert {0., 1000.} <= exponents and ({12.5, 0.5} <= exponents) == generic, (name, exponents)


def test_the_staged_budget_holds_eight_panes(pkg, O):
    """Why STAGED_MOST is no more, and why group 1's contexts lower RM_CULL_MIN: a ninth pane, or twelve primitives of which
    six are panes -- the cheapest such scene -- do not fit the 4 KB."""
    def words(spec):
        st, img = SI.scene_image(pkg, RM.scene_pair(pkg, O, spec, False)[0].flatten().desc(), 1, 1)
        assert st == 0
        return img["H"]["total_words"]

    staged = RM.SCENES["staged"]
    assert words(staged) <= LDS_SCENE_LIMIT_WORDS < words((RM.N_STAGED + 1,) + staged[1:])
    assert words((RM.N_STAGED,) + (RM.SQUARE,) + staged[2:]) > LDS_SCENE_LIMIT_WORDS            # ... and no eight squares
    # (the 20 small spheres stand in for the six cheapest other primitives: the hierarchy only adds to them)
    s, _ = RM.scene_pair(pkg, O, (6,) + staged[1:], False)
    for c, r, _m in VM.small_spheres()[:6]:
        s.shapes.append(pkg.sphere.create(pkg.Vec3f(*c), r, pkg.Reflectance()))
    st, img = SI.scene_image(pkg, s.flatten().desc(), 0, 0)
    assert st == 0 and img["H"]["n_spheres"] + img["H"]["n_polygons"] == 12 and img["H"]["total_words"] > LDS_SCENE_LIMIT_WORDS


@pytest.mark.parametrize("row", RM.rows(), ids=RM.row_id)
def test_a_cell_takes_the_kernel_it_claims(pkg, images, monkeypatch, row):
    flavour, camera, group, edges, order = row
    set_knobs(monkeypatch, RM.knobs(group, edges, order))
    for depth in RM.DEPTHS:
        for generic in (False, True):
            img = images[RM.SCENE_OF_GROUP[group], generic]
            claimed, oriented = RM.claim(row, depth, generic)
            assert oriented == (RM.basis_of(camera) is not None)
            assert planned(pkg, img, row, depth) == claimed, (RM.row_id(row), depth, generic)
    if group == 1:                   # the extra row: twelve primitives in 4 KB, no RM_CULL_MIN
        set_knobs(monkeypatch, RM.knobs(2, edges, order))
        for generic in (False, True):
            assert planned(pkg, images["staged-12", generic], row, 32) == RM.claim(row, 32, generic)[0]
    if group == 3:                   # the extra row: the triangle hierarchy
        assert planned(pkg, images["mesh", False], row, 32) == RM.claim(row, 32, False)[0]


def test_the_rolled_view_is_a_basis_the_library_takes(pkg):
    import ctypes as C
    b = RM.rolled_basis()
    assert pkg.lib().rm_camera_basis_check(C.byref(pkg._lib.camera_basis(b))) == 0
    assert b[2] == LP.FIXED[2] and abs(b[0][0]) > 0.1 and abs(b[0][1]) > 0.1     # the same axis, no quarter turn


def test_the_stack_rule_at_every_depth(pkg, images, monkeypatch):
    """max_depth <= 5 ? 4 : <= 9 ? 8 : <= 17 ? 16 : 32, asked of the planner at every depth from 1 to RM_MAX_DEPTH."""
    row = ("strict", "fixed", 2, True, True)
    set_knobs(monkeypatch, RM.knobs(2, True, True))
    for depth in range(1, LP.RM_MAX_DEPTH + 1):
        assert planned(pkg, images["global", False], row, depth)[1] == RM.stack_of(depth), depth
    assert [RM.stack_of(d) for d in RM.DEPTHS] == [4, 8, 8, 16, 16, 32, 32]


# ---------------------------------------------------------------- 2. the whole table
def test_the_cells_are_the_whole_table():
    claimed = {RM.claim(*cell) for cell in RM.cells()}
    assert len(RM.rows()) == 46 and len(RM.cells()) == 46 * 7 * 2
    table = RM.table()
    assert claimed == table
    assert len(table) == 368 and len({RM.kernel_text(*t) for t in table}) == 368
    for fast in (0, 1):
        mine = [t for t in table if t[0][0] == fast]
        assert len(mine) == 184
        # fixed: 16 | 32 | 32 | 32 | 16 = 128, oriented: 8 | 16 | 16 | 16 = 56, by (staged, bvh, cull, feedback)
        group = lambda t: (0 if not t[0][5] else 1) if t[0][3] else 2 if not t[0][4] else 4 if t[0][8] else 3
        assert [sum(1 for t in mine if not t[1] and group(t) == g) for g in RM.GROUPS] == [16, 32, 32, 32, 16]
        assert [sum(1 for t in mine if t[1] and group(t) == g) for g in RM.GROUPS] == [8, 16, 16, 16, 0]


# ---------------------------------------------------------------- 3. the stacks fill
@pytest.mark.parametrize("camera", RM.CAMERAS)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_the_stacks_fill(frames, name, camera):
    most = RM.PANES_OF[name]
    assert RM.PANES_OF["staged"] == STAGED_MOST and (name.startswith("staged") or most >= LP.RM_MAX_DEPTH - 1)
    for depth in RM.DEPTHS:
        parked = frames.parked(name, camera, depth)
        print("%s, %s, depth %2d: live siblings at once over %d primary rays: %s"
              % (name, camera, depth, len(parked), np.bincount(parked, minlength=min(depth, most + 1)).tolist()))
        expect = min(depth - 1, most)
        assert parked.max() == expect and (parked == expect).sum() >= MIN_PIXELS
        if depth in (6, 10, 18) and depth - 1 <= most:
            # the first depth of the next stack: one more than the smaller stack has entries
            assert parked.max() == RM.stack_of(depth - 1) + 1
    assert (RM.REPLAY_XY[:, 0] < RM.W).all() and (RM.REPLAY_XY[:, 1] < RM.H).all()


# ---------------------------------------------------------------- 4. resolving power
@pytest.mark.parametrize("camera", RM.CAMERAS)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_the_oracle_tells_the_variants_apart(frames, name, camera):
    flat = lambda depth, generic=False, half=VM.HALF: frames.frame(name, camera, depth, generic, half).reshape(-1, 3)
    most = RM.PANES_OF[name]
    for depth in RM.DEPTHS:
        for generic in (False, True):
            true = flat(depth, generic)
            assert np.isfinite(true).all()
            share = VM.told_apart(true, flat(depth - 1, generic))
            print("%s, %s, %s: depth %2d against %2d differs on %.1f %% of the pixels, by %.1e at the most"
                  % (name, camera, "generic" if generic else "integer", depth, depth - 1, 100. * share, np.abs(true - flat(depth - 1, generic)).max()))
            if depth - 1 <= most:    # (beyond its eight panes the staged scene's tree is no deeper: the frames are equal)
                assert share >= (RM.SHARE_DEEP if depth == 32 else VM.SHARE)
            elif name == "staged":
                assert share == 0.
    assert name.startswith("staged") or most >= LP.RM_MAX_DEPTH - 1
    rounded = VM.told_apart(flat(32, True), flat(32, True, 12.))
    print("%s, %s: exponent 12.5 against 12 differs on %.1f %%" % (name, camera, 100. * rounded))
    assert rounded >= VM.SHARE
    # what makes the hierarchies is seen, and so is the roll
    if name in ("spheres", "mesh"):
        assert VM.told_apart(flat(5), frames.frame("global", camera, 5, False).reshape(-1, 3)) >= VM.SHARE
    if camera == "rolled":
        assert VM.told_apart(flat(5), frames.frame(name, "fixed", 5, False).reshape(-1, 3)) >= VM.SHARE
