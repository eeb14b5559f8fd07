"""The scenes, views and cells of the render matrix: recipes that reach every instantiation of
rm_render_static<STACK, POW, 1, 1, STAGED, BVH, CULL, EDGES, ORDER, FEEDBACK> (csrc/rm_kernels.hip) with a ray tree that fills
the kernel's per-lane stack.  No GPU and no fixtures: tests/test_render_matrix.py pins on the CPU that a cell takes the kernel
it claims, that the cells are the picker's whole table, that the stacks fill and that the oracle alone tells the variants
apart; tests/test_gpu_render_matrix.py holds the GPU to the oracle.

A cell is (flavour, camera, group, edges, order, depth, generic):
  flavour  "strict" | "fast" (RM_FLAG_FAST_FP)
  camera   "fixed": the reference's view; "rolled": the same eye and view axis, rolled by ROLL about it -- the oriented kernels
  group    0..4, rm_kernels.hip's kernel groups, each with a scene sized by choose_kernel's rules (rm_plan.cpp):
           0 and 1  `staged`: eight triangular panes and nothing else, 510 of the 512 words an LDS copy may have; group 1's
                    contexts are made under RM_CULL_MIN=8, or the scene would take the plain walk
           2        `global`: 36 square panes, the back sphere, four lit spheres
           3 and 4  `spheres`: + 20 small spheres, a sphere hierarchy; group 4's contexts are made under RM_FEEDBACK=1
           extra rows: `mesh` (+ a 14-triangle mesh instead: a triangle hierarchy) through group 3's kernels, `staged-12`
           (five panes, seven spheres: what group 1 takes with no knob set) through group 1's
  edges    the cull's edge test (off: RM_CULL_EDGES=0; the plain walk of group 0 has no cull and so none)
  order    the dispatch order (on: RM_PATCH_ORDER=1 RM_TILE_CLASSIFY=1 RM_FIRST_ROUND=0, off: RM_PATCH_ORDER=0; the oriented
           kernels come with it only, the feedback kernels of group 4 without)
  depth    5, 6, 9, 10, 17, 18, 32: the last depth of each stack size (4 / 8 / 16 / 32) and the first of the next
  generic  exponents 12.5 and 0.5 in the scene: POW_GENERIC; otherwise POW_INTEGER

The panes: optics.rs gives a glass surface both children only where the ray meets its front at more than asin(1 / ri) off the
normal.  N square panes, 3 apart along -z, are tilted 20 degrees about +y, +x, -y, -x in turn and have ri = 3.5 (16.6 degrees): a
ray down the z axis meets every one at about 20 degrees, parks a reflected sibling at each and -- the four tilts cancelling over a
cycle -- stays near the axis for as many panes as there are.  (Tilted about y alone, as tests/variant_matrix.py's six are, the ray
drifts to the side where panes of opposite tilt converge and loses the reflection after five or so.)"""
import numpy as np

import radiance_reference as RR
import variant_matrix as VM
import workloads

W, H = 96, 64                        # 3 x 2 patches, 96 tiles: not square, more than one patch row
FOV = workloads.FOV
EYE = VM.EYE
ROLL = 0.6                           # radians about the view axis: no multiple of a quarter turn
DEPTHS = (5, 6, 9, 10, 17, 18, 32)
STACKS = (4, 8, 16, 32)
POW_GENERIC, POW_INTEGER = 0, 1
FLAVOURS = ("strict", "fast")
CAMERAS = ("fixed", "rolled")
GROUPS = (0, 1, 2, 3, 4)

PANE_HALF, PANE_TILT, PANE_GAP, PANE_Z0 = 6., 20., 3., -4.
N_DEEP = 36                          # the panes of the scenes in global memory: 31 of them park a sibling at depth 32
SHARE_DEEP = 0.03                    # the share of pixels depth 32 against 31 must change (the share shrinks by 0.9 a level)


def stack_of(depth):
    """choose_kernel's rule, restated: a lane parks at most one sibling per level below the cap."""
    return 4 if depth <= 5 else 8 if depth <= 9 else 16 if depth <= 17 else 32


# ---------------------------------------------------------------- the scenes
# a pane's outline in its own plane, in units of PANE_HALF, counter-clockwise: the square of the scenes in global memory, and
# the triangle of the staged scenes, whose incircle (radius 0.62) is centred on the axis -- a vertex less is 2 to 4 words less
SQUARE = ((-1., -1.), (1., -1.), (1., 1.), (-1., 1.))
TRIANGLE = ((-1., -0.62), (1., -0.62), (0., 1.38))


def panes(n, outline=SQUARE):
    """n panes about the z axis, tilted about +y, +x, -y, -x in turn, facing the camera, counter-clockwise in xy."""
    out = []
    a = np.deg2rad(PANE_TILT)
    for k in range(n):
        s = a if k % 4 < 2 else -a
        if k % 2 == 0:               # about y
            u, v = np.array([np.cos(s), 0., -np.sin(s)]), np.array([0., 1., 0.])
        else:                        # about x
            u, v = np.array([1., 0., 0.]), np.array([0., np.cos(s), np.sin(s)])
        c = np.array([0., 0., PANE_Z0 - PANE_GAP * k])
        out.append([tuple(float(x) for x in c + PANE_HALF * (su * u + sv * v)) for su, sv in outline])
    return out


def materials(generic, half=VM.HALF):
    """variant_matrix.materials with the panes' reflection and diffusion low enough for level 31 to stay visible, and two
    more pane materials for the scenes that have no room for an opaque sphere: `even` with `left`'s exponent (1000) and `odd`
    with `right`'s (0.5 in the generic rows)."""
    M = VM.materials(generic, half)
    for name in ("even", "odd"):
        M[name] = dict(M[name], refractive_index=3.5, reflection=0.1, diffusion=0.05)
    M["even-left"] = dict(M["even"], specular_exponent=M["left"]["specular_exponent"])
    M["odd-right"] = dict(M["odd"], specular_exponent=M["right"]["specular_exponent"])
    return M


CORE = {name: (c, r) for c, r, name in VM.CORE_SPHERES[1:]}           # right, left, below, marble
N_STAGED = 8                         # the panes 4 KB of scene image hold beside three lights (tests/test_render_matrix.py)
# name -> (panes, their outline, their materials in turn, the back sphere and CORE, how many of the 20 small spheres, the
# 14-triangle mesh)
SCENES = {
    "staged": (N_STAGED, TRIANGLE, ("even", "odd", "even-left", "odd-right"), False, 0, False),
    "staged-12": (5, TRIANGLE, ("even", "odd"), True, 2, False),
    "global": (N_DEEP, SQUARE, ("even", "odd"), True, 0, False),
    "spheres": (N_DEEP, SQUARE, ("even", "odd"), True, 20, False),
    "mesh": (N_DEEP, SQUARE, ("even", "odd"), True, 0, True),
}
SCENE_OF_GROUP = {0: "staged", 1: "staged", 2: "global", 3: "spheres", 4: "spheres"}
PANES_OF = {name: spec[0] for name, spec in SCENES.items()}          # the most live siblings a ray can hold: one a pane
# choose_kernel culls from RM_CULL_MIN primitives on, 12 unless set: 4 KB hold no 12 primitives of which more than five are
# panes, so group 1's contexts set it to the staged scene's eight, and groups 0 and 1 render the same scene.  `staged-12` is
# what group 1 takes with no knob set -- five panes and seven spheres, twelve primitives in 4 KB: an extra row, as `mesh` is
CULL_MIN_G1 = N_STAGED


def scene_pair(pkg, O, name, generic, half=VM.HALF):
    """-> (product Scene -- None without `pkg` --, oracle scene) of SCENES[name] (or of a tuple like its), from the one recipe."""
    n, outline, pane_materials, core, small, mesh = SCENES[name] if isinstance(name, str) else name
    s, o = (pkg.Scene.new() if pkg is not None else None), O.OracleScene()
    M = materials(generic, half)

    def sphere(c, r, m):
        if s is not None:
            s.shapes.append(pkg.sphere.create(pkg.Vec3f(*c), r, pkg.Reflectance(**M[m])))
        o.add_sphere(c, r, O.reflectance(**M[m]))

    for k, q in enumerate(panes(n, outline)):
        m = M[pane_materials[k % len(pane_materials)]]
        if s is not None:
            s.shapes.append(pkg.polygon.ConvexPolygon.create([pkg.Vec3f(*p) for p in q], pkg.Reflectance(**m)))
        o.add_polygon(q, O.reflectance(**m))
    if core:
        sphere((0., 0., PANE_Z0 - PANE_GAP * (n - 1) - 10.), 6., "back")
        for m in ("right", "left", "below", "marble"):
            sphere(CORE[m][0], CORE[m][1], m)
    for c, r, m in VM.small_spheres()[:small]:
        sphere(c, r, m)
    if mesh:
        tri = VM.mesh_triangles()
        if s is not None:
            s.shapes.append(pkg.obj.Obj(tri))
        o.add_obj(tri)
    for pos, col, inten in VM.LIGHTS:
        if s is not None:
            s.lights.append(pkg.create_light(pkg.Vec3f(*pos), pkg.Vec3f(*col), inten))
        o.add_light(pos, col, inten)
    if s is not None:
        s.camera = pkg.Vec3f(*EYE)
    o.set_camera(EYE)
    return s, o


# ---------------------------------------------------------------- the views
def rolled_basis():
    """(right, up, forward) of the fixed view rolled by ROLL about its axis, as plain tuples of doubles."""
    c, s = float(np.cos(ROLL)), float(np.sin(ROLL))
    return (c, s, 0.), (-s, c, 0.), (0., 0., -1.)


def basis_of(camera):
    return None if camera == "fixed" else rolled_basis()


def directions(orc, camera, xy=None):
    """The un-normalised primary directions of the W x H frame (or of the positions `xy`), as the header states them: the
    fixed view's are backproject's (renderer.rs:128-135), the rolled view's (bx * right + by * up) + forward per component --
    tests/test_gpu_camera.py's OracleCamera.directions, operation for operation."""
    xy = RR.pixel_positions(W, H) if xy is None else xy
    return RR.sample_directions(xy, orc.renderer(W, H, FOV), basis_of(camera))


# the pixels whose ray trees the CPU premises replay: a lattice over the frame's middle, which looks down the panes
REPLAY_XY = np.array([(x, y) for y in range(22, 43, 2) for x in range(38, 59, 2)], dtype=np.float64)


# ---------------------------------------------------------------- the cells
def rows():
    """The 46 rows the GPU module is parametrised by: (flavour, camera, group, edges, order), as the picker's table has them."""
    out = []
    for flavour in FLAVOURS:
        for group in GROUPS:
            for edges in ((False,) if group == 0 else (True, False)):
                for order in ((False,) if group == 4 else (True, False)):
                    out.append((flavour, "fixed", group, edges, order))
        for group in GROUPS[:4]:     # no oriented kernels with the tile-level feedback, none without the dispatch order
            for edges in ((False,) if group == 0 else (True, False)):
                out.append((flavour, "rolled", group, edges, True))
    return out


def row_id(row):
    flavour, camera, group, edges, order = row
    return "%s-%s-g%d-%s-%s" % (flavour, camera, group, "edges" if edges else "noedges", "order" if order else "noorder")


def knobs(group, edges, order):
    """The environment a context of the row is made under, of KNOB_NAMES; the others of them must be unset.  (The oriented
    kernels carry the dispatch order whatever the knobs say: a rolled row takes the context whose order is forced on, so
    that the launch uses it too.)"""
    env = {"RM_CULL_EDGES": "1" if edges or group == 0 else "0"}
    if group == 1:
        env["RM_CULL_MIN"] = str(CULL_MIN_G1)
    if group == 4:
        env["RM_FEEDBACK"] = "1"
    elif order:
        env.update({"RM_PATCH_ORDER": "1", "RM_TILE_CLASSIFY": "1", "RM_FIRST_ROUND": "0"})
    else:
        env["RM_PATCH_ORDER"] = "0"
    return env


KNOB_NAMES = ("RM_CULL_EDGES", "RM_FEEDBACK", "RM_PATCH_ORDER", "RM_TILE_CLASSIFY", "RM_FIRST_ROUND", "RM_FORCE_STACK",
              "RM_FORCE_GENERIC_POW", "RM_FORCE_FAST_FP", "RM_FORCE_UNSTAGED", "RM_DISABLE_BVH", "RM_CULL_MIN", "RM_TILE_ORDER",
              "RM_DEBUG_EMPTY", "RM_CLASSIFY_IN_LAUNCH", "RM_PATCH_ORDER_MAX", "RM_PATCH_ORDER_MAX_DEEP", "RM_CLASSIFY_MIN_TILES")


def claim(row, depth, generic):
    """What rm_render_static's template arguments must be for the cell:
    (fast, stack, pow_mode, staged, bvh, cull, edges, order, feedback), and whether the kernel is an oriented one."""
    flavour, camera, group, edges, order = row
    staged, bvh, cull, feedback = group <= 1, group >= 3, group >= 1, group == 4
    return (int(flavour == "fast"), stack_of(depth), POW_GENERIC if generic else POW_INTEGER, int(staged), int(bvh), int(cull),
            int(edges and cull), int(order), int(feedback)), camera == "rolled"


def kernel_text(claimed, oriented):
    """The name rm_kernel_name gives the claimed instantiation."""
    fast, stack, pow_mode, staged, bvh, cull, edges, order, feedback = claimed
    b = lambda x: "true" if x else "false"
    return "%s%s::rm_render_static<%d, %d, 1, 1, %s, %s, %s, %s, %s, %s>" % (
        "rmdev_fast" if fast else "rmdev_strict", "_o" if oriented else "", stack, pow_mode, b(staged), b(bvh), b(cull), b(edges),
        b(order), b(feedback))


def cells():
    """Every cell: (row, depth, generic)."""
    return [(row, depth, generic) for row in rows() for depth in DEPTHS for generic in (False, True)]


def table():
    """The picker's table written down as a rule (rm_kernels.hip pick_eo / RM_PICK_NAME): groups x edges x order x stack x
    pow; group 0 has no cull and so no edge test; group 4 carries the feedback and no order; the oriented set has no group 4 and
    the order always on.  -> the set of (claimed tuple, oriented)."""
    out = set()
    for fast in (0, 1):
        for oriented in (False, True):
            for group in GROUPS:
                if oriented and group == 4:
                    continue
                staged, bvh, cull, feedback = group <= 1, group >= 3, group >= 1, group == 4
                for edges in ((0, 1) if cull else (0,)):
                    for order in ((1,) if oriented else (0,) if feedback else (0, 1)):
                        for stack in STACKS:
                            for pow_mode in (POW_GENERIC, POW_INTEGER):
                                out.add(((fast, stack, pow_mode, int(staged), int(bvh), int(cull), edges, order, int(feedback)), oriented))
    return out


# ---------------------------------------------------------------- the oracle's frames, each made once
class Frames:
    """The scenes and the oracle's frames of the matrix, made once and shared (never written to)."""

    def __init__(self, pkg, O, orc):
        self.pkg, self.O, self.orc = pkg, O, orc
        self._pair, self._ref = {}, {}

    def pair(self, name, generic, half=VM.HALF):
        key = (name, generic, half)
        if key not in self._pair:
            self._pair[key] = scene_pair(self.pkg if half == VM.HALF else None, self.O, name, generic, half)
        return self._pair[key]

    def frame(self, name, camera, depth, generic, half=VM.HALF):
        """orc_cast_ray along the primary rays of the W x H frame: [H][W][3]."""
        key = (name, camera, depth, generic, half)
        if key not in self._ref:
            rgb = self.orc.cast(self.pair(name, generic, half)[1], EYE, directions(self.orc, camera), depth, normalize=True)
            self._ref[key] = rgb.reshape(H, W, 3)
            self._ref[key].setflags(write=False)
        return self._ref[key]

    def parked(self, name, camera, depth, generic=False):
        """The most live siblings at once under each primary ray of REPLAY_XY (cast_ray's tree replayed, variant_matrix.parked_at_once)."""
        key = ("parked", name, camera, depth, generic)
        if key not in self._ref:
            d = self.orc.normalized(directions(self.orc, camera, REPLAY_XY))
            oscene = self.pair(name, generic)[1]
            self._ref[key] = np.array([VM.parked_at_once(self.O, oscene, EYE, v, depth) for v in d])
        return self._ref[key]
