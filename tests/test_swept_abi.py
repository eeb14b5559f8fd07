"""CPU-side checks of the swept hierarchies (include/rusty_marcher_amd.h, "swept hierarchies"): the refit of a scene image's
boxes over per-shape offset extents (csrc/rm_swept_image.cpp), by the host-only hook and the oracle alone.

1. The entry points are exported and bound by ctypes, the Rust shim and the C++ mirror with the header's shapes,
   rm_build_info says " swept-hierarchy" and the ABI is still 5; a NULL context is refused.
2. The two small scenes end their device order in a partial leaf (1 of 4 spheres, 1 of 2 triangles).
3. Extents of zero reproduce the image's nodes byte for byte; any extents change no word outside the nodes' boxes.
4. Containment: every leaf child's box holds its primitives' boxes at both corners of the extents and at 16 random offsets
   within them; every inner child's box holds the two boxes of the node it refers to.
5. rm_swept_extents is numpy's min and max; every row of rm_motion_sequence lies within rm_swept_motion_extents.
6. The walk model: over 8 rows within the extents, no primitive the swept tree leaves unreached is the closest hit of the
   moved scene (the numpy restatement, held to the oracle's own decision and shape on moving_reference.MovedScene).
7. Refusals name the offender.
8. The refit as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hierarchy_reference as HR
import motion_reference as MR
import moving_reference as MV
import swept_reference as SW
import test_gpu_query as GQ
import test_rust_binding as RB

FUNCTIONS = ["rm_swept_extents", "rm_swept_motion_extents", "rm_swept_build", "rm_swept_free", "rm_accumulate_swept_device",
             "rm_accumulate_converging_swept_device"]
REFIT_SCENES = SW.SCENES + ("synthetic256",)


@pytest.fixture(scope="module")
def batch(O, entry, tmp_path_factory):
    d = tmp_path_factory.mktemp("orc_batch_swept")
    src, so = d / "orc_batch.c", d / "orc_batch.so"
    src.write_text(GQ.BATCH_C)
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-shared", "-fPIC",
                           "-I", os.path.join(entry.ROOT, "oracle"), str(src), "-o", str(so)])
    return GQ.OracleBatch(O, C.CDLL(str(so)))


@pytest.fixture(scope="module")
def images(pkg, O):
    """name -> (desc, image, oracle scene), each made once."""
    made = {}

    def get(name):
        if name not in made:
            scene, oscene = SW.scene_pair(pkg, O, name)
            made[name] = HR.image_of(pkg, scene) + (oscene,)
        return made[name]
    return get


# ---------------------------------------------------------------- 1. the ABI
def test_swept_symbols_are_exported_and_bound(pkg, entry):
    L = pkg.lib()
    header = open(os.path.join(entry.ROOT, "include", "rusty_marcher_amd.h")).read()
    c, r = RB.header_functions(), RB.rust_functions()
    for name in FUNCTIONS:
        assert hasattr(L, name) and name in pkg._lib.SIGNATURES, name
        assert re.search(r"^(rm_status|void) +%s\(" % name, header, flags=re.M), name
        assert c[name] == r[name], "%s: header %s, gpu.rs %s" % (name, c[name], r[name])
    # the two device calls are their moving-shapes siblings with the handle behind n_shapes
    for swept, moving, at in (("rm_accumulate_swept_device", "rm_accumulate_moving_device", 8),
                              ("rm_accumulate_converging_swept_device", "rm_accumulate_converging_moving_device", 10)):
        want = list(c[moving][1])
        want.insert(at, "ptr")
        assert c[swept] == (c[moving][0], want)
    assert b" swept-hierarchy" in L.rm_build_info() and L.rm_abi_version() == 5
    assert "swept hierarchies" in header and "RM_SWEPT_BVH" in header
    for name in ("swept", "accumulate_swept_device", "accumulate_converging_swept_device"):
        assert callable(getattr(pkg.backend.Context, name))
    assert callable(pkg.backend.swept_extents) and callable(pkg.backend.swept_motion_extents)
    mirror = open(os.path.join(entry.PKG_DIR, "host", "rusty_marcher.hpp")).read()
    for name in ("rm_swept_build", "rm_swept_free", "rm_accumulate_swept_device", "rm_accumulate_converging_swept_device"):
        assert name + "(" in mirror, name
    out = C.c_void_p(7)
    assert L.rm_swept_build(None, None, None, 0, C.byref(out)) == SW.INVALID_ARG and out.value == 7
    assert b"rm_swept_build: NULL ctx" in L.rm_last_error(None)
    assert L.rm_accumulate_swept_device(None, None, None, None, None, 0, None, 0, None, 0, None, None, None, None) == SW.INVALID_ARG
    assert L.rm_accumulate_converging_swept_device(None, None, None, None, None, 0, None, 0, None, 0, None, 0, None, None) == SW.INVALID_ARG
    L.rm_swept_free(None, None)                                        # allowed


def test_the_mirror_compiles_with_the_swept_calls(entry, tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "rusty_marcher.hpp"\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-I", os.path.join(entry.ROOT, "include"),
                           "-I", os.path.join(entry.PKG_DIR, "host"), str(src)])


# ---------------------------------------------------------------- 2. the small scenes
@pytest.mark.parametrize("name,held,leaf", [("seventeen", 1, 4), ("thirteen", 1, 2)])
def test_the_small_scenes_end_in_a_partial_leaf(images, name, held, leaf):
    """The leaves fetch `leaf` records whatever they hold; the pid map has no word for the ones behind the last primitive."""
    desc, img, _ = images(name)
    H = img["H"]
    kind = SW.HIERARCHY[name]
    assert (H["n_spheres"], H["n_polygons"], H["n_triangles"]) == ((17, 0, 0) if name == "seventeen" else (0, 0, 13))
    tree = HR.Tree(img, kind)
    first, count = SW.last_leaf(tree)
    assert tree.leaf_size == leaf and count == held < leaf
    assert len(img["pid_map"]) == tree.first_pid + tree.count          # nothing behind the last pid
    assert first + leaf > tree.count                                   # the leaf's unconditional fetches pass the last primitive


# ---------------------------------------------------------------- 3. what the refit writes
@pytest.mark.parametrize("name", REFIT_SCENES)
def test_zero_extents_are_the_image_and_any_extents_touch_the_boxes_alone(pkg, images, name):
    desc, img, _ = images(name)
    n = desc.n_shapes
    zero = np.zeros((n, 3))
    for lo, hi in ((zero, zero), (-zero, -zero), (-zero, zero)):
        st, blob = SW.swept_image(pkg, desc, lo, hi)
        assert st == 0 and blob.tobytes() == img["blob"].tobytes(), "%s: extents of zero change the image" % name
    rng = np.random.default_rng(20262001)
    lo, hi = SW.random_extents(rng, n, SW.scale_of(desc))
    st, blob = SW.swept_image(pkg, desc, lo, hi)
    assert st == 0 and blob.size == img["blob"].size
    nodes, boxes = SW.node_words(img)
    outside = np.ones(blob.size, bool)
    outside[boxes] = False
    assert np.array_equal(blob[outside], img["blob"][outside])          # refs, pads and every other section
    if name in SW.HIERARCHY:
        assert len(boxes) and (blob[boxes] != img["blob"][boxes]).any()
        assert sorted(HR.Tree(SW.swept_of(img, blob), SW.HIERARCHY[name]).nodes) == sorted(HR.Tree(img, SW.HIERARCHY[name]).nodes)
    else:
        assert not len(nodes) and blob.tobytes() == img["blob"].tobytes()   # no hierarchy: the image itself
    # ... and without hierarchies in the image the refit has nothing to write
    st, flat = SW.swept_image(pkg, desc, lo, hi, use_bvh=0)
    assert st == 0
    st0, flat0 = SW.swept_image(pkg, desc, zero, zero, use_bvh=0)
    assert st0 == 0 and flat.tobytes() == flat0.tobytes()


def holds(outer, inner):
    return (outer[:3] <= inner[..., :3]).all() and (outer[3:] >= inner[..., 3:]).all()


@pytest.mark.parametrize("name", sorted(SW.HIERARCHY))
def test_swept_boxes_contain_their_primitives_over_the_extents(pkg, images, name):
    desc, img, _ = images(name)
    kind = SW.HIERARCHY[name]
    rng = np.random.default_rng(20262002)
    lo, hi = SW.random_extents(rng, desc.n_shapes, SW.scale_of(desc))
    st, blob = SW.swept_image(pkg, desc, lo, hi)
    assert st == 0
    tree = HR.Tree(SW.swept_of(img, blob), kind)
    rows = np.concatenate([SW.rows_within(rng, lo, hi, 18)])            # both corners and 16 offsets within
    prim = [SW.primitive_boxes(desc, img, kind, row) for row in rows]
    leaves = inner = 0
    for lbox, rbox, left, right in tree.nodes.values():
        for box, (idx, cnt) in ((lbox, left), (rbox, right)):
            if cnt:
                for b in prim:
                    assert holds(box, b[idx:idx + cnt]), (name, idx, cnt)
                leaves += 1
            else:
                below = tree.nodes[idx]
                assert holds(box, below[0]) and holds(box, below[1]), (name, idx)
                inner += 1
    print("%s: %d leaf children and %d inner children hold what lies below them" % (name, leaves, inner))
    assert leaves >= 2


# ---------------------------------------------------------------- 5. the extents helpers
def test_swept_extents_are_numpys_min_and_max(pkg):
    rng = np.random.default_rng(20262003)
    table = rng.normal(size=(9, 7, 3)) * 10. ** rng.integers(-3, 4, size=(1, 7, 1))
    table[3, 2] = 0.
    lo, hi = pkg.backend.swept_extents(table)
    assert lo.tobytes() == table.min(axis=0).tobytes() and hi.tobytes() == table.max(axis=0).tobytes()
    one = pkg.backend.swept_extents(table[:1])
    assert one[0].tobytes() == one[1].tobytes() == table[0].tobytes()
    with pytest.raises(pkg._lib.BackendError, match="no rows"):
        pkg.backend.swept_extents(np.zeros((0, 3, 3)))


@pytest.mark.parametrize("name", ["demo", "cornell", "matrix-mesh", "synthetic256"])
def test_every_row_of_the_motion_sequence_lies_within_the_documented_extents(pkg, O, name):
    _, oscene = SW.scene_pair(None if name.startswith("matrix-") else pkg, O, name)
    kinds = [int(oscene.c.shapes[k].kind) for k in range(oscene.c.n_shapes)]
    v = MV.velocities(kinds, MV.SPEED.get(name, MV.CELL_SPEED))
    lo, hi = pkg.backend.swept_motion_extents(v, MV.SHUTTER)
    e = np.asarray(v, np.float64) * np.float64(MV.SHUTTER)
    assert lo.tobytes() == np.minimum(0., e).tobytes() and hi.tobytes() == np.maximum(0., e).tobytes()
    rows = MR.motion_sequence(0, 4096, v, MV.SHUTTER)
    assert (rows >= lo).all() and (rows <= hi).all() and (rows != 0.).any()


# ---------------------------------------------------------------- 6. the walk model
def rays_of(name, desc):
    if name in HR.SCENES:
        o, d = HR.unit_rays(name, desc)
        return o[:6000], d[:6000]
    if name.startswith("chain-"):
        return HR.chain_rays()
    lo, hi = GQ.bounds_of(desc)
    rng = np.random.default_rng(20262004)
    o, d = GQ.random_rays(rng, 3000, lo, hi)
    aim = GQ.unit(rng.uniform(lo, hi, size=(3000, 3)))                  # from the camera into the scene
    return np.concatenate([o, np.zeros((3000, 3))]), np.concatenate([d, aim])


@pytest.mark.parametrize("name", sorted(SW.HIERARCHY))
def test_the_swept_walk_reaches_what_the_moved_scene_hits(pkg, O, batch, images, name):
    desc, img, oscene = images(name)
    kind = SW.HIERARCHY[name]
    rng = np.random.default_rng(20262005)
    lo, hi = SW.random_extents(rng, desc.n_shapes, SW.scale_of(desc))
    st, blob = SW.swept_image(pkg, desc, lo, hi)
    assert st == 0
    swept = SW.swept_of(img, blob)
    o, d = rays_of(name, desc)
    rows = SW.rows_within(rng, lo, hi, 8)
    walked = 0
    for r, row in enumerate(rows):
        ref = SW.MovedRanged(desc, row).closest(o, d, (0., np.inf))
        if r < 2 and not name.startswith("chain-"):                     # the restatement is the oracle's on the moved scene
            hit, shape, _, _ = batch.closest(MV.MovedScene(O, oscene, np.zeros((oscene.c.n_lights, 3)), row), o, d)
            assert np.array_equal(ref["hit"], hit) and np.array_equal(ref["shape"][hit == 1] % 256, shape[hit == 1])
        pid = HR.pid_of(img, ref["shape"], ref["element"])
        missed = HR.unreached(swept, o, d, pid)
        assert not missed.any(), "%s row %d: %d closest hits on a primitive the swept walk never reaches" % (name, r, int(missed.sum()))
        tree = HR.Tree(swept, kind)
        walked += int(((pid >= tree.first_pid) & (pid < tree.first_pid + tree.count)).sum())
    # ... and the image's own boxes would not do: the rows move primitives out of them
    lost = 0
    for row in rows[:2]:
        ref = SW.MovedRanged(desc, row).closest(o, d, (0., np.inf))
        lost += int(HR.unreached(img, o, d, HR.pid_of(img, ref["shape"], ref["element"])).sum())
    print("%s: %d closest hits on a primitive of the hierarchy over 8 rows, all reached; the unswept boxes lose %d over 2 rows" % (name, walked, lost))
    assert walked >= 8


# ---------------------------------------------------------------- 7. refusals
def test_refusals_name_the_offender(pkg, images):
    desc, img, _ = images("matrix-mesh")
    n = desc.n_shapes
    L = pkg.lib()
    zero = np.zeros((n, 3))
    for bad, text in ((np.nan, b"shape 3"), (np.inf, b"shape 3"), (-np.inf, b"shape 3")):
        hi = zero.copy()
        hi[3, 1] = bad
        st, blob = SW.swept_image(pkg, desc, zero, hi)
        assert st == SW.INVALID_ARG and blob is None and text in L.rm_last_error(None) and b"finite" in L.rm_last_error(None)
    lo = zero.copy()
    lo[5, 2] = 1e-300
    st, _ = SW.swept_image(pkg, desc, lo, zero)
    assert st == SW.INVALID_ARG and b"shape 5" in L.rm_last_error(None) and b"lo <= hi" in L.rm_last_error(None)
    st, _ = SW.swept_image(pkg, desc, zero[:-1], zero[:-1])
    assert st == SW.INVALID_ARG and ("n_shapes %d, the resident scene has %d" % (n - 1, n)).encode() in L.rm_last_error(None)
    st, _ = SW.swept_image(pkg, desc, zero, zero, n_shapes=n + 1)
    assert st == SW.INVALID_ARG and b"n_shapes" in L.rm_last_error(None)
    with pytest.raises(ValueError, match="n_shapes, 3"):
        pkg.backend._extents(np.zeros((3, 2)), np.zeros((3, 2)))


# ---------------------------------------------------------------- 8. the refit, stand-alone under the sanitizers
def test_the_refit_under_asan_ubsan(entry, tmp_path):
    exe = tmp_path / "swept_refit"
    csrc = os.path.join(entry.PKG_DIR, "csrc")
    subprocess.check_call([
        "g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
        "-I", os.path.join(entry.ROOT, "include"), "-I", csrc,
        os.path.join(csrc, "rm_scene.cpp"), os.path.join(csrc, "rm_image.cpp"), os.path.join(csrc, "rm_swept_image.cpp"), os.path.join(entry.ROOT, "tests", "native", "swept_refit_main.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([str(exe)], capture_output=True, env=env)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert b"swept refit ok" in out.stdout
