"""Diffuse bounce in progressive frames on the GPU (-m gpu): rm_accumulate_bounce_device and rm_render_progressive_bounce through
the C ABI, the Python bindings and the C++ mirror, against tests/bounce_reference.py -- the lens rays and steps 1-3 of the rule in
numpy, the first hit and the bounce ray's cast_ray by the CPU oracle against the scene with its lights moved, folded in table
order across passes (pinned on the CPU by tests/test_bounce_abi.py) -- and against the frames of rm_accumulate_soft_device.

What the header calls byte for byte is demanded byte for byte; against the yardstick every channel of every pixel of the rows
a pass writes is demanded within TIGHT = 1e-9 of the mean (n TIGHT of a sum of n samples), no pixel left out.  Largest
deviations observed on an MI355X are recorded in DESIGN.md section 6x.

The fixed view meets no surface from behind and hardly enters the sg = -1 half of the basis: sections 2b and 2c run views from
every side (BR.VIEWS, the context turned by rm_camera_look_at) and rows that land on the edges of the square, each after
asserting, by the oracle alone, that its inputs do exercise what they are there for."""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bounce_reference as BR
import lens_reference as LR
import progressive_reference as PR
import radiance_reference as RR
import soft_reference as SR
import test_camera_basis as CB
import test_gpu_lens as GL
import test_gpu_progressive as GP
import test_gpu_query as GQ
import test_gpu_soft as GS
import workloads

pytestmark = pytest.mark.gpu

TIGHT = BR.TIGHT
NAN, BYTE = GP.NAN, GP.BYTE
# scene -> depth: depth 6 takes the kernels with STACK = 32, the 256 spheres those with the hierarchy; the Cornell box is all
# diffuse triangles (every first hit bounces), the penumbra scene a floor under a glass sphere (the bounce's tree has children)
SCENES = {"demo": 3, "cornell": 3, "penumbra": 3, "synthetic256": 6}
RADII = 1.5                          # of every light, where a test has area lights
FIRST = 3                            # the first row of the parity tests' tables (test_bounce_abi.py checks it for boundary rays)


@pytest.fixture(scope="module")
def ctx(pkg):
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    c = pkg.backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc(O, entry, tmp_path_factory):
    return RR.compile_helper(O, entry, tmp_path_factory.mktemp("orc_bounce"))


@pytest.fixture(scope="module")
def Y(pkg, O, entry, orc, tmp_path_factory):
    return BR.Yardstick(pkg, O, orc, BR.compile_helper(O, entry, tmp_path_factory.mktemp("orb_bounce")))


def run_bounce(pkg, c, w, h, depth, aperture, focus, table, offsets, bounce, strength, sizes, want_mean=True, want_bytes=True):
    """Passes of the sizes `sizes` over consecutive slices of the three tables on torch's current stream, the first with
    n_before = 0, into buffers that held NaN (and BYTE) -> (sum, mean, bytes) as numpy, None for what was not asked for."""
    import torch
    p = pkg.backend.make_params(workloads.FOV, float(h), float(w), depth)
    total = torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda:0")
    mean = torch.full((h, w, 3), NAN, dtype=torch.float64, device="cuda:0") if want_mean else None
    rgb8 = torch.full((h, w, 3), BYTE, dtype=torch.uint8, device="cuda:0") if want_bytes else None
    torch.cuda.synchronize()
    done = 0
    assert sum(sizes) == len(table) == len(offsets) == len(bounce)
    for n in sizes:
        c.accumulate_bounce_device(p, total, aperture, focus, np.ascontiguousarray(table[done:done + n]),
                                   np.ascontiguousarray(offsets[done:done + n]), np.ascontiguousarray(bounce[done:done + n]), strength, done,
                                   mean=mean, rgb8=rgb8)
        done += n
    torch.cuda.synchronize()
    return (total.cpu().numpy(), mean.cpu().numpy() if want_mean else None, rgb8.cpu().numpy() if want_bytes else None)


def zero_offsets(Y, name, n):
    return np.zeros((n, Y.n_lights(name), 3))


def host_view(pkg, Y, name):
    """The view BR.VIEWS[name] by the library's host look-at (rm_camera_basis_look_at: no context, no GPU) ->
    (scene, depth, (eye, basis) -- None for the fixed view --, the distance to the target, (eye, target, up hint) or None)."""
    scene = BR.VIEWS[name][0]
    scene, depth, eye, target, up = BR.look_from(name, *GQ.bounds_of(Y.scene(scene)[0].flatten().desc()))
    if eye is None:
        return scene, depth, None, float(np.linalg.norm(np.array(target) - np.array(Y.eye(scene)))), None
    st, basis = CB.look_at(pkg, eye, target, up)
    assert st == 0
    return scene, depth, (eye, RR.basis_tuple(basis)), float(np.linalg.norm(np.array(target) - np.array(eye))), (eye, target, up)


@contextlib.contextmanager
def looking(pkg, c, Y, name):
    """Uploads the scene of BR.VIEWS[name] and turns the context to the view -> (scene, depth, view, focus), view = (eye, basis)
    as the context reports them (None: the fixed view); the fixed view again afterwards."""
    scene, depth, host, focus, look = host_view(pkg, Y, name)
    GL.upload(c, Y.scene(scene)[0])
    try:
        view = None
        if look is not None:
            c.look_at(*look)
            pos, basis, on = c.camera()
            assert on
            view = ((pos.x, pos.y, pos.z), RR.basis_tuple(basis))
            assert view == host                                       # the CPU pins (test_bounce_abi.py) are pins of this view
        yield scene, depth, view, focus
    finally:
        c.orient(None)


# ---------------------------------------------------------------- 1. strength 0 is the area lights' frame
@pytest.mark.parametrize("name,depth", [("demo", 3), ("cornell", 3), ("synthetic256", 6)])
def test_strength_zero_is_the_soft_frame_byte_for_byte(pkg, ctx, Y, name, depth):
    """Two passes of 5 samples: 12 pixels a wave, four idle lanes.  The bounce table holds NaN: with strength 0 it is not read."""
    aperture, focus = GL.LENS[name]
    GL.upload(ctx, Y.scene(name)[0])
    table = ctx.lens_sequence(0, 10)
    offsets = ctx.light_sequence(0, 10, (RADII,) * Y.n_lights(name))
    soft = GS.run_soft(pkg, ctx, 32, 32, depth, aperture, focus, table, offsets, (5, 5))
    import torch
    nan_table = torch.full((5, 2), NAN, dtype=torch.float64, device="cuda:0")
    p = pkg.backend.make_params(workloads.FOV, 32., 32., depth)
    total = torch.full((32, 32, 3), NAN, dtype=torch.float64, device="cuda:0")
    mean = torch.full((32, 32, 3), NAN, dtype=torch.float64, device="cuda:0")
    rgb8 = torch.full((32, 32, 3), BYTE, dtype=torch.uint8, device="cuda:0")
    for k in (0, 1):
        ctx.accumulate_bounce_device(p, total, aperture, focus, table[5 * k:5 * k + 5], np.ascontiguousarray(offsets[5 * k:5 * k + 5]), nan_table,
                                     0., 5 * k, mean=mean, rgb8=rgb8)
    torch.cuda.synchronize()
    for a, b, what in zip((total.cpu().numpy(), mean.cpu().numpy(), rgb8.cpu().numpy()), soft, ("sum", "mean", "bytes")):
        assert not (what != "bytes" and np.isnan(a).any())
        assert a.tobytes() == b.tobytes(), "%s: %s differs in %d pixels" % (name, what, int((a != b).any(axis=2).sum()))
    assert soft[1].any()


# ---------------------------------------------------------------- 2. parity with the yardstick
@pytest.mark.parametrize("n", [1, 5, 64])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_bounce_frames_match_the_yardstick(pkg, ctx, Y, name, n):
    """The library's sequence, and a random bounce table: a lane that reads another sample's row is another picture.  With light
    radii and without (offsets of zero)."""
    depth = SCENES[name]
    GL.upload(ctx, Y.scene(name)[0])
    rng = np.random.default_rng(20262100 + n)
    table = ctx.lens_sequence(FIRST, n)
    for aperture in (0., LR.APERTURE):
        for what, bounce in (("sequence", pkg.backend.bounce_sequence(FIRST, n)), ("random", BR.random_table(rng, n))):
            for lights, offsets in (("radii", ctx.light_sequence(FIRST, n, (RADII,) * Y.n_lights(name))), ("points", zero_offsets(Y, name, n))):
                if (what, lights) == ("random", "radii") and n == 64:
                    continue                                          # (the longest case once with each table)
                total, mean, rgb8 = run_bounce(pkg, ctx, 32, 32, depth, aperture, LR.FOCUS, table, offsets, bounce, 1., (n,))
                ref_sum, ref_mean = Y.bounce(name, 32, 32, depth, aperture, LR.FOCUS, table, offsets, bounce, 1., (n,))
                plain = Y.soft(name, 32, 32, depth, aperture, LR.FOCUS, table, offsets, (n,))[1]
                d_mean, d_sum = GL.worst(mean, ref_mean), GL.worst(total, ref_sum)
                lit = int((np.abs(ref_mean - plain) > 0.05).any(axis=2).sum())
                print("%s depth %d, %d samples, aperture %g, %s table, %s: max |delta| mean %.3e, sum %.3e (%d pixels differ from the frame without)"
                      % (name, depth, n, aperture, what, lights, d_mean, d_sum, lit))
                assert not np.isnan(mean).any() and not np.isnan(total).any()
                assert d_mean < TIGHT and d_sum < n * TIGHT
                assert rgb8.tobytes() == PR.to_bytes(mean).tobytes()
                assert lit > 0                                        # (light did come back: not the frame without a bounce again)


@pytest.mark.parametrize("name", sorted(BR.BOUNCED))
def test_the_device_frame_differs_from_the_plain_one_in_the_committed_pixels(pkg, ctx, Y, name):
    depth, rows, pixels = BR.BOUNCED[name]
    GL.upload(ctx, Y.scene(name)[0])
    table, bounce = ctx.lens_sequence(0, rows), pkg.backend.bounce_sequence(0, rows)
    lit = run_bounce(pkg, ctx, 32, 32, depth, 0., LR.FOCUS, table, zero_offsets(Y, name, rows), bounce, 1., (rows,))[1]
    plain = GP.run_passes(pkg, ctx, 32, 32, depth, 0., LR.FOCUS, table, (rows,))[1]
    assert int((np.abs(lit - plain) > 0.05).any(axis=2).sum()) == pixels


def test_depth_one_returns_the_background_along_the_bounce(pkg, ctx, Y):
    """max_depth == 1: the bounce ray lies beyond the cap and brings back the background; max_depth == 0 is the member underneath."""
    GL.upload(ctx, Y.scene("cornell")[0])
    table, bounce = ctx.lens_sequence(FIRST, 5), pkg.backend.bounce_sequence(FIRST, 5)
    offsets = zero_offsets(Y, "cornell", 5)
    total, mean, _ = run_bounce(pkg, ctx, 32, 32, 1, 0., LR.FOCUS, table, offsets, bounce, 1., (5,))
    ref_sum, ref_mean = Y.bounce("cornell", 32, 32, 1, 0., LR.FOCUS, table, offsets, bounce, 1., (5,))
    plain = Y.soft("cornell", 32, 32, 1, 0., LR.FOCUS, table, offsets, (5,))[1]
    assert GL.worst(mean, ref_mean) < TIGHT and GL.worst(total, ref_sum) < 5 * TIGHT
    assert GL.worst(ref_mean, plain) > 0.01
    flat = run_bounce(pkg, ctx, 32, 32, 0, 0., LR.FOCUS, table, offsets, bounce, 1., (5,))
    soft = GS.run_soft(pkg, ctx, 32, 32, 0, 0., LR.FOCUS, table, offsets, (5,))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(flat, soft))


# ---------------------------------------------------------------- 2b. views from every side
@pytest.mark.parametrize("name", sorted(BR.REQUIRED))
def test_bounce_frames_match_the_yardstick_from_every_side(pkg, ctx, Y, name):
    """The views of BR.VIEWS: surfaces met from behind (Nf = -N), facing normals in the sg = -1 half of the basis and on both
    of its poles exactly, front and back faces in one wave.  Each case first demands of its own inputs, by the oracle alone,
    the counters it is there for (BR.REQUIRED), then what test_bounce_frames_match_the_yardstick demands: aperture 0 and 0.4,
    the library's sequence and a random table, point lights -- and area lights in the Cornell box."""
    n = 5
    with looking(pkg, ctx, Y, name) as (scene, depth, view, focus):
        table = ctx.lens_sequence(FIRST, n)
        lights = [("points", zero_offsets(Y, scene, n))]
        if scene == "cornell":
            lights.append(("radii", ctx.light_sequence(FIRST, n, (RADII,) * Y.n_lights(scene))))
        for what, bounce in BR.view_tables(name, FIRST, n):
            if what == "sequence":
                assert bounce.tobytes() == pkg.backend.bounce_sequence(FIRST, n).tobytes()
            for aperture in (0., LR.APERTURE):
                for how, offsets in lights:
                    c = Y.counters(scene, 32, 32, depth, aperture, focus, table, offsets, bounce, 1., view)
                    if aperture == 0.:
                        BR.assert_covers(name, c)
                    total, mean, rgb8 = run_bounce(pkg, ctx, 32, 32, depth, aperture, focus, table, offsets, bounce, 1., (n,))
                    ref_sum, ref_mean = Y.bounce(scene, 32, 32, depth, aperture, focus, table, offsets, bounce, 1., (n,), view)
                    plain = Y.soft(scene, 32, 32, depth, aperture, focus, table, offsets, (n,), view)[1]
                    d_mean, d_sum = GL.worst(mean, ref_mean), GL.worst(total, ref_sum)
                    lit = int((np.abs(ref_mean - plain) > 0.05).any(axis=2).sum())
                    print("%s, aperture %g, %s table, %s: max |delta| mean %.3e, sum %.3e (%d pixels differ from the frame without; %d samples "
                          "bounce, %d from behind, %d with Nf.z < 0, Nf.z %.4f .. %.4f, %d / %d on the poles)" % (
                              name, aperture, what, how, d_mean, d_sum, lit, c["bouncing"], c["back"], c["below"], c["min_z"], c["max_z"],
                              c["pole_up"], c["pole_down"]))
                    assert not np.isnan(mean).any() and not np.isnan(total).any()
                    assert d_mean < TIGHT and d_sum < n * TIGHT
                    assert rgb8.tobytes() == PR.to_bytes(mean).tobytes()
                    assert lit > 0
                    if view is not None:                              # another picture than the fixed view's
                        fixed = Y.bounce(scene, 32, 32, depth, aperture, focus, table, offsets, bounce, 1., (n,))[1]
                        assert GL.worst(ref_mean, fixed) > 0.05


# ---------------------------------------------------------------- 2c. the edges of the square
@pytest.mark.parametrize("name", BR.EDGE_VIEWS)
def test_samples_on_the_edges_of_the_square(pkg, ctx, Y, name):
    """Rows built so that one bouncing pixel a row lands on x == 0, x == 1 - 2^-53, the same of y, or a corner, exactly
    (BR.edge_table): where the radicand of the disc map rounds below zero and only step 2's clamp keeps the square root from NaN."""
    n = len(BR.EDGE_KINDS)
    with looking(pkg, ctx, Y, name) as (scene, depth, view, focus):
        table = ctx.lens_sequence(FIRST, n)
        bounce, _ = BR.edge_table(np.random.default_rng(BR.EDGE_SEED), Y.bouncing_pixels(scene, 32, 32, 0., focus, table, view), BR.EDGE_KINDS)
        offsets = zero_offsets(Y, scene, n)
        c = Y.counters(scene, 32, 32, depth, 0., focus, table, offsets, bounce, 1., view)
        BR.assert_edges(c)
        total, mean, rgb8 = run_bounce(pkg, ctx, 32, 32, depth, 0., focus, table, offsets, bounce, 1., (n,))
        ref_sum, ref_mean = Y.bounce(scene, 32, 32, depth, 0., focus, table, offsets, bounce, 1., (n,), view)
        d_mean, d_sum = GL.worst(mean, ref_mean), GL.worst(total, ref_sum)
        print("%s, %d edge rows: max |delta| mean %.3e, sum %.3e (%d samples on an edge, %d on a corner, %d with a radicand below zero, "
              "the lowest %.3e)" % (name, n, d_mean, d_sum, c["edge"], c["corner"], c["negative"], c["min_radicand"]))
        assert not np.isnan(mean).any() and not np.isnan(total).any()
        assert d_mean < TIGHT and d_sum < n * TIGHT
        assert rgb8.tobytes() == PR.to_bytes(mean).tobytes()
        # the edge samples are not special to a pass size: two passes are the one pass byte for byte
        two = run_bounce(pkg, ctx, 32, 32, depth, 0., focus, table, offsets, bounce, 1., (n - 11, 11))
        for a, b, what in zip(two, (total, mean, rgb8), ("sum", "mean", "bytes")):
            assert a.tobytes() == b.tobytes(), what


# ---------------------------------------------------------------- 3. folding
def test_three_passes_over_slices_are_one_pass_byte_for_byte(pkg, ctx, Y):
    depth = SCENES["penumbra"]
    GL.upload(ctx, Y.scene("penumbra")[0])
    table, offsets, bounce = ctx.lens_sequence(0, 12), ctx.light_sequence(0, 12, SR.PENUMBRA_RADII), pkg.backend.bounce_sequence(0, 12)
    one = run_bounce(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table, offsets, bounce, 1., (12,))
    three = run_bounce(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table, offsets, bounce, 1., (5, 4, 3))
    for a, b, what in zip(three, one, ("sum", "mean", "bytes")):
        assert a.tobytes() == b.tobytes(), what
    assert not np.isnan(one[1]).any()
    # the optional outputs change nothing in the sum
    bare = run_bounce(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table, offsets, bounce, 1., (5, 4, 3), want_mean=False, want_bytes=False)
    assert bare[0].tobytes() == one[0].tobytes()


def test_200_rows_in_five_passes_match_the_yardstick(pkg, ctx, Y):
    depth = SCENES["demo"]
    GL.upload(ctx, Y.scene("demo")[0])
    table, offsets, bounce = ctx.lens_sequence(0, 200), ctx.light_sequence(0, 200, (RADII, RADII)), pkg.backend.bounce_sequence(0, 200)
    assert bounce.tobytes() == BR.bounce_sequence(0, 200).tobytes()
    total, mean, rgb8 = run_bounce(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table, offsets, bounce, 0.75, (40,) * 5)
    ref_sum, ref_mean = Y.bounce("demo", 32, 32, depth, LR.APERTURE, LR.FOCUS, table, offsets, bounce, 0.75, (40,) * 5)
    d_mean, d_sum = GL.worst(mean, ref_mean), GL.worst(total, ref_sum)
    print("demo depth %d, 5 x 40 samples, strength 0.75: max |delta| mean %.3e, sum %.3e" % (depth, d_mean, d_sum))
    assert not np.isnan(mean).any() and d_mean < TIGHT and d_sum < 200 * TIGHT
    assert rgb8.tobytes() == PR.to_bytes(mean).tobytes()


# ---------------------------------------------------------------- 4. the hash reaches the device
def test_the_per_pixel_shift_is_the_headers_hash_of_the_pixel_index(pkg, ctx, Y):
    """One table row over a flat floor under one light: all that tells two pixels' bounces apart is the shift.  64 x 32 and
    32 x 32: the pixel (x, y) is numbered y * frame_width + x, so the same (x, y) takes another shift in the narrower frame."""
    GL.upload(ctx, Y.scene("floor")[0])
    table, bounce = ctx.lens_sequence(FIRST, 1), pkg.backend.bounce_sequence(FIRST, 1)
    offsets = zero_offsets(Y, "floor", 1)
    for w, other in ((64, 32), (32, 64)):
        total, mean, _ = run_bounce(pkg, ctx, w, 32, 3, 0., LR.FOCUS, table, offsets, bounce, 1., (1,))
        ref = Y.bounce("floor", w, 32, 3, 0., LR.FOCUS, table, offsets, bounce, 1., (1,))[1]
        unshifted = Y.bounce("floor", w, 32, 3, 0., LR.FOCUS, table, offsets, bounce, 1., (1,), shift=False)[1]
        renumbered = Y.bounce("floor", w, 32, 3, 0., LR.FOCUS, table, offsets, bounce, 1., (1,), pix_width=other)[1]
        plain = Y.soft("floor", w, 32, 3, 0., LR.FOCUS, table, offsets, (1,))[1]
        print("floor %d x 32: max |delta| %.3e; without the shift %.3e, numbered by width %d %.3e" % (
            w, GL.worst(mean, ref), GL.worst(mean, unshifted), other, GL.worst(mean, renumbered)))
        assert GL.worst(mean, ref) < TIGHT
        assert GL.worst(mean, unshifted) > 1e-3 and GL.worst(mean, renumbered) > 1e-3
        assert (np.abs(ref - plain) > 1e-3).any(axis=2).sum() > 100   # the floor fills a good part of the view and every hit of it bounces


# ---------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_buffers_alone(pkg, ctx, Y):
    import torch
    L, B = pkg.lib(), pkg._lib
    GL.upload(ctx, Y.scene("demo")[0])
    p = pkg.backend.make_params(workloads.FOV, 32., 32., 3)
    lens = B.rm_lens(0., 1., 4, 0)
    vp = lambda t: C.c_void_p(t.data_ptr())
    table = torch.from_numpy(ctx.lens_sequence(0, 4)).to("cuda:0")
    offsets = torch.zeros((4, 2, 3), dtype=torch.float64, device="cuda:0")
    bounce = torch.from_numpy(pkg.backend.bounce_sequence(0, 4)).to("cuda:0")
    total = torch.full((32, 32, 3), NAN, dtype=torch.float64, device="cuda:0")

    def call(bounce_ptr, strength, n_lights=2):
        return L.rm_accumulate_bounce_device(ctx.ptr, C.byref(p), C.byref(lens), vp(table), vp(offsets), n_lights, bounce_ptr, strength, 0,
                                             vp(total), None, None, None)

    assert call(None, 1.) == B.RM_ERR_INVALID_ARG and b"NULL bounce table" in L.rm_last_error(ctx.ptr)
    for bad in (-1e-9, -1., NAN, float("inf"), -float("inf")):
        assert call(vp(bounce), bad) == B.RM_ERR_INVALID_ARG and b"strength" in L.rm_last_error(ctx.ptr)
    assert call(vp(bounce), 1., n_lights=3) == B.RM_ERR_INVALID_ARG and b"n_lights" in L.rm_last_error(ctx.ptr)
    torch.cuda.synchronize()
    assert torch.isnan(total).all()                                   # nothing was launched
    assert call(vp(bounce), 1.) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(total).any()
    # the tick: a refused strength changes neither the count nor the key
    host = np.full((32, 32, 3), -3.5)
    assert ctx.render_progressive_bounce(p, 0., 1., 4, 1., restart=True)[1] == 4
    n_total = C.c_uint32(77)
    D = C.POINTER(C.c_double)
    for bad in (-1., NAN, float("inf")):
        st = L.rm_render_progressive_bounce(ctx.ptr, C.byref(p), C.byref(lens), None, 0, bad, 0, host.ctypes.data_as(D), None, C.byref(n_total), None)
        assert st == B.RM_ERR_INVALID_ARG and n_total.value == 77 and np.all(host == -3.5) and b"strength" in L.rm_last_error(ctx.ptr)
    assert ctx.render_progressive_bounce(p, 0., 1., 4, 1.)[1] == 8


# ---------------------------------------------------------------- 6. the host path
CPP_MAIN = r"""
#include <cstdio>
#include "rusty_marcher.hpp"
using namespace rusty_marcher;
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    scene::Scene sc = scene::Scene::create_default();
    framebuffer::FrameBuffer fb = framebuffer::create_frame_buffer(32, 32);
    renderer::Renderer r = renderer::create_renderer(1.5, 32., 32.);
    const std::vector<double> radii{1.5, 1.5};
    for (int k = 0; k < 3; k++) {
        r.render_progressive_bounce(fb, sc, 8u, 1., radii, 0.4, 5.);
        std::printf("samples %u\n", r.last_samples);
    }
    std::FILE *f = std::fopen(argv[1], "wb");
    if (!f) return 3;
    for (const auto &row : fb.buffer) std::fwrite(row.data(), sizeof(Vec3f), row.size(), f);
    std::fclose(f);
    r.render_progressive_soft(fb, sc, radii, 0.4, 5., 8u);
    std::printf("soft %u\n", r.last_samples);
    r.render_progressive_bounce(fb, sc, 8u, 1., radii, 0.4, 5.);
    std::printf("bounce %u\n", r.last_samples);
    r.render_progressive_bounce(fb, sc, 8u, 0.5, radii, 0.4, 5.);
    std::printf("strength %u\n", r.last_samples);
    return 0;
}
"""


def test_host_path_c_python_and_the_cpp_mirror(pkg, entry, ctx, Y, capsys, tmp_path):
    assert workloads.FOV == 1.5 and (LR.APERTURE, LR.FOCUS) == (0.4, 5.)
    L, B = pkg.lib(), pkg._lib
    depth, radii = SCENES["demo"], (RADII, RADII)
    scene = Y.scene("demo")[0]
    GL.upload(ctx, scene)
    table, offsets, bounce = ctx.lens_sequence(0, 24), ctx.light_sequence(0, 24, radii), pkg.backend.bounce_sequence(0, 24)
    _, device, device8 = run_bounce(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table, offsets, bounce, 1., (8, 8, 8))
    ref_mean = Y.bounce("demo", 32, 32, depth, LR.APERTURE, LR.FOCUS, table, offsets, bounce, 1., (8, 8, 8))[1]
    assert GL.worst(device, ref_mean) < TIGHT                         # rows [N, N + 8) of the three sequences, tick after tick
    p = pkg.backend.make_params(workloads.FOV, 32., 32., depth)
    host, host8 = np.full((32, 32, 3), -3.5), np.full((32, 32, 3), 7, np.uint8)

    def tick(strength=1., r=radii, restart=False, **kw):
        return ctx.render_progressive_bounce(p, LR.APERTURE, LR.FOCUS, 8, strength, r, restart, **kw)[1]

    def soft(restart=False, **kw):
        return ctx.render_progressive_soft(p, radii, LR.APERTURE, LR.FOCUS, 8, restart, **kw)[1]

    # three ticks of 8: the frame goes on, and is the device call's
    assert tick(restart=True) == 8 and tick() == 16
    timing, total = ctx.render_progressive_bounce(p, LR.APERTURE, LR.FOCUS, 8, 1., radii, host_rgb=host, host_rgb8=host8)
    assert total == 24 and host.tobytes() == device.tobytes() and host8.tobytes() == device8.tobytes()
    assert timing.kernel_ms > 0. and timing.total_ms >= timing.kernel_ms
    # the same through the C entry point itself
    r64 = np.ascontiguousarray(radii, dtype=np.float64)
    lens, n_total, again = B.rm_lens(LR.APERTURE, LR.FOCUS, 8, 0), C.c_uint32(0), np.full((32, 32, 3), -3.5)
    D = C.POINTER(C.c_double)
    for k in range(3):
        st = L.rm_render_progressive_bounce(ctx.ptr, C.byref(p), C.byref(lens), r64.ctypes.data_as(D), 2, 1., 1 if k == 0 else 0,
                                            again.ctypes.data_as(D), None, C.byref(n_total), None)
        assert st == 0 and n_total.value == 8 * (k + 1)
    assert again.tobytes() == device.tobytes()
    # what begins the frame again, one at a time (each followed by a tick that goes on: 16)
    assert tick(0.5) == 8 and tick(0.5) == 16                         # a changed strength
    assert tick() == 8 and tick() == 16                               # ... and back
    assert soft() == 8 and soft() == 16                               # bounce -> soft
    assert tick() == 8 and tick() == 16                               # soft -> bounce
    assert tick(0.) == 8                                              # a strength of zero is a strength: not the soft call's frame
    zero = np.full((32, 32, 3), -3.5)
    assert tick(0., host_rgb=zero) == 16 and soft() == 8
    assert zero.tobytes() == GS.run_soft(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table[:16], offsets[:16], (8, 8))[1].tobytes()
    # point lights: no radii
    points = np.full((32, 32, 3), -3.5)
    assert tick(1., None, host_rgb=points) == 8
    assert points.tobytes() == run_bounce(pkg, ctx, 32, 32, depth, LR.APERTURE, LR.FOCUS, table[:8], np.zeros((8, 2, 3)), bounce[:8], 1., (8,))[1].tobytes()
    # ... and the frame of the first three ticks again, byte for byte (all three sequences start over)
    assert tick() == 8 and tick() == 16
    again.fill(-3.5)
    assert tick(host_rgb=again) == 24 and again.tobytes() == device.tobytes()
    # Renderer.render_progressive_bounce and render_global_illumination: the prints and the return value of render()
    r = pkg.create_renderer(workloads.FOV, 32., 32.)
    r.max_depth = depth
    fb = pkg.create_frame_buffer(32, 32)
    capsys.readouterr()
    message = r.render_progressive_bounce(fb, scene, 8, 1., radii, LR.APERTURE, LR.FOCUS, restart=True)
    out = capsys.readouterr().out
    assert message.startswith("Scene rendered in ") and message in out and "compute units used" in out
    assert r.last_samples == 8 and r.last_timing.kernel_ms > 0.
    r.render_progressive_bounce(fb, scene, 8, 1., radii, LR.APERTURE, LR.FOCUS)
    r.render_progressive_bounce(fb, scene, 8, 1., radii, LR.APERTURE, LR.FOCUS)
    assert r.last_samples == 24 and fb.buffer.tobytes() == device.tobytes()
    r.render_global_illumination(fb, scene, 72)                       # 64 + 8, restarted, through a pinhole, point lights
    t72, b72 = ctx.lens_sequence(0, 72), pkg.backend.bounce_sequence(0, 72)
    whole = run_bounce(pkg, ctx, 32, 32, depth, 0., 1., t72, np.zeros((72, 2, 3)), b72, 1., (64, 8))[1]
    assert r.last_samples == 72 and fb.buffer.tobytes() == whole.tobytes()
    # the C++ mirror, from compiled code
    src, exe, dump = tmp_path / "tick.cpp", tmp_path / "tick", tmp_path / "tick.f64"
    src.write_text(CPP_MAIN)
    lib_dir = os.path.join(entry.PKG_DIR, "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(entry.ROOT, "include"), "-I", os.path.join(entry.PKG_DIR, "host"),
                           str(src), "-o", str(exe), "-L", lib_dir, "-lrusty_marcher_amd", "-Wl,-rpath," + lib_dir, "-Wl,-rpath," + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")])
    log = subprocess.check_output([str(exe), str(dump)]).decode()
    assert [l for l in log.splitlines() if l.split()[0] in ("samples", "soft", "bounce", "strength")] == \
        ["samples 8", "samples 16", "samples 24", "soft 8", "bounce 8", "strength 8"]
    assert np.fromfile(str(dump)).tobytes() == device.tobytes()
