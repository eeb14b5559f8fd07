// AddressSanitizer / UBSan exercise of the host half of the C ABI (csrc/rm_scene.cpp):
// scene builder, OBJ ingest (good and malformed files), status formatting, the hierarchy
// builder (csrc/rm_bvh.hpp) and the device image the upload builds from a description, good
// and bad ones (csrc/rm_image.cpp); and the two decisions of a shading launch (csrc/rm_plan.cpp rm_shading_variant_of,
// rm_shading_grid) over the cases of tests/test_launch_plan.py; and the sampled frames' host arithmetic (csrc/rm_sampling.cpp):
// the three sequences, the frame identity and the staging rule.  CPU only.
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rusty_marcher_amd.h"
#include "rm_internal.h"
#include "rm_bvh.hpp"
#include "rm_image.hpp"
#include "rm_plan.hpp"
#include "rm_sampling.hpp"

// the device half (rm_device.hip) is not part of this CPU-only build: its one symbol the
// host half's callers need is the error accessor
extern "C" const char *rm_last_error(const rm_ctx *) { return rm_get_host_error(); }
// ... and the kernel tables the render launch's plan hands out (rm_plan.cpp links against them; no plan is made here)
const void *rm_pick_kernel(bool, bool, bool, bool, bool, int, bool, int, int) { return nullptr; }
const void *rm_pick_kernel_oriented(bool, bool, bool, bool, bool, int, int) { return nullptr; }
const void *rmdev::rm_classify_kernel(bool) { return nullptr; }
const void *rmdev::rm_classify_kernel_oriented(bool) { return nullptr; }

// rm_build_bvh invariants the kernel's walk relies on: `order` is a permutation; every leaf
// holds 1..leaf_size consecutive primitives and every primitive sits in exactly one leaf;
// a child box contains the boxes of everything below it (with the builder's inflation).
static void walk_hierarchy(const rm_bvh &h, const std::vector<rm_aabb> &boxes, uint64_t ref, const double *box,
                           uint32_t leaf_size, std::vector<int> &seen, int depth) {
    assert(depth <= (int)h.depth && h.depth <= RM_BVH_MAX_DEPTH);     // the kernel's stack: 64 entries, one per level
    const uint32_t idx = (uint32_t)ref, cnt = (uint32_t)(ref >> 32);
    if (cnt) {                                                          // leaf
        assert(cnt <= leaf_size && (size_t)idx + cnt <= boxes.size());
        for (uint32_t k = 0; k < cnt; k++) {
            const rm_aabb &b = boxes[h.order[idx + k]];
            seen[idx + k]++;
            for (int a = 0; a < 3; a++) assert(box[a] <= b.lo[a] && b.hi[a] <= box[3 + a]);
        }
        return;
    }
    assert((size_t)(idx + 1) * RM_BVH_NODE_WORDS <= h.nodes.size());
    const double *n = &h.nodes[(size_t)idx * RM_BVH_NODE_WORDS];
    uint64_t l, r;
    std::memcpy(&l, &n[12], 8);
    std::memcpy(&r, &n[13], 8);
    for (int a = 0; a < 3; a++) {                                       // children inside the parent (root: no parent box)
        if (box) { assert(box[a] <= n[a] + 1e-6 && n[3 + a] <= box[3 + a] + 1e-6); assert(box[a] <= n[6 + a] + 1e-6 && n[9 + a] <= box[3 + a] + 1e-6); }
        assert(n[a] <= n[3 + a] && n[6 + a] <= n[9 + a]);
    }
    walk_hierarchy(h, boxes, l, n, leaf_size, seen, depth + 1);
    walk_hierarchy(h, boxes, r, n + 6, leaf_size, seen, depth + 1);
}

static void check_hierarchy(uint32_t n_prims, uint32_t leaf_size) {
    std::vector<rm_aabb> boxes(n_prims);
    uint64_t state = 0x9E3779B97F4A7C15ull * (n_prims + 1);
    auto rnd = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (double)(state >> 11) / 9007199254740992.; };
    for (rm_aabb &b : boxes)
        for (int a = 0; a < 3; a++) {
            const double c = (n_prims % 2 ? 0. : 100. * rnd() - 50.), e = 2. * rnd();   // odd counts: all coincident centres
            b.lo[a] = c - e; b.hi[a] = c + e;
        }
    if (n_prims <= leaf_size) return;                                   // the upload never builds one over so few
    const rm_bvh h = rm_build_bvh(boxes, leaf_size);
    assert(h.order.size() == n_prims && h.nodes.size() % RM_BVH_NODE_WORDS == 0 && !h.nodes.empty());
    std::vector<int> perm(n_prims, 0), seen(n_prims, 0);
    for (uint32_t o : h.order) { assert(o < n_prims); perm[o]++; }
    for (int c : perm) assert(c == 1);
    walk_hierarchy(h, boxes, 0, nullptr, leaf_size, seen, 0);           // ref 0 = inner node 0, the root
    for (int c : seen) assert(c == 1);
}

// rm_build_image over a good description, every way the upload and the hooks ask for it: the sections inside the blob,
// the occluder masks behind total_words, a pid map entry per primitive
static void check_image(const rm_scene_desc &d) {
    for (const rm_image_options opt : {rm_image_options{true, true}, rm_image_options{false, true}, rm_image_options{true, false}}) {
        rm_image img;
        std::string error;
        assert(rm_build_image(&d, opt, img, error) == RM_OK && error.empty());
        const rm_dev_header &H = img.H;
        const uint32_t n = H.n_spheres + H.n_polygons + H.n_triangles;
        assert(H.n_spheres <= d.n_spheres && H.n_polygons <= d.n_polygons && H.n_triangles <= d.n_triangles && H.n_lights == d.n_lights);
        assert(img.pid_map.size() == 2u * n && H.total_words >= 64u && H.total_words % 2u == 0u);
        assert(img.blob.size() == (H.off_occ ? (size_t)H.total_words + (((size_t)n * H.n_lights + 1u) & ~(size_t)1) : (size_t)H.total_words));
        assert(!H.off_occ || (opt.shadow_masks && H.off_occ == H.total_words));
        assert(opt.use_bvh || (!H.off_bvh_spheres && !H.off_bvh_triangles));
        for (uint32_t q = 0; q < n; q++) assert(img.pid_map[2u * q] < d.n_shapes);
    }
}

// ... and over descriptions it must refuse: a status and the upload's text, never a crash
static void check_refusals(const rm_scene_desc &good) {
    std::vector<rm_shape_ref> shapes(good.shapes, good.shapes + good.n_shapes);
    std::vector<rm_polygon> polygons(good.polygons, good.polygons + good.n_polygons);
    auto refused = [&](const rm_scene_desc &d, const char *text) {
        rm_image img;
        std::string error;
        assert(rm_build_image(&d, rm_image_options{}, img, error) == RM_ERR_INVALID_ARG);
        assert(error == text);
    };
    auto with_shape = [&](size_t at, rm_shape_ref ref, const char *text) {
        std::vector<rm_shape_ref> edited = shapes;
        edited[at] = ref;
        rm_scene_desc d = good;
        d.shapes = edited.data();
        refused(d, text);
    };
    size_t sphere = shapes.size(), polygon = shapes.size(), mesh = shapes.size();
    for (size_t i = 0; i < shapes.size(); i++) {
        if (shapes[i].kind == RM_SHAPE_SPHERE) sphere = i;
        if (shapes[i].kind == RM_SHAPE_POLYGON) polygon = i;
        if (shapes[i].kind == RM_SHAPE_MESH) mesh = i;
    }
    assert(sphere < shapes.size() && polygon < shapes.size() && mesh < shapes.size() && !polygons.empty());
    with_shape(sphere, rm_shape_ref{RM_SHAPE_SPHERE, good.n_spheres, 1u, 0u}, "rm_scene_upload: bad sphere ref");
    with_shape(sphere, rm_shape_ref{RM_SHAPE_SPHERE, 0u, 2u, 0u}, "rm_scene_upload: bad sphere ref");
    with_shape(polygon, rm_shape_ref{RM_SHAPE_POLYGON, good.n_polygons, 1u, 0u}, "rm_scene_upload: bad polygon ref");
    with_shape(mesh, rm_shape_ref{RM_SHAPE_MESH, good.n_triangles, 1u, 0u}, "rm_scene_upload: bad mesh ref");
    with_shape(mesh, rm_shape_ref{RM_SHAPE_MESH, 0xFFFFFFFFu, 2u, 0u}, "rm_scene_upload: bad mesh ref");
    with_shape(sphere, rm_shape_ref{7u, 0u, 1u, 0u}, "rm_scene_upload: unknown shape kind");
    const uint32_t ranges[3][2] = {{0u, 2u}, {good.n_polygon_vertices - 1u, 3u}, {0xFFFFFFFFu, 3u}};
    for (const auto &range : ranges) {
        std::vector<rm_polygon> edited = polygons;
        edited[shapes[polygon].first].first_vertex = range[0];
        edited[shapes[polygon].first].n_vertices = range[1];
        rm_scene_desc d = good;
        d.polygons = edited.data();
        refused(d, "rm_scene_upload: bad polygon vertex range");
    }
    rm_scene_desc d = good;
    d.shapes = nullptr; refused(d, "rm_scene_upload: NULL array with non-zero count"); d = good;
    d.spheres = nullptr; refused(d, "rm_scene_upload: NULL array with non-zero count"); d = good;
    d.polygons = nullptr; refused(d, "rm_scene_upload: NULL array with non-zero count"); d = good;
    d.polygon_vertices = nullptr; refused(d, "rm_scene_upload: NULL array with non-zero count"); d = good;
    d.triangles = nullptr; refused(d, "rm_scene_upload: NULL array with non-zero count"); d = good;
    d.lights = nullptr; refused(d, "rm_scene_upload: NULL array with non-zero count");
}

// The shading launches' variant and grid: every outcome of the rule, the grid against the formula in 64-bit integers
static void check_shading_plan() {
    rm_knobs plain, generic, deep;
    generic.force_generic_pow = true;
    deep.force_stack = 32;
    for (uint32_t spheres : {0u, 512u})
        for (uint32_t triangles : {0u, 768u})
            for (bool integer : {false, true})
                for (uint32_t depth : {0u, 5u, 6u, (uint32_t)RM_MAX_DEPTH}) {
                    rm_dev_header H{};
                    H.off_bvh_spheres = spheres;
                    H.off_bvh_triangles = triangles;
                    const rm_shading_variant v = rm_shading_variant_of(plain, H, integer, depth);
                    assert(v.bvh == (spheres != 0u || triangles != 0u));
                    assert(v.pow_mode == (integer ? rmdev::POW_INTEGER : rmdev::POW_GENERIC));
                    assert(v.stack == (depth <= 5u ? 4 : 32));
                    const rm_shading_variant g = rm_shading_variant_of(generic, H, integer, depth), d = rm_shading_variant_of(deep, H, integer, depth);
                    assert(g.bvh == v.bvh && g.pow_mode == rmdev::POW_GENERIC && g.stack == v.stack);
                    assert(d.bvh == v.bvh && d.pow_mode == v.pow_mode && d.stack == v.stack);   // RM_FORCE_STACK changes nothing
                }
    for (uint32_t rays : {1u, 4u, 9u, 49u, 64u})
        for (uint32_t total : {1u, 63u, 64u, 65u, 0x7fffffffu})
            for (uint32_t cap : {0u, 1u, 3u})
                for (int n_cus : {0, 1, 256})
                    for (int per_cu : {1, 8}) {
                        const uint64_t group = 64u / rays;
                        uint64_t g = std::min<uint64_t>((total + group - 1u) / group, (uint64_t)std::max(1, n_cus) * (uint64_t)per_cu);
                        if (cap) g = std::min<uint64_t>(g, cap);
                        assert(rm_shading_grid(total, rays, n_cus, per_cu, cap) == std::max<uint64_t>(g, 1u));
                    }
    assert(rm_shading_grid(0x7fffffffu, 64u, 1 << 20, 1 << 11, 0u) == 0x7fffffffu);
}

// A call the host arithmetic must refuse: RM_ERR_INVALID_ARG and a text that says what
template <class CALL>
static void refused_with(CALL call, const char *word) {
    rm_set_host_error("");
    assert(call() == RM_ERR_INVALID_ARG);
    assert(std::strstr(rm_last_error(nullptr), word) != nullptr);
}

// The three sequences: a slice is the same rows of the whole, the last row is 65535, nothing is touched for zero counts
static void check_sequences() {
    const double radii[2] = {1.5, 0.};
    const rm_vec3 vel[3] = {{1., -2., 0.5}, {0., 0., 0.}, {-0., 3., 1e-300}};
    const uint32_t whole = 40u, first = 7u, count = 13u;
    std::vector<double> lens(whole * 4u), lights(whole * 2u * 3u), shapes(whole * 3u * 3u);
    assert(rm_lens_sequence(0u, whole, lens.data()) == RM_OK);
    assert(rm_light_sequence(0u, whole, radii, 2u, lights.data()) == RM_OK);
    assert(rm_motion_sequence(0u, whole, vel, 3u, 0.75, shapes.data()) == RM_OK);
    std::vector<double> a(count * 4u), b(count * 2u * 3u), c(count * 3u * 3u);
    assert(rm_lens_sequence(first, count, a.data()) == RM_OK && std::memcmp(a.data(), &lens[first * 4u], a.size() * sizeof(double)) == 0);
    assert(rm_light_sequence(first, count, radii, 2u, b.data()) == RM_OK && std::memcmp(b.data(), &lights[first * 6u], b.size() * sizeof(double)) == 0);
    assert(rm_motion_sequence(first, count, vel, 3u, 0.75, c.data()) == RM_OK && std::memcmp(c.data(), &shapes[first * 9u], c.size() * sizeof(double)) == 0);
    for (double x : lens) assert(std::isfinite(x));
    // the range: row 65535 and first + count = 65536 pass, 65537 and a first that would wrap do not
    const uint32_t most = RM_PROGRESSIVE_MAX_SAMPLES;
    std::vector<double> tail(6u * 9u);
    assert(rm_lens_sequence(most - 1u, 1u, tail.data()) == RM_OK && rm_lens_sequence(most - 6u, 6u, tail.data()) == RM_OK);
    assert(rm_light_sequence(most - 1u, 1u, radii, 2u, tail.data()) == RM_OK && rm_light_sequence(most - 6u, 6u, radii, 2u, tail.data()) == RM_OK);
    assert(rm_motion_sequence(most - 1u, 1u, vel, 3u, 1., tail.data()) == RM_OK && rm_motion_sequence(most - 6u, 6u, vel, 3u, 1., tail.data()) == RM_OK);
    const uint32_t beyond[2][2] = {{most - 6u, 7u}, {0xFFFFFFFFu, 1u}};
    for (const auto &r : beyond) {
        refused_with([&]() { return rm_lens_sequence(r[0], r[1], tail.data()); }, "rm_lens_sequence: first + count");
        refused_with([&]() { return rm_light_sequence(r[0], r[1], radii, 2u, tail.data()); }, "rm_light_sequence: first + count");
        refused_with([&]() { return rm_motion_sequence(r[0], r[1], vel, 3u, 1., tail.data()); }, "rm_motion_sequence: first + count");
    }
    // zero counts: no pointer is looked at
    assert(rm_lens_sequence(0u, 0u, nullptr) == RM_OK && rm_lens_sequence(most, 0u, nullptr) == RM_OK);
    assert(rm_light_sequence(5u, 0u, nullptr, 2u, nullptr) == RM_OK && rm_light_sequence(5u, 3u, nullptr, 0u, nullptr) == RM_OK);
    assert(rm_motion_sequence(5u, 0u, nullptr, 3u, NAN, nullptr) == RM_OK && rm_motion_sequence(5u, 3u, nullptr, 0u, NAN, nullptr) == RM_OK);
    // every other refusal
    refused_with([&]() { return rm_lens_sequence(0u, 1u, nullptr); }, "NULL table");
    refused_with([&]() { return rm_light_sequence(0u, 1u, nullptr, 2u, tail.data()); }, "NULL radii");
    refused_with([&]() { return rm_light_sequence(0u, 1u, radii, 2u, nullptr); }, "NULL offsets");
    for (double bad : {-1e-300, (double)NAN, (double)INFINITY}) {
        const double r[2] = {1., bad};
        refused_with([&]() { return rm_light_sequence(0u, 1u, r, 2u, tail.data()); }, "radii[1]");
        refused_with([&]() { return rm_motion_sequence(0u, 1u, vel, 3u, bad, tail.data()); }, "shutter");
    }
    refused_with([&]() { return rm_motion_sequence(0u, 1u, nullptr, 3u, 1., tail.data()); }, "NULL velocities");
    refused_with([&]() { return rm_motion_sequence(0u, 1u, vel, 3u, 1., nullptr); }, "NULL offsets");
    for (int axis = 0; axis < 3; axis++) {
        rm_vec3 v[3] = {vel[0], vel[1], vel[2]};
        (axis == 0 ? v[2].x : axis == 1 ? v[2].y : v[2].z) = axis == 1 ? (double)NAN : (double)INFINITY;
        refused_with([&]() { return rm_motion_sequence(0u, 1u, v, 3u, 1., tail.data()); }, "velocities[2]");
    }
}

// The frame identity: equal to itself, unequal after every single change
static void check_identity() {
    rm_params p{};
    p.fov = 1.5; p.half_fov = 0.75; p.height = 32.; p.width = 64.; p.ratio = 2.;
    p.frame_width = 64u; p.frame_height = 32u; p.max_depth = 3u; p.patch_size = 32u;
    p.background = rm_vec3{0.1, 0.2, 0.3};
    const rm_lens lens{0.4, 5., 8u, 0u};
    const rm_vec3 camera{1., 2., 3.};
    const rm_camera_basis basis{{1., 0., 0.}, {0., 1., 0.}, {0., 0., -1.}};
    const double radii[2] = {1.5, 3.};
    const rm_vec3 vel[2] = {{1., 0., 0.}, {0., 0., 0.}};
    rm_sampling_rules rules;
    rules.soft = true; rules.radii = radii; rules.n_lights = 2u;
    rules.motion = true; rules.velocities = vel; rules.n_shapes = 2u; rules.shutter = 1.;
    const rm_frame_identity base = rm_frame_identity_of(p, lens, camera, basis, false, 7u, rules);
    assert(rm_same_frame(base, base) && rm_same_frame(base, rm_frame_identity_of(p, lens, camera, basis, false, 7u, rules)));
    assert(base.radii.size() == 2u && base.velocities.size() == 2u);
    int changes = 0;
    auto differs = [&](const rm_frame_identity &other) {
        assert(!rm_same_frame(base, other) && !rm_same_frame(other, base) && rm_same_frame(other, other));
        changes++;
    };
    // every key field: the params', the lens', the camera, the basis, the oriented flag, the upload count
    double rm_params::*const doubles[] = {&rm_params::fov, &rm_params::half_fov, &rm_params::height, &rm_params::width, &rm_params::ratio};
    for (auto m : doubles) { rm_params q = p; q.*m += 0.25; differs(rm_frame_identity_of(q, lens, camera, basis, false, 7u, rules)); }
    uint32_t rm_params::*const words[] = {&rm_params::frame_width, &rm_params::frame_height, &rm_params::max_depth};
    for (auto m : words) { rm_params q = p; q.*m += 1u; differs(rm_frame_identity_of(q, lens, camera, basis, false, 7u, rules)); }
    double rm_vec3::*const axes[] = {&rm_vec3::x, &rm_vec3::y, &rm_vec3::z};
    for (auto m : axes) {
        rm_params q = p; q.background.*m += 0.5; differs(rm_frame_identity_of(q, lens, camera, basis, false, 7u, rules));
        rm_vec3 cam = camera; cam.*m += 0.5; differs(rm_frame_identity_of(p, lens, cam, basis, false, 7u, rules));
        rm_camera_basis t = basis; t.right.*m += 0.5; differs(rm_frame_identity_of(p, lens, camera, t, false, 7u, rules));
        t = basis; t.up.*m += 0.5; differs(rm_frame_identity_of(p, lens, camera, t, false, 7u, rules));
        t = basis; t.forward.*m += 0.5; differs(rm_frame_identity_of(p, lens, camera, t, false, 7u, rules));
    }
    differs(rm_frame_identity_of(p, rm_lens{0.5, 5., 8u, 0u}, camera, basis, false, 7u, rules));
    differs(rm_frame_identity_of(p, rm_lens{0.4, 6., 8u, 0u}, camera, basis, false, 7u, rules));
    differs(rm_frame_identity_of(p, lens, camera, basis, true, 7u, rules));
    differs(rm_frame_identity_of(p, lens, camera, basis, false, 8u, rules));
    assert(changes == 8 + 15 + 4);
    // ... what is not in the key: the samples a tick, the band, the flags
    rm_params q = p; q.flags = 1u; q.patch_row_begin = 1u;
    assert(rm_same_frame(base, rm_frame_identity_of(q, rm_lens{0.4, 5., 4u, 0u}, camera, basis, false, 7u, rules)));
    // the rules: one radius, the radii's count, one velocity component, -0. for 0., the shutter
    auto with = [&](const rm_sampling_rules &r) { return rm_frame_identity_of(p, lens, camera, basis, false, 7u, r); };
    const double other_radii[2] = {1.5, 2.};
    rm_sampling_rules r = rules; r.radii = other_radii; differs(with(r));
    assert(!rm_same_radii(base, with(r)) && rm_same_radii(base, base));
    r = rules; r.n_lights = 1u; differs(with(r));
    for (auto m : axes) {
        rm_vec3 v[2] = {vel[0], vel[1]};
        v[1].*m = 1e-300;
        r = rules; r.velocities = v; differs(with(r));
        v[1].*m = -0.;
        r = rules; r.velocities = v; differs(with(r));
    }
    r = rules; r.n_shapes = 1u; differs(with(r));
    r = rules; r.shutter = 0.5; differs(with(r));
    // "no radii" is not "zero lights' worth of radii", "no velocities" not "velocities of zero" (nor none of them)
    rm_sampling_rules none, no_lights, still, no_shapes;
    no_lights.soft = true;
    const rm_vec3 zero[2] = {{0., 0., 0.}, {0., 0., 0.}};
    still.motion = true; still.velocities = zero; still.n_shapes = 2u;
    no_shapes.motion = true;
    assert(rm_same_frame(with(none), with(none)) && !rm_same_frame(with(none), with(no_lights)) && rm_same_radii(with(none), with(no_lights)));
    assert(!rm_same_frame(with(none), with(still)) && !rm_same_frame(with(none), with(no_shapes)) && !rm_same_frame(with(still), with(no_shapes)));
}

// The staging rule: point lights or radii, with and without motion, on scenes with and without lights and spheres
static void check_staging() {
    const double radii[2] = {1., 2.};
    const rm_vec3 vel[5] = {};
    for (uint32_t scene_lights : {0u, 2u})
        for (uint32_t scene_spheres : {0u, 3u})
            for (bool soft : {false, true})
                for (bool motion : {false, true}) {
                    const uint32_t scene_shapes = scene_spheres + 2u;  // (two shapes that are not spheres)
                    rm_sampling_rules r;
                    if (soft) { r.soft = true; r.radii = radii; r.n_lights = scene_lights; }
                    if (motion) { r.motion = true; r.velocities = vel; r.n_shapes = scene_shapes; r.shutter = 1.; }
                    const rm_staging a = rm_staging_of(RM_TICK_PROGRESSIVE, r, scene_lights, scene_spheres, scene_shapes);
                    const rm_staging c = rm_staging_of(RM_TICK_CONVERGING, r, scene_lights, scene_spheres, scene_shapes);
                    assert(a.light_columns == (soft || motion ? scene_lights : 0u) && c.light_columns == a.light_columns);
                    assert(a.light_zeros == (motion && !soft) && c.light_zeros == a.light_zeros);
                    assert(a.shape_columns == (motion ? scene_shapes : 0u));
                    assert(c.shape_columns == (motion && scene_spheres > 0u ? scene_shapes : 0u));   // the one difference
                    // the rows the rule asks for are what the fill functions write: not a double more
                    std::vector<double> rows(3u * (a.light_columns + a.shape_columns) * 3u + 1u, 7.);
                    double *end = rows.data() + 3u * a.light_columns * 3u;
                    if (a.light_columns > 0u) assert(rm_fill_light_rows(r, a, 4u, 3u, rows.data()) == RM_OK);
                    if (a.shape_columns > 0u) assert(rm_fill_shape_rows(r, 4u, 3u, end) == RM_OK);
                    assert(rows.back() == 7.);
                    for (size_t i = 0; i + 1u < rows.size(); i++) assert(rows[i] != 7. && (!a.light_zeros || rows[i] == 0.));
                }
    double lens[8];
    assert(rm_fill_lens_rows(3u, 2u, lens) == RM_OK && lens[0] == 0.75 && lens[4] == 0.125);   // (rows 3 and 4 in base 2)
}

int main(int argc, char **argv) {
    assert(argc >= 3);
    const std::string cornell = argv[1], tmpdir = argv[2];
    rm_scene *s = nullptr;
    assert(rm_scene_create_default(&s) == RM_OK);
    rm_scene_desc d;
    assert(rm_scene_get_desc(s, &d) == RM_OK);
    assert(d.n_shapes == 6 && d.n_lights == 2 && d.n_polygon_vertices == 7);
    check_image(d);
    rm_vec3 off = {1., 2., 3.};
    assert(rm_scene_offset_shape(s, 5, off) == RM_OK);
    assert(rm_scene_offset_shape(s, 0, off) == RM_ERR_INVALID_ARG);
    assert(rm_scene_offset_shape(s, 77, off) == RM_ERR_INVALID_ARG);
    assert(rm_scene_offset_camera(s, off) == RM_OK);
    rm_reflectance r;
    rm_reflectance_default(&r);
    std::vector<rm_vec3> poly;
    for (int i = 0; i < 9; i++) poly.push_back(rm_vec3{(double)i, (double)(i * i % 5), -10.});
    assert(rm_scene_add_polygon(s, poly.data(), (uint32_t)poly.size(), &r) == RM_OK);
    assert(rm_scene_add_polygon(s, poly.data(), 2, &r) == RM_ERR_INVALID_ARG);
    std::vector<double> tri(9 * 100);
    for (size_t i = 0; i < tri.size(); i++) tri[i] = (double)((i * 7919) % 101) - 50.;
    assert(rm_scene_add_mesh(s, tri.data(), 100, off) == RM_OK);
    assert(rm_scene_add_mesh(s, nullptr, 0, off) == RM_OK);
    assert(rm_scene_get_desc(s, &d) == RM_OK);
    assert(d.n_triangles == 100 && d.n_shapes == 9);
    check_image(d);                                                     // (a hierarchy over its triangles; beyond the masks' 64 pids)
    check_refusals(d);
    rm_scene_free(s);

    rm_scene *c = nullptr;
    assert(rm_scene_open_obj(cornell.c_str(), &c) == RM_OK);
    assert(rm_scene_get_desc(c, &d) == RM_OK);
    assert(d.n_shapes == 8 && d.n_triangles == 36 && d.n_lights == 2);
    check_image(d);
    rm_scene_free(c);

    // malformed inputs: every one must come back as a status, never as a crash
    const char *bad[] = {
        "f 1 2 3\n",                                   // face before any vertex
        "v 0 0\nf 1 1 1\n",                            // short vertex
        "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n",        // index out of range
        "v 0 0 0\nv 1 0 0\nv 0 1 0\nf -4 -1 -2\n",     // negative index out of range
        "v 0 0 0\nv 1 0 0\nv 0 1 0\nf a b c\n",        // not a number
        "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1/ 2/x 3\n",     // odd separators
        "usemtl\nv 0 0 0\n",                           // usemtl without a name
        "mtllib\n",                                    // mtllib without a file
        "o empty\n",                                   // no faces at all
        "v 1e999 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n",    // overflowing float
        "",                                            // empty file
    };
    int n_ok = 0;
    for (size_t i = 0; i < sizeof bad / sizeof bad[0]; i++) {
        const std::string path = tmpdir + "/bad" + std::to_string(i) + ".obj";
        FILE *f = std::fopen(path.c_str(), "w");
        std::fputs(bad[i], f);
        std::fclose(f);
        rm_scene *b = nullptr;
        assert(rm_scene_new(&b) == RM_OK);
        uint32_t n = 0;
        const rm_status st = rm_scene_load_obj(b, path.c_str(), off, &n);
        if (st == RM_OK) n_ok++;
        else assert(std::strlen(rm_last_error(nullptr)) > 0);
        rm_scene_free(b);
    }
    // Spheres whose radii double along a line: the surface-area split peels one off per level
    // (depth ~ count); the builder must switch to median splits and stay under the stack bound.
    for (uint32_t leaf : {1u, 2u, 4u}) {
        const uint32_t n = 400;
        std::vector<rm_aabb> boxes(n);
        double x = 0., r = 1e-30;
        for (uint32_t i = 0; i < n; i++) {
            x += 3. * r;
            for (int a = 0; a < 3; a++) { boxes[i].lo[a] = (a == 0 ? x : 0.) - r; boxes[i].hi[a] = (a == 0 ? x : 0.) + r; }
            r *= 2.;
        }
        const rm_bvh h = rm_build_bvh(boxes, leaf);
        assert(h.depth > RM_BVH_SAH_DEPTH && h.depth <= RM_BVH_SAH_DEPTH + 10u);
        std::vector<int> seen(n, 0);
        walk_hierarchy(h, boxes, 0, nullptr, leaf, seen, 0);
        for (int c : seen) assert(c == 1);
    }
    check_hierarchy(1, 4);
    check_hierarchy(5, 4);
    check_hierarchy(257, 4);
    check_hierarchy(1000, 2);
    check_hierarchy(64, 1);
    check_shading_plan();
    check_sequences();
    check_identity();
    check_staging();
    char buf[8];
    assert(rm_format_status(buf, sizeof buf, 92, 1280, 800) > 7);   // truncated, NUL-terminated
    assert(buf[7] == '\0');
    std::printf("host sanitize ok (%d of the malformed files were acceptable to the loader)\n", n_ok);
    return 0;
}
