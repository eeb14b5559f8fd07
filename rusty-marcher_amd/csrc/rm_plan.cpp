// rm_plan.cpp -- the knobs' table, the kernel choice and the launch plan (rm_plan.hpp).  Host arithmetic only: no device
// header is included here, so nothing in this unit can touch one.
#include "rm_plan.hpp"
#include "rm_image.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace rmdev;

// ---------------------------------------------------------------------------
// Knobs
// ---------------------------------------------------------------------------
namespace {

// How a knob's text becomes its value.  The differences are behaviour: RM_X=2 switches an IS_1 knob off and leaves a
// NOT_0 knob on.
enum knob_rule {
    IS_1,          // bool: text[0] == '1'
    NOT_0,         // bool: text[0] != '0'
    IS_SET,        // bool: the variable exists
    ONE_OR_ZERO,   // int: text[0] == '1' ? 1 : 0 (unset: the field's -1)
    ATOI,          // int: atoi
    ATOI_MIN_0,    // int / uint32_t: max(0, atoi)
    ATOI_MIN_1,    // uint32_t: max(1, atoi)
    STRTOUL,       // uint32_t: strtoul, base 10
    TILE_ORDER,    // int: "reverse" | "hash" | anything else: natural
    TAIL_PLACE,    // int: "ev..." 1 | "e..." 2 | anything else 0
    CULL_OFF,      // double: text[0] == '1' sets 2 (no bundle is ever narrow enough)
    CULL_COS,      // double: max(0.05, atof)   (the cone tests hold for half-angles below 90 degrees)
    DEAD_CHILDREN, // bool: text[0] != '0'; and early_fates: text[0] is neither '0' nor '1'
};

struct knob {
    const char *name;
    knob_rule rule;
    bool rm_knobs::*b = nullptr;
    int rm_knobs::*i = nullptr;
    uint32_t rm_knobs::*u = nullptr;
    double rm_knobs::*d = nullptr;
    constexpr knob(const char *n, bool rm_knobs::*f, knob_rule r) : name(n), rule(r), b(f) {}
    constexpr knob(const char *n, int rm_knobs::*f, knob_rule r) : name(n), rule(r), i(f) {}
    constexpr knob(const char *n, uint32_t rm_knobs::*f, knob_rule r) : name(n), rule(r), u(f) {}
    constexpr knob(const char *n, double rm_knobs::*f, knob_rule r) : name(n), rule(r), d(f) {}
};

// (in order: RM_DISABLE_CULL sets cull_cos before RM_CULL_COS may override it)
const knob k_knobs[] = {
    {"RM_FORCE_GENERIC_POW", &rm_knobs::force_generic_pow, IS_1},
    {"RM_FORCE_FAST_FP", &rm_knobs::force_fast_fp, IS_1},
    {"RM_FORCE_UNSTAGED", &rm_knobs::force_unstaged, IS_1},
    {"RM_SHADOW_MASKS", &rm_knobs::shadow_masks, NOT_0},
    {"RM_DEAD_CHILDREN", &rm_knobs::dead_children, DEAD_CHILDREN},
    {"RM_SCENE_SIG", &rm_knobs::scene_sig, NOT_0},
    {"RM_DISABLE_BVH", &rm_knobs::disable_bvh, IS_1},
    {"RM_SWEPT_BVH", &rm_knobs::swept_bvh, NOT_0},
    {"RM_FORCE_STACK", &rm_knobs::force_stack, ATOI},
    {"RM_FEEDBACK", &rm_knobs::feedback_mode, ONE_OR_ZERO},
    {"RM_FEEDBACK_US", &rm_knobs::feedback_us, ATOI_MIN_1},
    {"RM_FEEDBACK_TARGET", &rm_knobs::feedback_target, ATOI_MIN_0},
    {"RM_DEBUG_EMPTY", &rm_knobs::debug_empty, IS_1},
    {"RM_TILE_CLASSIFY", &rm_knobs::classify_mode, ONE_OR_ZERO},
    {"RM_CLASSIFY_IN_LAUNCH", &rm_knobs::classify_in_launch, IS_1},
    {"RM_PATCH_ORDER", &rm_knobs::patch_order_mode, ONE_OR_ZERO},
    {"RM_SKY_TAIL", &rm_knobs::sky_tail, NOT_0},
    {"RM_SKY_TAIL_FORCE", &rm_knobs::sky_tail_force, ATOI},
    {"RM_PATCH_ORDER_MAX", &rm_knobs::patch_order_max, ATOI_MIN_0},
    {"RM_SKY_TAIL_BIG", &rm_knobs::sky_tail_big, NOT_0},
    {"RM_PATCH_ORDER_MAX_DEEP", &rm_knobs::patch_order_max_deep, ATOI_MIN_0},
    {"RM_SKY_TAIL_ROOM_DIV", &rm_knobs::sky_tail_room_div, ATOI_MIN_1},
    {"RM_SKY_TAIL_BIG_MIN", &rm_knobs::sky_tail_big_min, ATOI_MIN_0},
    {"RM_SKY_TAIL_PLACE", &rm_knobs::sky_tail_place, TAIL_PLACE},
    {"RM_SKY_TAIL_MOTION", &rm_knobs::sky_tail_motion, NOT_0},
    {"RM_SKY_TAIL_CAP", &rm_knobs::sky_tail_cap, ATOI_MIN_0},
    {"RM_ORDER_KEYS", &rm_knobs::order_keys, ATOI},
    {"RM_FIRST_ROUND", &rm_knobs::first_round, ATOI_MIN_0},
    {"RM_FIRST_ROUND_FROM_ORDER", &rm_knobs::first_round_from_order, NOT_0},
    {"RM_ORDER_REUSE", &rm_knobs::order_reuse, NOT_0},
    {"RM_STATIC_ROUNDS", &rm_knobs::static_rounds, ATOI_MIN_1},
    {"RM_CLS_MAX_BLOCKS", &rm_knobs::cls_max_blocks, ATOI_MIN_1},
    {"RM_ORDER_FREEZE", &rm_knobs::order_freeze, ATOI_MIN_0},
    {"RM_ORDER_LATE_PLACES", &rm_knobs::order_late_places, NOT_0},
    {"RM_MASK_REUSE", &rm_knobs::mask_reuse, NOT_0},
    {"RM_CLASSIFY_LDS", &rm_knobs::classify_lds, NOT_0},
    {"RM_CLASSIFY_IN_LAUNCH_PRIMS", &rm_knobs::classify_in_launch_prims, ATOI_MIN_0},
    {"RM_CLASSIFY_MIN_TILES", &rm_knobs::classify_min_tiles, ATOI_MIN_0},
    {"RM_ORD_TAG_WRAP", &rm_knobs::ord_tag_wrap, ATOI_MIN_1},
    {"RM_TEST_STALL_ORDER", &rm_knobs::test_stall_order, ATOI},
    {"RM_TILE_ORDER", &rm_knobs::tile_order, TILE_ORDER},
    {"RM_DISABLE_CULL", &rm_knobs::cull_cos, CULL_OFF},
    {"RM_CULL_COS", &rm_knobs::cull_cos, CULL_COS},
    {"RM_CULL_MIN", &rm_knobs::cull_min_prims, STRTOUL},
    {"RM_CULL_EDGES", &rm_knobs::cull_edges, NOT_0},
    {"RM_CHECKED_NUMERICS", &rm_knobs::checked_numerics, NOT_0},
    {"RM_REFINE_MAX_BLOCKS", &rm_knobs::refine_max_blocks, ATOI_MIN_0},
    {"RM_LENS_MAX_BLOCKS", &rm_knobs::lens_max_blocks, ATOI_MIN_0},
    {"RM_DEBUG_TAIL", &rm_knobs::debug_tail, IS_SET},
};

}  // namespace

rm_knobs rm_knobs_from_env() {
    rm_knobs kn;
    for (const knob &k : k_knobs) {
        const char *env = std::getenv(k.name);
        if (!env) continue;
        switch (k.rule) {
        case IS_1: kn.*k.b = env[0] == '1'; break;
        case NOT_0: kn.*k.b = env[0] != '0'; break;
        case IS_SET: kn.*k.b = true; break;
        case ONE_OR_ZERO: kn.*k.i = env[0] == '1' ? 1 : 0; break;
        case ATOI: kn.*k.i = std::atoi(env); break;
        case ATOI_MIN_0:
            if (k.i) kn.*k.i = std::max(0, std::atoi(env));
            else kn.*k.u = (uint32_t)std::max(0, std::atoi(env));
            break;
        case ATOI_MIN_1: kn.*k.u = (uint32_t)std::max(1, std::atoi(env)); break;
        case STRTOUL: kn.*k.u = (uint32_t)std::strtoul(env, nullptr, 10); break;
        case TILE_ORDER:
            kn.*k.i = !std::strcmp(env, "reverse") ? TILE_ORDER_REVERSE : !std::strcmp(env, "hash") ? TILE_ORDER_HASH : TILE_ORDER_NATURAL;
            break;
        case TAIL_PLACE: kn.*k.i = env[0] == 'e' && env[1] == 'v' ? 1 : env[0] == 'e' ? 2 : 0; break;
        case CULL_OFF: kn.*k.d = env[0] == '1' ? 2. : kn.*k.d; break;
        case CULL_COS: kn.*k.d = std::max(0.05, std::atof(env)); break;
        case DEAD_CHILDREN: kn.*k.b = env[0] != '0'; kn.early_fates = env[0] != '0' && env[0] != '1'; break;
        }
    }
    if (kn.classify_min_tiles == 0u) kn.classify_min_tiles = RM_CLASSIFY_MIN_TILES_DEFAULT;
    return kn;
}

// ---------------------------------------------------------------------------
// The kernel
// ---------------------------------------------------------------------------

// Scenes up to this size get a copy in every workgroup's LDS for the per-lane gathers;
// larger ones are read from global memory only (the primitive loops always are, through
// scalar loads).  Measured: the LDS copy is worth 2 % on the 1.3 KB demo scene (81.3 vs
// 82.8 us), nothing on the 7.6 KB cornell box (153 vs 150 us) and costs 20 % on the 29 KB
// synthetic scene (10.5 vs 8.7 ms: every workgroup re-stages the blob).
// RM_ERR_SCENE_LIMIT is left for what the blob's 32-bit word offsets cannot address.
static constexpr size_t RM_LDS_SCENE_LIMIT_BYTES = RM_LDS_SCENE_LIMIT_WORDS * sizeof(double);   // (4 KB)
static constexpr uint32_t RM_FEEDBACK_MIN_TILES = 32768;
// What a lane of the classification spends on its share of a patch's primitives, in vector instructions: ~22
// per bounding sphere, ~110 more for the edge and plane tests of a planar primitive.  Beyond this the launch
// is not worth its time.
static constexpr uint32_t RM_CLASSIFY_MAX_COST = 4000;
// ... and at the head of the render launch itself, where every wave behind the first round may wait for it: a quarter of that
static constexpr uint32_t RM_CLASSIFY_IN_LAUNCH_MAX_COST = 1000;

uint32_t rm_scene_signature(const rm_dev_header &H, const double *blob) {
    if (H.off_bvh_spheres != 0u || H.off_bvh_triangles != 0u || !blob) return 0u;
    for (uint32_t s = 0; s < RM_SCENE_SIG_COUNT; s++) {
        const SceneSignature &g = RM_SCENE_SIGNATURES[s];
        bool match = H.n_spheres == g.n_spheres && H.n_polygons == g.n_polygons && H.n_triangles == g.n_triangles &&
                     H.n_lights == g.n_lights && H.list_ordered == g.list_ordered && H.n_polygons <= sizeof g.polygon_nv;
        for (uint32_t i = 0; match && i < H.n_polygons; i++) {
            uint32_t first_and_count[2];                              // the polygon record's seventh word (rm_internal.h)
            std::memcpy(first_and_count, blob + H.off_polygons + (size_t)RM_POLYGON_WORDS * i + 6u, sizeof first_and_count);
            match = first_and_count[1] == g.polygon_nv[i];
        }
        if (match) return s + 1u;
    }
    return 0u;
}

bool choose_kernel(const rm_knobs &kn, const rm_plan_scene &sc, const rm_params &p, uint32_t tiles, rm_kernel_choice *k) {
    const rm_dev_header &H = *sc.H;
    // launch geometry: one tile per wave, one wave per workgroup; small scenes get an LDS copy
    // of the scene for the per-lane gathers, larger ones none
    const size_t scene_bytes = (size_t)H.total_words * sizeof(double);
    const uint32_t n_prims = k->n_prims = H.n_spheres + H.n_polygons + H.n_triangles;
    const uint32_t n_planar = k->n_planar = H.n_polygons + H.n_triangles;
    k->classify_cost = (22u * n_prims + 110u * n_planar) / 16u;   // a lane's share of the patch step
    k->bvh = H.off_bvh_spheres != 0 || H.off_bvh_triangles != 0;
    k->staged = scene_bytes <= RM_LDS_SCENE_LIMIT_BYTES && !kn.force_unstaged && !k->bvh;
    // Bundle culling pays from about a dozen primitives on (a cull step costs about what two
    // primitive tests cost); the six primitives of the demo scene are walked as they are.
    k->cull = n_prims >= kn.cull_min_prims || !k->staged;
    // One wave per workgroup in every kernel: the waves of a workgroup share nothing but the LDS
    // scene copy (which only small scenes get), and a wave slot a workgroup of four has freed is
    // handed on only when the whole workgroup fits -- with tiles of 1 to 18 ray steps that kept
    // 2.6 of a SIMD's 4 slots filled on the 256-sphere scene (1,777 -> 1,425 us with one wave).
    k->mode.waves = 1;
    k->mode.per_wave = 1;
    k->lds_bytes = ((k->staged ? (size_t)H.total_words : 0u) + (size_t)k->mode.waves * RM_WAVE_LDS_WORDS) * sizeof(double);

    // A lane parks at most one sibling per level below the cap: max_depth - 1 entries.
    k->stack = p.max_depth <= 5 ? 4 : p.max_depth <= 9 ? 8 : p.max_depth <= 17 ? 16 : 32;
    if (kn.force_stack > k->stack && (kn.force_stack == 8 || kn.force_stack == 16 || kn.force_stack == 32)) k->stack = kn.force_stack;
    k->pow_mode = (sc.integer_exponents && !kn.force_generic_pow) ? POW_INTEGER : POW_GENERIC;
    k->fast = (p.flags & RM_FLAG_FAST_FP) != 0 || kn.force_fast_fp;
    // the cull's edge test for planar primitives where there are several of them
    k->planar_edges = n_planar >= RM_CULL_EDGES_MIN_PLANAR;
    k->edges = k->cull && kn.cull_edges && k->planar_edges;
    const int st = k->stack, pw = k->pow_mode;
    const bool f = k->fast;
    // Feedback where tile costs have a long tail: deep ray trees in scenes with a hierarchy (a
    // step of incoherent rays through it costs thirty coherent ones) and launches long enough for
    // a tail to matter.  Elsewhere a tile costs its ray steps, the expensive rows are known (the
    // ground: dispatched first) and the bookkeeping only costs -- measured with it forced on: demo
    // scene 1080p 85.0 -> 87.7 us, 4K 306 -> 328, 8K depth 8 1,205 -> 1,375, Cornell box 72 -> 77.
    // RM_FEEDBACK=1 forces it for every launch of a kernel with the hierarchy walk, =0 switches it off.
    // r4: scenes with a hierarchy take the dispatch order from the launch's own classification instead where that can run
    // at the launch's head (patches timed by their longest tile, the sky tail on top): 256 spheres 4096x4096 1,174-1,185 ->
    // 1,160 us.  The tile-level feedback stays for what is left (RM_FEEDBACK=1 forces it).
    k->order_in_big_scene = k->bvh && kn.patch_order_mode != 0 && kn.feedback_mode != 1 && !kn.debug_empty && kn.classify_mode != 0 &&
                            kn.classify_in_launch && kn.tile_order == TILE_ORDER_REVERSE && k->classify_cost <= RM_CLASSIFY_IN_LAUNCH_MAX_COST &&
                            tiles / 16u <= kn.patch_order_max_deep && (kn.patch_order_mode == 1 || tiles >= kn.classify_min_tiles);
    // (an oriented launch never carries it: the oriented kernels come without -- it takes the hierarchy kernels as they are)
    k->feedback = k->bvh && !k->order_in_big_scene && kn.feedback_mode != 0 && !kn.debug_empty && !sc.oriented &&
                  (kn.feedback_mode == 1 || (p.max_depth >= 6u && tiles >= RM_FEEDBACK_MIN_TILES));
    // the dispatch order: launches of up to 4,096 patches that do not carry the tile-level feedback (launches of more patches
    // than that may take the same kernels for the sky tail alone -- RM_SKY_TAIL_BIG=1: by place, below; r4: measured to buy
    // nothing any more, 8K 988.9 against 985.6 us for the kernels without)
    k->order = k->order_in_big_scene ||
               (kn.patch_order_mode != 0 && !k->feedback && !kn.debug_empty && kn.tile_order == TILE_ORDER_REVERSE &&
                (tiles / 16u <= kn.patch_order_max || (kn.sky_tail && kn.sky_tail_big && n_prims <= 56u && tiles / 16u >= kn.sky_tail_big_min)) &&
                (kn.patch_order_mode == 1 || tiles >= kn.classify_min_tiles));
    // (the oriented kernels are the ones with the dispatch order: a launch without one runs them with ord_cnt == NULL)
    k->fn = sc.oriented ? rm_pick_kernel_oriented(f, k->staged, k->bvh, k->cull, k->edges, st, pw)
                        : rm_pick_kernel(f, k->staged, k->bvh, k->cull, k->edges, k->order ? 1 : 0, k->feedback, st, pw);
    return k->fn != nullptr;
}

// The shading kernels' variant (rm_plan.hpp): the rules above for the hierarchy and the power, two stacks for the four -- and
// no look at RM_FORCE_STACK, which choose_kernel alone obeys.
rm_shading_variant rm_shading_variant_of(const rm_knobs &kn, const rm_dev_header &H, bool integer_exponents, uint32_t max_depth) {
    rm_shading_variant v;
    v.bvh = H.off_bvh_spheres != 0 || H.off_bvh_triangles != 0;
    v.pow_mode = (integer_exponents && !kn.force_generic_pow) ? POW_INTEGER : POW_GENERIC;
    v.stack = max_depth <= 5u ? 4 : 32;
    return v;
}

uint32_t rm_shading_grid(uint32_t total, uint32_t rays_per_pixel, int n_cus, int per_cu, uint32_t max_blocks) {
    const uint32_t P = 64u / rays_per_pixel;
    const uint64_t need = ((uint64_t)total + P - 1u) / P;
    uint64_t g = std::min<uint64_t>(need, (uint64_t)std::max(1, n_cus) * (uint64_t)per_cu);
    if (max_blocks > 0u) g = std::min<uint64_t>(g, max_blocks);
    return (uint32_t)std::max<uint64_t>(g, 1u);
}

// ---------------------------------------------------------------------------
// The launch
// ---------------------------------------------------------------------------

// args.*field = buf + bytes, once the launcher knows where buf is
template <class T>
static void point(rm_launch_plan &P, T *KernelArgs::*field, rm_buf buf, size_t bytes) {
    const char *at = reinterpret_cast<const char *>(&(P.args.*field));
    P.refs[P.n_refs++] = rm_arg_ref{(uint16_t)(at - reinterpret_cast<const char *>(&P.args)), buf, (uint32_t)bytes};
}

bool rm_camera_exact_only(const rm_plan_scene &sc) {
    bool ok = rm_checked_coord_ok(sc.camera.x) && rm_checked_coord_ok(sc.camera.y) && rm_checked_coord_ok(sc.camera.z);
    if (sc.oriented && sc.basis) {
        const rm_camera_basis &b = *sc.basis;
        for (const rm_vec3 &v : {b.right, b.up, b.forward}) ok = ok && rm_checked_coord_ok(v.x) && rm_checked_coord_ok(v.y) && rm_checked_coord_ok(v.z);
    }
    return !ok;
}

bool plan_launch(const rm_knobs &kn, const rm_plan_scene &sc, const rm_params &p, const rm_band &band, const rm_stream_state &before,
                 uint32_t order_cap, const rm_feedback_state &fb, unsigned long long hint, rm_launch_plan *out) {
    rm_launch_plan &P = *out;
    KernelArgs &a = P.args;
    const rm_dev_header &H = *sc.H;
    a.H = H;
    a.half_fov = p.half_fov; a.height = p.height; a.width = p.width; a.ratio = p.ratio;
    a.cam_x = sc.camera.x; a.cam_y = sc.camera.y; a.cam_z = sc.camera.z;
    const rm_camera_basis &cb = *sc.basis;                  // (the fixed view's own while the oriented state is off; its kernels do not read it)
    a.cam_rx = cb.right.x; a.cam_ry = cb.right.y; a.cam_rz = cb.right.z;
    a.cam_ux = cb.up.x; a.cam_uy = cb.up.y; a.cam_uz = cb.up.z;
    a.cam_fx = cb.forward.x; a.cam_fy = cb.forward.y; a.cam_fz = cb.forward.z;
    // (the occluder masks hold for hit points within 1e-7 of the scene's size of their primitives: a camera
    // far enough out to round its hit points coarser than that renders without them)
    if (!(std::fabs(sc.camera.x) + std::fabs(sc.camera.y) + std::fabs(sc.camera.z) <= sc.occ_camera_limit)) a.H.off_occ = 0u;
    a.bg_x = p.background.x; a.bg_y = p.background.y; a.bg_z = p.background.z;
    // checked numerics: the scene's verdict from its upload, the camera's here, the knob's on top (kernels without them do not look)
    P.exact_only = !kn.checked_numerics || sc.exact_only || rm_camera_exact_only(sc);
    a.exact_only = P.exact_only ? 1u : 0u;
    a.frame_width = p.frame_width;
    a.patch_row_begin = band.begin;
    a.patch_row_stride = band.stride;
    a.u8_compact = (p.flags & RM_FLAG_U8_COMPACT) ? 1u : 0u;
    a.f64_compact = (p.flags & RM_FLAG_F64_COMPACT) ? 1u : 0u;
    a.max_depth = p.max_depth;
    a.n_width = p.frame_width / RM_PATCH_SIZE;
    a.n_tiles = band.count() * a.n_width * 16u;
    // dispatch order: tile = (id * order_mul + order_add) % n_tiles, a bijection
    a.order_mul = 1; a.order_add = 0;
    if (kn.tile_order == TILE_ORDER_REVERSE && a.n_tiles > 1) {             // id -> n-1-id
        a.order_mul = a.n_tiles - 1; a.order_add = a.n_tiles - 1;
    } else if (kn.tile_order == TILE_ORDER_HASH && a.n_tiles > 2) {
        uint32_t mul = (uint32_t)(a.n_tiles * 0.6180339887) | 1u;
        auto gcd = [](uint32_t x, uint32_t y) { while (y) { uint32_t t = x % y; x = y; y = t; } return x; };
        while (gcd(mul, a.n_tiles) != 1) mul += 2;
        a.order_mul = mul % a.n_tiles;
    }

    if (!choose_kernel(kn, sc, p, a.n_tiles, &P.k)) return false;
    const rm_kernel_choice &k = P.k;
    const uint32_t n_prims = k.n_prims, n_planar = k.n_planar;
    // children that leave a planar primitive into an empty half-space are not walked (render_tile): the plain-walk kernels
    // only, and -- like the occluder masks -- only while the camera is near enough for its hit points to round far below
    // the offset such a child starts with
    // (... and, a bit of the same word, whether a refracted child's fate is decided before its ray is formed: the knob's alone)
    a.dead_children = ((kn.dead_children && !k.bvh && !k.cull && sc.dead_camera_limit > 0. &&
                        std::fabs(sc.camera.x) + std::fabs(sc.camera.y) + std::fabs(sc.camera.z) <= sc.dead_camera_limit) ? RM_DEAD_DROP : 0u) |
                      ((kn.early_fates && !k.bvh && !k.cull) ? RM_DEAD_EARLY_FATES : 0u);
    // (... and, in bits of the same word, the resident scene's signature: the kernels that carry a body for it take that body)
    if (kn.scene_sig && sc.scene_sig <= RM_SCENE_SIG_COUNT && rm_scene_sig_kernel(k.staged, k.bvh, k.cull))
        a.dead_children |= (sc.scene_sig & RM_SCENE_SIG_MASK) << RM_SCENE_SIG_SHIFT;
    // A cull step handles 64 primitives for ~25 vector instructions, ~110 when it holds planar
    // primitives and the edge test runs; a bundle pays for every step.  The hierarchy walk finds a
    // bundle's few primitives in a few hundred instructions whatever their number, so scenes whose
    // cull would cost more than that take the hierarchy only (2 = no bundle is ever narrow
    // enough).  Measured at 1080p: 36 triangles cull 67 us / hierarchy 110; 320 triangles
    // 190 / 119; 1,280 triangles 389 / 155; 256 spheres + 1 quad 1.76 ms / 2.77.
    const uint32_t cull_steps = (n_prims + 63u) / 64u;
    const uint32_t planar_steps = n_planar ? cull_steps - H.n_spheres / 64u : 0u;   // (the first planar primitive's pid: n_spheres)
    const uint32_t cull_cost = 25u * cull_steps + (k.planar_edges ? 85u * planar_steps : 0u);
    a.cull_cos = cull_cost > RM_CULL_MAX_COST ? 2. : kn.cull_cos;
    // the launch's first round -- the waves resident at once -- does not wait for its tiles' classification (Cornell, whose
    // edge-test kernel holds three waves to a SIMD: 31.5 -> 30.8 us with 3,072 instead of 4,096)
    a.first_round = sc.n_cus * 4u * (k.edges ? RM_EDGES_WAVES : RM_MIN_WAVES);
    if (kn.first_round >= 0) a.first_round = (uint32_t)kn.first_round;     // (RM_FIRST_ROUND: A/B knob, and how the tests reach the order in frames of a few thousand tiles)
    P.block = (uint32_t)k.mode.waves * 64u;
    P.lds_bytes = k.lds_bytes;
    const uint32_t per_wg = (uint32_t)(k.mode.waves * k.mode.per_wave);
    P.grid = (a.n_tiles + per_wg - 1) / per_wg;
    P.feedback = k.feedback && per_wg == 1u && !kn.debug_empty;
    if (P.feedback) {
        // (the sets are created, or cleared when the geometry or the scene changed: the first frame then has no list)
        const rm_feedback_layout L(a.n_tiles);
        rm_feedback_state &next = P.feedback_after;
        next.valid = true;
        next.key[0] = (uint64_t)a.n_tiles | ((uint64_t)p.frame_width << 32);
        next.key[1] = (uint64_t)band.begin | ((uint64_t)band.stride << 32);
        next.key[2] = sc.scene_epoch;
        next.n_tiles = a.n_tiles;
        const bool same = fb.valid && fb.n_tiles == a.n_tiles && std::memcmp(fb.key, next.key, sizeof fb.key) == 0;
        P.feedback_reset = !same;
        P.feedback_bytes = L.bytes();
        P.feedback_set_bytes = L.set_bytes;
        const int r = same ? fb.cur : 0, w = (r + 1) % 3, z = (r + 2) % 3;
        next.cur = w;
        point(P, &KernelArgs::fb_list, RM_BUF_FEEDBACK, L.list(r)); point(P, &KernelArgs::fb_count, RM_BUF_FEEDBACK, L.count(r));
        point(P, &KernelArgs::fb_flag, RM_BUF_FEEDBACK, L.flag(r)); point(P, &KernelArgs::fb_hist, RM_BUF_FEEDBACK, L.hist(r));
        point(P, &KernelArgs::fb_next_list, RM_BUF_FEEDBACK, L.list(w)); point(P, &KernelArgs::fb_next_count, RM_BUF_FEEDBACK, L.count(w));
        point(P, &KernelArgs::fb_next_flag, RM_BUF_FEEDBACK, L.flag(w)); point(P, &KernelArgs::fb_next_hist, RM_BUF_FEEDBACK, L.hist(w));
        point(P, &KernelArgs::fb_zero, RM_BUF_FEEDBACK, L.hist(z));
        point(P, &KernelArgs::fb_threshold, RM_BUF_FEEDBACK, L.threshold());
        a.fb_cap = L.cap;
        a.fb_long_ticks = kn.feedback_us * 100u;            // s_memrealtime: 100 MHz
        // longest-first scheduling needs the longest tiles first, a few per wave slot: the rest fill in
        const uint32_t slots = sc.n_cus * 16u;
        a.fb_target = kn.feedback_target >= 0 ? (uint32_t)kn.feedback_target : 4u * slots;
        a.fb_target = std::min(a.fb_target, L.cap / 2u);
        P.grid = a.n_tiles + L.cap;                         // ids [0, cap): the list; the rest: the tiles in order
    }
    if (kn.debug_empty) a.n_tiles = 0;   // RM_DEBUG_EMPTY=1: same grid, every wave exits after staging

    rm_stream_state s = before;          // the stream's bookkeeping as a launch that classifies leaves it
    uint32_t mask_tag_before = 0u;       // the tag the previous launch on this stream gave its tiles' words (0: none that this launch could take)
    uint32_t cls_words_wanted = 0u;
    // Tile classification in front of the render launch (rm_classify.hip): tiles whose primary rays can hit
    // nothing are filled there and never get a wave; the others are listed, with the primitives their primary
    // rays can reach.  Worth a launch of its own from a few thousand tiles on, in scenes whose primitives a
    // lane can get through.  Only the primary rays are concerned: frames are bit-identical with it off.
    P.classify = kn.classify_mode != 0 && !kn.debug_empty && per_wg == 1u && n_prims > 0u &&
                 k.classify_cost <= RM_CLASSIFY_MAX_COST && (kn.classify_mode == 1 || a.n_tiles >= kn.classify_min_tiles);
    if (P.classify) {
        // Scenes of up to 56 primitives are classified at the head of the render launch itself (its first
        // workgroups; the words carry the launch's tag): no launch of its own, no gap, and the classification
        // runs while the first round of tiles renders.  Measured at 1080p, demo scene: 82.6 us with the launch
        // in front, against 82.1 without any classification.  Larger scenes, and launches that carry the
        // frame-to-frame feedback, get the launch in front.
        // (RM_CLASSIFY_IN_LAUNCH_PRIMS: larger scenes too -- their words then only say whether there is anything to hit)
        const bool in_launch = kn.classify_in_launch && (n_prims <= kn.classify_in_launch_prims || k.order_in_big_scene) && !k.feedback;
        if (in_launch) {
            if (!s.tagged || s.tagged_tiles != a.n_tiles || s.tagged_scene != sc.scene_epoch || s.tag >= 255u) {
                // (a word is taken by its tag: after anything that could leave an old word with a tag in use, start afresh)
                P.clear_masks = true;
                s.tag = 0;
                s.tagged = true; s.tagged_tiles = a.n_tiles; s.tagged_scene = sc.scene_epoch;
            }
            a.mask_tag = ++s.tag;
            mask_tag_before = a.mask_tag > 1u ? a.mask_tag - 1u : 0u;     // (the previous launch's words are still there, under this tag)
            a.cls_blocks = (a.n_tiles / 16u + 3u) / 4u;
            a.cls_prims = n_prims;
            P.grid += a.cls_blocks;
            // Scenes too long for an LDS copy (the Cornell box: 36 triangles, 15 KB): the classifying workgroups pack what their
            // tests read -- bounds, lifted vertices, plane records: 4 n + 22 n_planar words -- into their LDS block, where there is
            // room for it at the kernel's occupancy (every workgroup of the launch is given the block: 16 to a CU, 12 in the
            // edge-test kernels, of 160 KB).  RM_CLASSIFY_LDS=0: from memory.
            // (decided where the launch's geometry is final, below: the workgroups' records lie behind the packed data)
            cls_words_wanted = (!k.staged && kn.classify_lds) ? 4u * n_prims + 22u * n_planar : 0u;
        } else {
            s.tagged = false;
            // sixteen lanes to a 32x32 patch, four patches to a wave
            P.cls_fn = sc.oriented ? rm_classify_kernel_oriented(n_planar > 0u) : rm_classify_kernel(n_planar > 0u);
            P.cls_grid = (a.n_tiles / 16u + 3u) / 4u;
            P.cls_args.n_prims = n_prims;
        }
        point(P, &KernelArgs::tile_mask, RM_BUF_MASKS, 0);
        a.mask_exact = n_prims <= (in_launch ? 56u : 64u) ? 1u : 0u;      // (a tagged word names 56 primitives, rm_classify.inc)
    }
    // Dispatch order from the launch's own classification, and the sky tail (KernelArgs::ord_*; rm_classify.inc place_patch /
    // order_slot / order_places, rm_render_kernel.inc order_entry / sky_tail_patch).  The reference renders only after the camera has moved
    // (main.rs:74-78): an order by place from earlier frames is stale exactly then (r3: demo 1080p 68.5 us standing, 78.7 with a
    // press before every frame).  The classifying workgroups at the launch's head give every patch behind the first round
    // one of sixteen keys -- by its longest tile's time in the previous frame while the view stands still, by the cost of what
    // it can reach (learned per primitive from earlier frames: it moves with the picture) once it has moved, the sky last.
    // Only the order of dispatch and the launch's geometry depend on any of it: every tile of every frame is rendered in full by
    // the same code, exactly once.
    const uint32_t n_patches = a.n_tiles / 16u;
    // (the waves that take their patches from the previous ranking and wait for no order: static_rounds times what is resident at
    // once -- those behind the first of them start when its tiles are done, their classification words are there by then)
    // (two rounds where the launch is at least four deep: a rank's share of a frame keeps one and its order.  Measured with a
    // press before every frame, 1 / 2 / 3 rounds: Cornell 38.9-40.0 / 37.2 / 38.8-38.9 us, standing 30.0-30.4 / 29.8-29.9 / 31.4;
    // demo within its noise)
    const uint64_t rounds = (uint64_t)a.first_round * kn.static_rounds * 2u <= a.n_tiles ? kn.static_rounds : 1u;
    a.n_static = (uint32_t)std::min<uint64_t>(((uint64_t)a.first_round * rounds) & ~15ull, a.n_tiles);
    const uint32_t n_dyn = n_patches - a.n_static / 16u;
    // the classifying workgroups wait for each other: they must all be resident, whatever the kernel's occupancy --
    // at most 1,024 of them, each taking as many groups of four patches, one after the other, as that needs
    // (at most sixteen turns a classifying workgroup: its records -- 48 bytes a turn -- lie in its LDS block)
    const uint32_t cls_max = std::min<uint32_t>(RM_ORD_MAX_CLS, std::max(1u, kn.cls_max_blocks));
    P.ordered = k.order && per_wg == 1u && a.cls_blocks != 0u && n_dyn > 0u && n_patches < (1u << RM_ORD_PATCH_BITS) &&
                n_patches <= 16u * 4u * cls_max;
    if (P.ordered) {
        const uint64_t key[3] = {(uint64_t)a.n_tiles | ((uint64_t)p.frame_width << 32), (uint64_t)band.begin | ((uint64_t)band.stride << 32),
                                 sc.scene_epoch ^ ((uint64_t)a.n_static << 40)};
        P.order_patches = n_patches;
        const bool grown = order_cap < n_patches;
        const rm_order_layout L{grown ? n_patches : order_cap};
        P.order_cap = (uint32_t)L.cap;
        // (an entry of the order is taken by its tag: another geometry or scene, or the tags used up -> start afresh)
        const uint32_t tag_wrap = kn.ord_tag_wrap ? kn.ord_tag_wrap : (1u << RM_ORD_TAG_BITS) - 1u;
        const bool fresh = grown || std::memcmp(s.order_key, key, sizeof key) != 0;
        if (fresh || s.ord_tag >= tag_wrap) {
            P.order_clear = fresh ? rm_launch_plan::ORDER_CLEAR_ALL : rm_launch_plan::ORDER_CLEAR_FLAT;
            if (fresh) {
                std::memcpy(s.order_key, key, sizeof key);
                s.order_frames = 0;
                s.static_read = s.static_written = -1;
                s.list_tag[0] = s.list_tag[1] = 0u;
            }
            s.ord_tag = 0;
            s.last_tag = 0;
        }
        const uint32_t f = s.order_frames++;
        const uint32_t seq = ++s.seq;
        if (f == 0u) s.key_seq0 = seq;
        // (the basis with it: a turn is a view that has moved -- no predecessor's order, first round or classification words)
        const double view[16] = {sc.camera.x, sc.camera.y, sc.camera.z, p.half_fov, p.height, p.width, p.ratio,
                                 cb.right.x, cb.right.y, cb.right.z, cb.up.x, cb.up.y, cb.up.z, cb.forward.x, cb.forward.y, cb.forward.z};
        if (f == 0u || std::memcmp(s.view, view, sizeof view) != 0) {
            std::memcpy(s.view, view, sizeof view);
            s.view_seq0 = seq;
        }
        const bool timed = n_patches <= (k.order_in_big_scene ? kn.patch_order_max_deep : kn.patch_order_max);             // (larger launches are many rounds deep: by place, for the sky tail alone)
        const uint32_t groups4 = (n_patches + 3u) / 4u;
        a.cls_iters = (groups4 + cls_max - 1u) / cls_max;
        a.cls_blocks = (groups4 + a.cls_iters - 1u) / a.cls_iters;
        // While the view stands still a launch dispatches by the order its predecessor laid out -- same view, same
        // classification, the same first round: nothing to wait for -- and lays out the next launch's, from tile times a
        // frame fresher.  A view that has moved dispatches by its own order (the waves behind the first round wait for it).
        // (from the view's FOURTH launch on.  A launch that dispatches by its predecessor's order keeps its predecessor's first
        // round, and so do all after it: that first round had better be the view's dearest patches -- the first places of an
        // order sorted by this view's own tile times, which the view's second launch is the first to lay out and its third
        // the first to take its first round from.  Measured with the first round frozen a launch earlier, by place: a
        // quarter of the 1080p frame 45 us a frame against 34.5.)
        const bool reuse = kn.order_reuse && f >= 3u && seq >= s.view_seq0 + 3u && s.last_tag != 0u;
        a.ord_cap = P.order_cap;
        a.ord_tag = ++s.ord_tag;
        a.ord_read_tag = reuse ? s.last_tag : a.ord_tag;
        s.last_tag = a.ord_tag;
        const bool late_places = reuse && kn.order_late_places;
        // (same view as the launch before: its classification is this launch's)
        a.mask_tag_prev = reuse && kn.mask_reuse ? mask_tag_before : 0u;
        // A standing view, further: a launch that dispatches by its predecessor's order and takes its predecessor's
        // classification words computes, at its head, the very words and (but for a frame's noise in the tile times) the very
        // order its predecessor did.  Of order_freeze + 1 such launches only one does: the others are that launch less its
        // classifying workgroups and the workgroups that write the places -- same order read, same first round, same words
        // (all of them there: the predecessor is over), same tail -- and leave the stream's bookkeeping as they found it, so
        // the next launch that does classify is set up exactly as if they had not been.  Their tile times go into the same
        // counters (a maximum, a sum and a count: of two frames then).  What it spares: ~500 waves that hold a slot for 5-13 us
        // at the launch's start and ~500 short workgroups at its end.
        P.frozen = kn.order_freeze > 0 && reuse && f >= 4u && before.frozen_run < (uint32_t)kn.order_freeze && a.mask_tag > 1u &&
                   a.mask_tag_prev != 0u && late_places && kn.test_stall_order == 0 && kn.sky_tail_force < 0 && !kn.debug_tail;
        const bool lays_out = !P.frozen;                                     // (its own order, for whoever comes next)
        point(P, &KernelArgs::ord_cnt, RM_BUF_ORDER, 4u * L.cnt(f & 1u));
        point(P, &KernelArgs::ord_flat, RM_BUF_ORDER, 4u * L.flat(f & 1u));
        point(P, &KernelArgs::ord_read, RM_BUF_ORDER, 4u * L.flat(reuse ? (f + 1u) & 1u : f & 1u));
        if (lays_out) point(P, &KernelArgs::ord_cnt_next, RM_BUF_ORDER, 4u * L.cnt((f + 1u) & 1u));
        if (lays_out && late_places) point(P, &KernelArgs::ord_rec, RM_BUF_ORDER, 4u * L.rec());
        if (timed) point(P, &KernelArgs::patch_cost, RM_BUF_ORDER, 4u * L.cost(f % 3u));
        if (timed) point(P, &KernelArgs::cost_prev, RM_BUF_ORDER, 4u * L.cost((f + 2u) % 3u));
        if (timed && lays_out) point(P, &KernelArgs::cost_zero, RM_BUF_ORDER, 4u * L.cost((f + 1u) % 3u));
        point(P, &KernelArgs::ctab, RM_BUF_ORDER, 4u * L.ctab((f + 2u) % 3u));
        if (timed && kn.order_keys != 1) point(P, &KernelArgs::ctab_cur, RM_BUF_ORDER, 4u * L.ctab(f % 3u));
        if (lays_out) point(P, &KernelArgs::ctab_zero, RM_BUF_ORDER, 4u * L.ctab((f + 1u) % 3u));
        // The first round: the first places of the order the previous launch laid out (its classifying workgroups wrote them
        // down) -- unless this launch dispatches by that very order: then it keeps its predecessor's first round, which that
        // order leaves out.  Every launch writes the first places of the order it lays out for whoever comes next.
        if (kn.first_round_from_order) {
            const int read = reuse ? s.static_read : s.static_written;
            const uint32_t write = read == 0 ? 1u : 0u;
            if (read >= 0) {
                point(P, &KernelArgs::static_list, RM_BUF_ORDER, 4u * L.first((uint32_t)read));
                point(P, &KernelArgs::dyn_index, RM_BUF_ORDER, 4u * L.index((uint32_t)read));
                point(P, &KernelArgs::dyn_inv, RM_BUF_ORDER, 4u * L.inv((uint32_t)read));
                point(P, &KernelArgs::lists_done, RM_BUF_ORDER, 4u * (L.done() + (uint32_t)read));
                a.lists_tag = s.list_tag[read];
            }
            if (lays_out) {
                point(P, &KernelArgs::static_next, RM_BUF_ORDER, 4u * L.first(write));
                point(P, &KernelArgs::dyn_index_next, RM_BUF_ORDER, 4u * L.index(write));
                point(P, &KernelArgs::dyn_inv_next, RM_BUF_ORDER, 4u * L.inv(write));
                point(P, &KernelArgs::lists_done_next, RM_BUF_ORDER, 4u * (L.done() + write));
            }
            s.list_tag[write] = a.ord_tag;
            s.static_read = read;
            s.static_written = (int)write;
        } else {
            s.static_read = s.static_written = -1;
        }
        // what the patches are ordered by: the previous frame's times by place while the view is the one that frame had; else
        // the cost of what a patch can reach, once a table exists (written by the launch before from the launch before that)
        a.key_mode = !timed || f == 0u || kn.order_keys == 0 ? RM_KEY_PLACE
                   : (seq > s.view_seq0 && kn.order_keys != 2) ? RM_KEY_COST
                   : (a.mask_exact && a.mask_tag && kn.order_keys != 1) ? RM_KEY_CONTENT : RM_KEY_PLACE;
        point(P, &KernelArgs::ord_hint, RM_BUF_HINT, 0);
        point(P, &KernelArgs::err_word, RM_BUF_HINT, sizeof(unsigned long long));
        a.launch_seq = seq;
        a.test_stall = (uint32_t)kn.test_stall_order;                     // (test hooks)
        // Sky tail.  The first classifying workgroup of every launch tells the host how many of the ordered patches had
        // something to hit (page-locked memory, read by the launcher without a wait: `hint`).  The places behind them -- the sky -- get one wave
        // each instead of sixteen (the dispatcher takes ~0.7 ns per wave that finds out that its tile is sky: half of a
        // Cornell launch).  From a frame of THIS view the count is exact; from an earlier view it is a guess, and the places
        // it gets wrong -- the tail's first -- are rendered by sixteen waves each behind the grid's end.
        uint32_t tail = 0, cap = 0;
        if (kn.sky_tail) {
            bool guess = false;
            if (kn.sky_tail_force >= 0) {                                 // (test hook: a hint that is wrong)
                tail = std::min((uint32_t)kn.sky_tail_force, n_dyn);
                guess = true;
            } else {
                const uint32_t h_seq = (uint32_t)(hint >> 32), n_lit = (uint32_t)hint;
                const bool valid = h_seq >= s.key_seq0 && h_seq < seq && hint != 0ull && n_lit <= n_dyn;
                guess = h_seq < s.view_seq0 + 1u;                 // (the view's first launch may have had another first round)
                if (valid && (!guess || kn.sky_tail_motion)) tail = n_dyn - n_lit;
                if (tail < 8u) tail = 0u;
            }
            // (room to hand on: a press of the reference's buttons turns a few hundred of a 1080p frame's 1,980 patches)
            // (a count from this very view is exact -- which patches went first does not change it -- but a place too many in the
            // tail with nobody to hand it to costs sixteen tiles one after the other: a little room all the same)
            // (a guess's room, a press before every frame, 512 / 768 / 1,024 places: demo 50.2 / 47.9 / 47.8 us, Cornell 37.1 / - / 38.2 --
            // the walk turns up to 700 of the demo's patches at a press; a place beyond the room costs sixteen tiles one after the
            // other, an empty place sixteen waves that look and leave.  Sizing the room from how wrong the stream's recent guesses
            // were was tried and is worse, 60-80 us: the shortfall is mostly small and now and then 500)
            if (tail) cap = std::min(tail, kn.sky_tail_cap >= 0 ? (uint32_t)kn.sky_tail_cap : guess ? std::max(768u, n_patches / kn.sky_tail_room_div) : 32u);
        }
        a.tail_patches = tail;
        a.ov_cap = cap;
        // (dealt out evenly among the tile waves behind the launch's first round: rm_render_kernel.inc)
        const uint64_t behind = 16ull * (n_dyn - tail);
        a.tail_q = (tail && behind) ? (uint32_t)((((uint64_t)tail << 32) + behind + tail - 1u) / (behind + tail)) : 0u;
        // Launches of up to 4,096 patches: the tail BEHIND every tile wave instead (same box: Cornell 32.7 -> 31.4 us, demo
        // 69.2 -> 68.5 -- a tile with something to hit never waits for a slot behind a wave that only stores, and the
        // tail's stores, 24-43 MB, overlap the drain); an 8K launch ends with 380 MB of them if they wait: 960 -> 1,020 us.
        if (a.tail_q > 1u && (kn.sky_tail_place == 2 || (kn.sky_tail_place == 0 && timed))) a.tail_q = 1u;
        if (P.frozen) {
            a.cls_blocks = 0u; a.cls_iters = 0u; a.cls_prims = 0u;
            a.mask_tag = a.mask_tag_prev = before.tag;                    // (the words as the predecessor left them)
            cls_words_wanted = 0u;
            // (the bookkeeping as it was; only the count of launches like this one moves)
            s = before;
            s.frozen_run = before.frozen_run + 1u;
        } else {
            s.frozen_run = 0u;
        }
        // the classifying workgroups | the first round | sixteen waves a patch | one a place of the tail | sixteen a place handed
        // on | the workgroups that write the places
        P.grid = a.cls_blocks + a.n_static + 16u * (n_dyn - tail) + tail + 16u * cap + (lays_out && late_places ? a.cls_blocks : 0u);
    }
    if (cls_words_wanted) {
        // a record of three words per group of four patches and turn (OrdRec), behind the packed data; the block every workgroup
        // of the launch is given must still let the kernel's waves all be resident: 16 workgroups to a CU, 12 in the edge-test kernels
        const uint32_t rec_words = (std::max(a.cls_iters, 1u) * 4u * 3u + 1u) / 2u;
        if (cls_words_wanted + rec_words <= (k.edges ? 1664u : 1248u)) {
            a.cls_lds_words = cls_words_wanted;
            P.lds_bytes = std::max(P.lds_bytes, (size_t)(cls_words_wanted + rec_words) * sizeof(double));
        }
    }
    P.after = s;
    return true;
}

bool rm_band_of(const rm_params &p, rm_band *band) {
    const uint32_t n_height = p.frame_height / RM_PATCH_SIZE;   // renderer.rs:53: bottom H%32 rows never rendered
    uint32_t b = p.patch_row_begin, e = p.patch_row_end == 0 ? n_height : p.patch_row_end;
    if (e > n_height) e = n_height;
    if (b > e) return false;
    band->begin = b;
    band->end = e;
    band->stride = p.patch_row_stride == 0 ? 1u : p.patch_row_stride;
    return true;
}

// Test hook, not part of the ABI (tests/test_launch_plan.py): the plans of `n` render launches, one after the other on one
// imaginary stream, with the knobs as the environment has them now.  Every launch is given as the scene's header counts, the
// params, the camera and the hint word the host would read; every plan's "state after" is committed before the next is made.
// No device is needed.
struct rmi_plan_case {
    uint32_t n_spheres, n_polygons, n_triangles, total_words;
    uint32_t bvh, integer_exponents, oriented, n_cus;
    uint64_t scene_epoch;
    rm_params params;
    rm_vec3 camera;
    rm_camera_basis basis;
    unsigned long long hint;
};
struct rmi_plan_row {
    uint32_t grid, block, lds_bytes;
    uint32_t fast, stack, pow_mode, waves, per_wave, staged, bvh, cull, edges, order, feedback;   // rm_kernel_name's template arguments
    uint32_t classify, classify_in_front, ordered, frozen;
    uint32_t clear_masks, order_patches, order_clear;                   // the device work asked for (order_clear: 0 none, 1 flat[0..2), 2 the whole block)
    uint32_t n_tiles, cls_blocks, cls_iters, n_static, tail_patches, ov_cap, key_mode, mask_tag, mask_tag_prev, ord_tag, ord_read_tag, launch_seq;
    uint32_t reads_own_order, late_places;                              // ord_read == ord_flat; ord_rec != NULL
    rm_stream_state after;
};
extern "C" rm_status rmi_plan_launches(const rmi_plan_case *cases, uint32_t n, rmi_plan_row *rows) {
    if (!cases || !rows) { rm_set_host_error("rmi_plan_launches: NULL argument"); return RM_ERR_INVALID_ARG; }
    const rm_knobs kn = rm_knobs_from_env();
    rm_stream_state s;
    rm_feedback_state fb;
    uint32_t order_cap = 0;
    for (uint32_t i = 0; i < n; i++) {
        const rmi_plan_case &c = cases[i];
        rm_dev_header H{};
        H.n_spheres = c.n_spheres; H.n_polygons = c.n_polygons; H.n_triangles = c.n_triangles; H.total_words = c.total_words;
        H.off_bvh_spheres = c.bvh;
        const rm_plan_scene sc{&H, c.scene_epoch, 0., c.integer_exponents != 0, c.oriented != 0, c.camera, &c.basis, c.n_cus};
        rm_band band;
        rm_launch_plan P;
        if (!rm_band_of(c.params, &band) || band.count() == 0 || !plan_launch(kn, sc, c.params, band, s, order_cap, fb, c.hint, &P)) {
            rm_set_host_error("rmi_plan_launches: launch " + std::to_string(i) + " has no plan");
            return RM_ERR_INVALID_ARG;
        }
        auto offset_of = [&](size_t field) {     // of the address the plan gives that pointer of KernelArgs, + 1 (0: none)
            for (uint32_t r = 0; r < P.n_refs; r++)
                if (P.refs[r].field == field) return P.refs[r].offset + 1u;
            return 0u;
        };
        const KernelArgs &a = P.args;
        const rm_kernel_choice &k = P.k;
        rows[i] = rmi_plan_row{P.grid, P.block, (uint32_t)P.lds_bytes,
                               k.fast, (uint32_t)k.stack, (uint32_t)k.pow_mode, (uint32_t)k.mode.waves, (uint32_t)k.mode.per_wave, k.staged, k.bvh, k.cull, k.edges, k.order || c.oriented, k.feedback,
                               P.classify, P.cls_fn != nullptr, P.ordered, P.frozen, P.clear_masks, P.order_patches, (uint32_t)P.order_clear,
                               a.n_tiles, a.cls_blocks, a.cls_iters, a.n_static, a.tail_patches, a.ov_cap, a.key_mode, a.mask_tag, a.mask_tag_prev, a.ord_tag, a.ord_read_tag, a.launch_seq,
                               P.ordered && offset_of(offsetof(KernelArgs, ord_read)) == offset_of(offsetof(KernelArgs, ord_flat)), offset_of(offsetof(KernelArgs, ord_rec)) != 0u,
                               P.after};
        if (P.classify) s = P.after;
        if (P.ordered) order_cap = P.order_cap;
        if (P.feedback) fb = P.feedback_after;
    }
    return RM_OK;
}

// Test hook, not part of the ABI (tests/test_dead_children.py): what a launch of a scene of these counts whose upload found
// empty half-spaces up to `dead_camera_limit` carries with this camera, with the knobs as the environment has them now --
// out[0] = KernelArgs::dead_children, out[1] = 1 where the kernel is a plain-walk one.  No device is needed.
extern "C" rm_status rmi_plan_dead_children(const rm_vec3 *camera, double dead_camera_limit, uint32_t n_spheres, uint32_t n_polygons,
                                            uint32_t n_triangles, uint32_t total_words, uint32_t *out) {
    if (!camera || !out) { rm_set_host_error("rmi_plan_dead_children: NULL argument"); return RM_ERR_INVALID_ARG; }
    const rm_knobs kn = rm_knobs_from_env();
    rm_dev_header H{};
    H.n_spheres = n_spheres; H.n_polygons = n_polygons; H.n_triangles = n_triangles; H.total_words = total_words;
    const rm_camera_basis basis{rm_vec3{1., 0., 0.}, rm_vec3{0., 1., 0.}, rm_vec3{0., 0., -1.}};
    const rm_plan_scene sc{&H, 1u, 0., true, false, *camera, &basis, 256u, false, dead_camera_limit};
    rm_params p{};
    p.half_fov = 0.75; p.height = 64.; p.width = 64.; p.ratio = 1.;
    p.frame_width = 64; p.frame_height = 64; p.max_depth = 3;
    rm_band band;
    rm_launch_plan P;
    if (!rm_band_of(p, &band) || !plan_launch(kn, sc, p, band, rm_stream_state{}, 0u, rm_feedback_state{}, 0ull, &P)) {
        rm_set_host_error("rmi_plan_dead_children: no plan");
        return RM_ERR_INVALID_ARG;
    }
    out[0] = P.args.dead_children & RM_DEAD_DROP;
    out[1] = (!P.k.bvh && !P.k.cull) ? 1u : 0u;
    return RM_OK;
}

// Test hook, not part of the ABI (tests/test_scene_sig.py): the scene signature of the image the upload of `d` builds, and what
// a 96x64 launch of it with this depth cap carries, with the knobs as the environment has them now (rmi_plan_launches' cases
// hold a scene's counts only: a signature needs the image) -- out[0] = the image's signature (rm_scene_signature), out[1] = the
// signature in the launch's KernelArgs::dead_children, out[2] = 1 where the kernel is one that has a body for signatures.
// No device is needed.
extern "C" rm_status rmi_plan_scene_sig(const rm_scene_desc *d, uint32_t use_bvh, uint32_t max_depth, uint32_t fast_fp, uint32_t *out) {
    if (!d || !out) { rm_set_host_error("rmi_plan_scene_sig: NULL argument"); return RM_ERR_INVALID_ARG; }
    const rm_knobs kn = rm_knobs_from_env();
    rm_image img;
    std::string error;
    if (rm_status st = rm_build_image(d, rm_image_options{use_bvh != 0 && !kn.disable_bvh, kn.shadow_masks}, img, error)) { rm_set_host_error(error); return st; }
    img.scene_sig = rm_scene_signature(img.H, img.blob.data());
    const rm_camera_basis basis{rm_vec3{1., 0., 0.}, rm_vec3{0., 1., 0.}, rm_vec3{0., 0., -1.}};
    // (field by field, by name: what rm_device.hip's plan_scene_of takes from the context comes from the image here, and a
    // field the struct gains later keeps its default instead of shifting these)
    rm_plan_scene sc{};
    sc.H = &img.H; sc.scene_epoch = 1u; sc.occ_camera_limit = img.occ_camera_limit; sc.integer_exponents = img.integer_exponents;
    sc.oriented = false; sc.camera = d->camera; sc.basis = &basis; sc.n_cus = 256u; sc.exact_only = img.exact_only;
    sc.dead_camera_limit = img.dead_camera_limit; sc.scene_sig = img.scene_sig;
    rm_params p{};
    p.half_fov = 0.75; p.height = 64.; p.width = 96.; p.ratio = 1.5;
    p.frame_width = 96; p.frame_height = 64; p.max_depth = max_depth;
    p.flags = fast_fp ? RM_FLAG_FAST_FP : 0u;
    rm_band band;
    rm_launch_plan P;
    if (!rm_band_of(p, &band) || !plan_launch(kn, sc, p, band, rm_stream_state{}, 0u, rm_feedback_state{}, 0ull, &P)) {
        rm_set_host_error("rmi_plan_scene_sig: no plan");
        return RM_ERR_INVALID_ARG;
    }
    out[0] = img.scene_sig;
    out[1] = (P.args.dead_children >> RM_SCENE_SIG_SHIFT) & RM_SCENE_SIG_MASK;
    out[2] = rm_scene_sig_kernel(P.k.staged, P.k.bvh, P.k.cull) ? 1u : 0u;
    return RM_OK;
}

// Test hook, not part of the ABI (tests/test_checked_numerics.py): whether a launch with this camera (and this basis, where
// `oriented`) of a scene whose upload said `scene_exact_only` would be exact only, with the knobs as the environment has them
// now -- the decision plan_launch puts into its plan.  No device is needed.
extern "C" rm_status rmi_plan_exact_only(const rm_vec3 *camera, const rm_camera_basis *basis, uint32_t oriented, uint32_t scene_exact_only, uint32_t *out) {
    if (!camera || !basis || !out) { rm_set_host_error("rmi_plan_exact_only: NULL argument"); return RM_ERR_INVALID_ARG; }
    const rm_knobs kn = rm_knobs_from_env();
    rm_dev_header H{};
    H.n_spheres = 1; H.total_words = 128;
    const rm_plan_scene sc{&H, 1u, 0., true, oriented != 0, *camera, basis, 256u, scene_exact_only != 0};
    rm_params p{};
    p.half_fov = 0.75; p.height = 64.; p.width = 64.; p.ratio = 1.;
    p.frame_width = 64; p.frame_height = 64; p.max_depth = 3;
    rm_band band;
    rm_launch_plan P;
    if (!rm_band_of(p, &band) || !plan_launch(kn, sc, p, band, rm_stream_state{}, 0u, rm_feedback_state{}, 0ull, &P)) {
        rm_set_host_error("rmi_plan_exact_only: no plan");
        return RM_ERR_INVALID_ARG;
    }
    *out = (P.exact_only ? 1u : 0u) | (P.args.exact_only ? 2u : 0u);
    return RM_OK;
}

// Test hook, not part of the ABI (tests/test_launch_plan.py, tests/test_variant_matrix.py): the two decisions of a shading
// launch, with the knobs as the environment has them now.  header (rmi_scene_image's: rm_dev_header's 19 integer fields in their
// order) with the image's integer_exponents verdict and a depth cap -> variant[3] = bvh, pow_mode, stack; and, where `grid` is
// given, *grid = rm_shading_grid of the five numbers.  Either half may be left out (header / grid NULL).  No device is needed.
extern "C" rm_status rmi_shading_launch(const uint32_t *header, uint32_t integer_exponents, uint32_t max_depth, uint32_t *variant,
                                        uint32_t total, uint32_t rays_per_pixel, int32_t n_cus, int32_t per_cu, uint32_t max_blocks,
                                        uint32_t *grid) {
    if (header) {
        if (!variant) { rm_set_host_error("rmi_shading_launch: NULL variant"); return RM_ERR_INVALID_ARG; }
        rm_dev_header H{};
        std::memcpy(&H, header, 19u * sizeof(uint32_t));
        const rm_shading_variant v = rm_shading_variant_of(rm_knobs_from_env(), H, integer_exponents != 0, max_depth);
        variant[0] = v.bvh ? 1u : 0u; variant[1] = (uint32_t)v.pow_mode; variant[2] = (uint32_t)v.stack;
    }
    if (grid) {
        if (rays_per_pixel < 1u || rays_per_pixel > 64u) { rm_set_host_error("rmi_shading_launch: rays_per_pixel is outside 1..64"); return RM_ERR_INVALID_ARG; }
        *grid = rm_shading_grid(total, rays_per_pixel, n_cus, per_cu, max_blocks);
    }
    return RM_OK;
}
