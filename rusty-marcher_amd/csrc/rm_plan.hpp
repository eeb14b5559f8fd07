// rm_plan.hpp -- the host's decisions about a render launch, as values: the A/B knobs and test hooks read from
// the environment (rm_knobs), the kernel a launch takes (rm_kernel_choice) and everything else the launcher needs
// (rm_launch_plan).  rm_plan.cpp computes them and touches no device: it is a host-only unit, this header and it
// include nothing of HIP, and a stream is not even a key here -- the launcher (rm_device.hip launch_render) looks
// the stream's state up, does the device work a plan lists, launches, and only then commits the plan's "state after".
#ifndef RM_PLAN_HPP
#define RM_PLAN_HPP

#include <stddef.h>
#include <stdint.h>

#include "rm_internal.h"
#include "rm_kernel_args.hpp"

// dispatch order of the tiles (tile_origin): RM_TILE_ORDER = natural | reverse | hash
enum { TILE_ORDER_NATURAL = 0, TILE_ORDER_REVERSE = 1, TILE_ORDER_HASH = 2 };

// (launches of more than one round of wave slots -- 4,096 -- and a little: with the patches sorted by their longest tile the order
// pays from there on: 640x480, 4,800 tiles, 35.9 -> 31.9 us, 800x600 34.1 -> 31.0, a quarter of a 1080p frame 44.4 -> 34.8;
// 320x240, 1,120 tiles, which all start at once: 18.0 -> 19.3, left alone)
// (3,584: both share sizes of a 1080p frame at N = 8 -- 3,840 and 4,800 tiles -- take the same path; measured no difference in time)
static constexpr uint32_t RM_CLASSIFY_MIN_TILES_DEFAULT = 3584;
static constexpr uint32_t RM_CULL_MIN_PRIMS = 12, RM_CULL_EDGES_MIN_PLANAR = 4, RM_CULL_MAX_COST = 250;

// A/B knobs and test hooks, read once from the environment by rm_init (rm_knobs_from_env: one table of names, fields
// and parse rules); const from then on.
struct rm_knobs {
    bool force_generic_pow = false;   // RM_FORCE_GENERIC_POW=1
    bool force_fast_fp = false;       // RM_FORCE_FAST_FP=1 (same as RM_FLAG_FAST_FP on every call)
    // Bottom-up by default: workgroups are dispatched in id order and the drain at the end
    // of a launch runs at low occupancy, so the rows that are expensive in the
    // reference's scenes (ground, objects resting on it) go first and the cheap sky rows
    // drain (1080p demo: 124 -> 116 us; hashed order 131 us).
    int tile_order = TILE_ORDER_REVERSE;
    bool disable_bvh = false;         // RM_DISABLE_BVH=1: brute-force walk
    // The six ticks that move a shape -- the moving shapes' (rm_render_progressive_moving, rm_render_converging_moving), the
    // moving camera's given velocities (rm_render_progressive_camera, rm_render_converging_camera) and the moving spheres'
    // (rm_render_progressive_motion, rm_render_converging_motion) -- walk a swept hierarchy where the resident image holds one
    // (rm_swept_host.inc, tick_walks_swept): RM_SWEPT_BVH=0 returns all six to the flat walk (the A/B switch; frames are
    // bit-equal).  On by measurement: the Cornell box's 36 triangles, the smallest hierarchy there is, take 0.50 to 0.73 of the
    // flat pass's time (profiles/swept_figures.txt; the camera's and the spheres' ticks: profiles/camera_swept_figures.txt).
    bool swept_bvh = true;
    // Ray bundles whose half-angle has at least this cosine cull primitives before a walk
    // (rm_trace.inc); wider ones take the plain walk / the hierarchy.  RM_DISABLE_CULL=1 sets 2
    // (never), RM_CULL_COS overrides.
    double cull_cos = 0.975;          // (synthetic-256: 0.9 1,911 us, 0.95 1,825, 0.97-0.98 1,777, 0.99 1,791, 0.999 1,847; cornell flat)
    uint32_t cull_min_prims = RM_CULL_MIN_PRIMS;   // RM_CULL_MIN
    bool cull_edges = true;           // RM_CULL_EDGES=0: the bundle cull without its edge test
    bool force_unstaged = false;      // RM_FORCE_UNSTAGED=1
    // The shadow rays' occluder masks of the plain-walk kernels (rm_build_shadow_masks): RM_SHADOW_MASKS=0 uploads no
    // table, and every shadow walk tests every primitive
    bool shadow_masks = true;
    // Children of a glass-like polygon / triangle that leave it into an empty half-space (rm_build_empty_sides) are not
    // walked by the plain-walk kernels: RM_DEAD_CHILDREN=0 walks them all the same (the A/B switch; frames are bit-equal)
    bool dead_children = true;
    // ... and a refracted child's fate -- beyond the depth cap, or into a flagged side for certain -- is decided before its ray
    // is formed (render_tile).  RM_DEAD_CHILDREN=0 and =1 form every ray and decide on its computed dot, as before
    bool early_fates = true;
    // A resident scene whose shape counts are a compiled-in signature's (rm_kernel_args.hpp RM_SCENE_SIGNATURES) is rendered by
    // the plain-walk kernels' body for those counts: RM_SCENE_SIG=0 keeps every launch on the generic body (the A/B switch;
    // frames are bit-equal)
    bool scene_sig = true;
    int force_stack = 0;              // RM_FORCE_STACK=4|8|16|32: a deeper ray stack than the depth cap needs
    bool debug_empty = false;         // RM_DEBUG_EMPTY=1: measure the dispatch floor of a launch geometry
    // frame-to-frame feedback (rm_feedback): RM_FEEDBACK=0 never, 1 always, unset: launches of
    // RM_FEEDBACK_MIN_TILES tiles and more with a depth cap of 6 and more (below, no tile is long)
    int feedback_mode = -1;
    uint32_t feedback_us = 50;        // RM_FEEDBACK_US: a tile is long from here on, until a frame's histogram says better
    int feedback_target = -1;         // RM_FEEDBACK_TARGET: tiles the list should hold (-1: two per wave slot; 0: fixed threshold)
    // tile classification (rm_classify.hip): RM_TILE_CLASSIFY=0 never, 1 whenever the scene allows; unset:
    // launches of RM_CLASSIFY_MIN_TILES tiles and more
    int classify_mode = -1;
    bool classify_in_launch = true;      // RM_CLASSIFY_IN_LAUNCH=0: always a launch of its own in front
    bool sky_tail = true;                // RM_SKY_TAIL=0: every patch gets its sixteen waves
    uint32_t patch_order_max = 4096;     // RM_PATCH_ORDER_MAX: launches of up to this many patches take the kernels with the patch order
    uint32_t patch_order_max_deep = 65536;   // RM_PATCH_ORDER_MAX_DEEP: ... in scenes with a hierarchy (tile times with a long tail)
    // Launches of this many patches and more take the kernels with the patch order for the sky tail alone (by place):
    // measured 8K 987 -> 960 us; at 4K (8,100 patches) the sorting workgroup and the order's indirection cost what the tail saves
    // (245.3 against 243.8 us).
    uint32_t sky_tail_big_min = 16384;   // RM_SKY_TAIL_BIG_MIN (patches)
    uint32_t sky_tail_room_div = 16;     // RM_SKY_TAIL_ROOM_DIV: a guessed tail's room in launches of many patches: patches / this
    bool sky_tail_big = true;            // RM_SKY_TAIL_BIG=0: launches of more than patch_order_max patches keep the kernels without the patch order
    bool sky_tail_motion = true;         // RM_SKY_TAIL_MOTION=0: no tail in a frame whose view differs from the frames the hint came from
    int sky_tail_place = 0;              // RM_SKY_TAIL_PLACE=even|end: the tail's waves dealt out among the tile waves / behind them (unset: behind them in launches of up to patch_order_max patches)
    int sky_tail_cap = -1;               // RM_SKY_TAIL_CAP=n: places a guessed tail can hand on to waves behind the grid's end (unset: max(512, patches / 16))
    bool classify_lds = true;            // RM_CLASSIFY_LDS=0: the classifying workgroups of scenes without an LDS copy read their tests' data from memory
    uint32_t classify_in_launch_prims = 56;   // RM_CLASSIFY_IN_LAUNCH_PRIMS: scenes of up to this many primitives are classified at the head of the render launch
    uint32_t classify_min_tiles = RM_CLASSIFY_MIN_TILES_DEFAULT;   // RM_CLASSIFY_MIN_TILES: launches of this many tiles and more are classified (and ordered); 0: the built-in
    bool mask_reuse = true;              // RM_MASK_REUSE=0: a launch waits for its own classification even where its predecessor's is as good
    uint32_t static_rounds = 2;          // RM_STATIC_ROUNDS=n: n rounds of waves take their patches from the previous ranking without waiting for the order
    uint32_t cls_max_blocks = RM_ORD_MAX_CLS;   // RM_CLS_MAX_BLOCKS=n: at most n classifying workgroups (each then takes more groups of four patches)
    int order_freeze = 7;                // RM_ORDER_FREEZE=n: of n + 1 launches of a standing view only one classifies and lays out an order (0: every launch)
    bool order_late_places = true;       // RM_ORDER_LATE_PLACES=0: the classifying workgroups always write the order's places themselves
    bool order_reuse = true;             // RM_ORDER_REUSE=0: every launch dispatches by its own order, standing view or not
    bool first_round_from_order = true;  // RM_FIRST_ROUND_FROM_ORDER=0: the first round is the bottom rows by place
    int first_round = -1;                // RM_FIRST_ROUND=n: the waves that neither wait for their tiles' classification nor take a place in the order (unset: what is resident at once)
    int order_keys = -1;                 // RM_ORDER_KEYS=0 by place only, 1 the previous frame's times by place only, 2 cost by content only (unset: times while the view stands, content once it has moved)
    uint32_t ord_tag_wrap = 0;           // RM_ORD_TAG_WRAP=n (test hook): the order's tags start afresh after n launches instead of 4,095
    int test_stall_order = 0;            // RM_TEST_STALL_ORDER (test hook) = 1: the launch's order is never laid out (the frame is void); = 2: its classifying workgroups never say they have arrived (the order of last resort)
    int sky_tail_force = -1;             // RM_SKY_TAIL_FORCE=n (test hook): the last n patches of the order are taken for sky, whatever the hint says
    int patch_order_mode = -1;           // RM_PATCH_ORDER=0 never, 1 whenever possible; unset: launches of RM_CLASSIFY_MIN_TILES tiles and more
    // RM_CHECKED_NUMERICS=0: every launch of the strict plain-walk kernels is exact only -- the compiler's own square roots and
    // divisions throughout (the A/B switch, and what the bit-equality tests compare with)
    bool checked_numerics = true;
    uint32_t refine_max_blocks = 0;      // RM_REFINE_MAX_BLOCKS=n: at most n workgroups shade the pixels an anti-aliased frame refines, each then loops over more groups (unset / 0: what the device holds at once; results do not change)
    uint32_t lens_max_blocks = 0;        // RM_LENS_MAX_BLOCKS=n: at most n workgroups shade a thin-lens frame or a pass of a progressive one (rm_accum.hip has the lens kernel's grid), each then loops over more groups of pixels (unset / 0: what the device holds at once; results do not change)
    bool debug_tail = false;             // RM_DEBUG_TAIL (set at all): every ordered launch is waited for and its order dumped to stderr; no launch is frozen
};
rm_knobs rm_knobs_from_env();

// The patch rows a call owns: begin, begin + stride, ... < end.
struct rm_band {
    uint32_t begin = 0, end = 0, stride = 1;
    uint32_t count() const { return end > begin ? (end - begin + stride - 1) / stride : 0; }
};

// false: patch_row_begin > patch_row_end
bool rm_band_of(const rm_params &p, rm_band *band);

// What a plan needs to know of the context: the resident scene and the camera.
struct rm_plan_scene {
    const rm_dev_header *H;
    uint64_t scene_epoch;
    double occ_camera_limit;          // cameras farther out (L1 norm) render without the image's occluder masks
    bool integer_exponents;           // every material's specular_exponent is a small non-negative integer
    bool oriented;
    rm_vec3 camera;
    const rm_camera_basis *basis;     // (the fixed view's own while the oriented state is off)
    uint32_t n_cus;
    bool exact_only = false;          // the resident scene is outside what the checked numerics are proven for (rm_image.cpp scene_exact_only)
    double dead_camera_limit = 0.;    // cameras farther out (L1 norm) walk every child ray (0: the image has no empty half-space, rm_build_empty_sides)
    uint32_t scene_sig = 0u;          // the resident image's signature (rm_scene_signature at its upload; 0: none)
};

// The number of the compiled-in signature (rm_kernel_args.hpp RM_SCENE_SIGNATURES, from 1) that the image of header `H` and
// words `blob` carries, 0 where it carries none: every count, every polygon's vertex count (read from its record),
// list_ordered, and no hierarchy.  Pure: decided once per upload, and by the tests' hook.
uint32_t rm_scene_signature(const rm_dev_header &H, const double *blob);

// Checked numerics (rm_trace.inc RM_CHECKED): a coordinate, radius, camera or light word is inside the proven range when it is
// finite and at most this in magnitude -- no intermediate of a sphere test can then overflow -- ...
static constexpr double RM_CHECKED_COORD_MAX = 0x1p+200;
// ... and a sphere's radius_square when the discriminant's root needs no scaling: a non-zero r^2 - d^2 is at least r^2 2^-54
static constexpr double RM_CHECKED_R2_MIN = 0x1p-600, RM_CHECKED_R2_MAX = 0x1p+600;
inline bool rm_checked_coord_ok(double v) { return v >= -RM_CHECKED_COORD_MAX && v <= RM_CHECKED_COORD_MAX; }   // (NaN: no)
// The camera a launch carries (rm_camera_update can set it to anything), and the basis where the launch is oriented.
bool rm_camera_exact_only(const rm_plan_scene &sc);

// How the 64-pixel tiles of a band are handed to waves (see rm_render_kernel.hpp): `waves`
// waves per workgroup, `per_wave` tiles per wave.  Measured at 1080p on the demo scene
// (profiles/r01_ab_launch_modes.txt): one tile per wave wins (finer units for the
// hardware dispatcher: 4 tiles per wave 193 us vs 1 tile 122 us); 1 or 4 waves per
// workgroup differ by ~2 % there -- but not where tile costs differ widely: a slot freed by a
// workgroup of four is handed on only when a whole workgroup fits (256 spheres: 1,777 us with
// four waves, 1,420 with one).
// A persistent variant (waves pulling tiles from a global counter) was measured too and
// dropped: one atomic word serves ~70 claims/us, a 1080p frame needs >300 tiles/us.
// This build instantiates one tile per wave, one wave per workgroup only; the other geometries
// were measured with earlier builds.
struct rm_launch_mode {
    int waves = 0;      // waves per workgroup
    int per_wave = 1;   // tiles per wave
};

// Which kernel instantiation a render with these params launches, and how.
struct rm_kernel_choice {
    const void *fn = nullptr;
    rm_launch_mode mode;
    size_t lds_bytes = 0;
    int stack = 0, pow_mode = 0;
    bool fast = false, staged = false, bvh = false, cull = false, edges = false, order = false, feedback = false;
    bool order_in_big_scene = false;  // a scene with a hierarchy whose launches are classified at their own head and dispatched by that
    // the scene as the classification sees it: primitives, planar ones among them, and a lane's share of a patch's
    // classification in vector instructions (order_in_big_scene assumes that the launch classifies: one figure for both)
    uint32_t n_prims = 0, n_planar = 0, classify_cost = 0;
    bool planar_edges = false;        // planar primitives enough for the bundle cull's edge test to pay (`edges`: ... and the kernel has it)
};
// false: no kernel for this scene / depth combination
bool choose_kernel(const rm_knobs &kn, const rm_plan_scene &sc, const rm_params &p, uint32_t tiles, rm_kernel_choice *k);

// Which instantiation of radiance_steps<BVH, POW, STACK> (rm_radiance_step.inc) a launch of the shading kernels takes -- the
// radiance queries, adaptive anti-aliasing, the thin-lens camera, progressive, soft and converging frames alike.  choose_kernel's
// rules for the hierarchy and the power, with a reduced set of stacks: a lane parks at most max_depth - 1 rays, 4 serves a cap
// of up to 5, 32 every other.  Unlike choose_kernel this rule does not look at RM_FORCE_STACK: these kernels are instantiated
// for 4 and 32 only, and the knob's deeper stack is the render kernels' A/B switch.
struct rm_shading_variant {
    bool bvh;
    int pow_mode;
    int stack;
};
rm_shading_variant rm_shading_variant_of(const rm_knobs &kn, const rm_dev_header &H, bool integer_exponents, uint32_t max_depth);

// Workgroups of a launch that shades `total` pixels with `rays_per_pixel` (1..64) rays each, 64 / rays_per_pixel pixels a
// workgroup at a time: what the frame needs, at most what the device holds at once (max(1, n_cus) x per_cu, the kernel's
// occupancy), at most `max_blocks` where that is not 0 (RM_REFINE_MAX_BLOCKS / RM_LENS_MAX_BLOCKS), at least 1.  The
// workgroups loop over what is left.
uint32_t rm_shading_grid(uint32_t total, uint32_t rays_per_pixel, int n_cus, int per_cu, uint32_t max_blocks);

// The bookkeeping of the render launches on one stream (rm_tile_lists holds it next to the stream's buffers).  A plan is
// made from it as it stands and carries what it is after the launch; the launcher stores that once the launch is out.
struct rm_stream_state {
    // dispatch order: launches of this geometry and scene so far, and that geometry and scene
    uint32_t order_frames = 0;
    uint64_t order_key[3] = {0, 0, 0};
    uint32_t list_tag[2] = {0, 0};    // the tag of the launch that was to write first[] / index[] / inv[] of that number
    int static_read = -1, static_written = -1;   // the first[] / index[] pair the previous launch's first round came from / the one it wrote for a successor (-1: none)
    uint32_t last_tag = 0;            // the tag of the order the previous launch laid out (0: none to dispatch by)
    // the launches on this stream counted, the first launch of the view being rendered, the first of this geometry and
    // scene, and that view
    uint32_t seq = 0, view_seq0 = 0, key_seq0 = 0, ord_tag = 0;
    double view[16] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};   // camera, Renderer, the camera's basis
    // classification at the head of the render launch: the words carry the launch's tag (1..255)
    uint32_t tag = 0, tagged_tiles = 0;
    uint64_t tagged_scene = 0;
    bool tagged = false;
    uint32_t frozen_run = 0;          // launches in a row that took everything from their predecessor (order_freeze)
};

// ... and of the frame-to-frame feedback's three sets (rm_feedback)
struct rm_feedback_state {
    bool valid = false;               // the sets exist
    uint64_t key[3] = {0, 0, 0};      // launch geometry and scene they belong to
    uint32_t n_tiles = 0;
    int cur = 0;                      // the set the next frame reads
};

// Layout of a stream's order block, in u32 words (cap: patches):
//   cost[3][cap] | ctab[3][128] | cnt[2][RM_ORD_CNT_WORDS] | flat[2][cap] | first[2][cap] | index[2][cap] | inv[2][cap] | rec[3][cap + 4096] | done[2]
// the sets take turns from launch to launch (a launch reads what its predecessor on the stream wrote, and clears what
// its successor will count into)
struct rm_order_layout {
    size_t cap;
    size_t cost(uint32_t j) const { return (size_t)j * cap; }
    size_t ctab(uint32_t j) const { return 3u * cap + j * RM_CTAB_WORDS; }
    size_t cnt(uint32_t j) const { return 3u * cap + 3u * RM_CTAB_WORDS + j * RM_ORD_CNT_WORDS; }
    size_t flat(uint32_t j) const { return cnt(2) + (size_t)j * cap; }
    size_t first(uint32_t j) const { return flat(2u + j); }
    size_t index(uint32_t j) const { return flat(4u + j); }
    size_t inv(uint32_t j) const { return flat(6u + j); }
    size_t rec() const { return flat(8u); }
    size_t done() const { return rec() + 3u * (cap + 4096u); }
    size_t bytes() const { return (cap * 11u + 64u + 3u * (cap + 4096u) + 3u * RM_CTAB_WORDS + 2u * RM_ORD_CNT_WORDS) * 4u; }
};

// Layout of a stream's feedback block, in bytes: 3 x (hist[64] | count | 3 pad | list[cap] u32 | flag[n_tiles] u8) + threshold
struct rm_feedback_layout {
    uint32_t n_tiles, cap;
    size_t set_bytes;
    explicit rm_feedback_layout(uint32_t tiles)
        : n_tiles(tiles), cap((tiles + 7u) / 8u > 64u ? (tiles + 7u) / 8u : 64u),
          set_bytes((((size_t)cap + RM_FB_BUCKETS + 4u) * sizeof(uint32_t) + tiles + 255u) & ~(size_t)255u) {}
    size_t hist(int j) const { return (size_t)j * set_bytes; }
    size_t count(int j) const { return hist(j) + RM_FB_BUCKETS * 4u; }          // (cleared together with the histogram)
    size_t list(int j) const { return hist(j) + (RM_FB_BUCKETS + 4u) * 4u; }
    size_t flag(int j) const { return list(j) + (size_t)cap * 4u; }
    size_t threshold() const { return hist(3); }
    size_t bytes() const { return 3u * set_bytes + 256u; }
};

// The buffers a launch's arguments point into.  A plan names an address by buffer and byte offset: the order block and
// the hint may not exist yet when it is made.
enum rm_buf : uint8_t { RM_BUF_MASKS, RM_BUF_ORDER, RM_BUF_HINT, RM_BUF_FEEDBACK, RM_BUF_COUNT };
struct rm_arg_ref {
    uint16_t field;                   // offset of the pointer in KernelArgs
    rm_buf buf;
    uint32_t offset;                  // bytes
};

struct rm_launch_plan {
    rm_kernel_choice k;
    uint32_t grid = 0, block = 0;
    size_t lds_bytes = 0;
    // the render launch's arguments, complete but for bp_x / bp_y / frame8 / debug_stamps (the launcher's own) and the
    // pointers `refs` lists, which the launcher resolves once the buffers exist
    rmdev::KernelArgs args{};
    rm_arg_ref refs[40];              // (a launch has at most 22: the masks, the order's nineteen and the hint's two -- or the masks and the feedback's ten)
    uint32_t n_refs = 0;
    bool feedback = false;            // the launch carries the frame-to-frame feedback (the stream's feedback block must exist)
    bool classify = false;            // the tiles are classified (the stream's mask block must hold n_tiles words) ...
    const void *cls_fn = nullptr;     // ... by a launch of its own in front (NULL: at the head of the render launch, or not at all)
    uint32_t cls_grid = 0;
    rmdev::ClassifyArgs cls_args{};   // (tile_mask: the launcher's)
    bool exact_only = false;          // checked numerics: the launch renders every tile with the exact twin (args.exact_only says so to the kernel)
    bool ordered = false;             // the launch has a dispatch order (the order block and the hint must exist)
    bool frozen = false;              // ... and takes everything from its predecessor (order_freeze)
    // device work in front of the launch, in this order
    bool feedback_reset = false;      // (re)allocate the feedback block to feedback_bytes where its sets' size differs, and clear it
    size_t feedback_bytes = 0, feedback_set_bytes = 0;
    bool clear_masks = false;         // clear the stream's mask words
    uint32_t order_patches = 0;       // the order block to hold this many patches (a larger one stays; a new one is cleared whole)
    enum { ORDER_CLEAR_NONE, ORDER_CLEAR_FLAT, ORDER_CLEAR_ALL } order_clear = ORDER_CLEAR_NONE;   // FLAT: flat[0..2) only
    uint32_t order_cap = 0;           // the block's capacity after that: what `refs` into it were computed with
    // the stream's bookkeeping after this launch
    rm_stream_state after;
    rm_feedback_state feedback_after;
};

// Everything about the next render launch on a stream whose bookkeeping is `s` (and `fb`), whose order block holds
// `order_cap` patches (0: none) and whose hint word reads `hint`.  Calls nothing of the device, reads no environment,
// writes to nothing but *out.  false: no kernel for this scene / depth combination.
bool plan_launch(const rm_knobs &kn, const rm_plan_scene &sc, const rm_params &p, const rm_band &band, const rm_stream_state &s,
                 uint32_t order_cap, const rm_feedback_state &fb, unsigned long long hint, rm_launch_plan *out);

#endif
