// rm_device.hip -- device half of the C ABI: context, scene upload, the render
// kernel and the framebuffer post-process kernels.  gfx950 (MI355X) only.
//
// Replaces Renderer::render's Rayon patch loop (renderer.rs:63-89), the serial
// scatter (renderer.rs:92-108) and cast_ray's recursion (renderer.rs:254-309).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "rm_image.hpp"
#include "rm_internal.h"
#include "rm_kernel_args.hpp"
#include "rm_plan.hpp"
#include "rm_sampling.hpp"
#include "rm_query.hpp"
#include "rm_radiance.hpp"
#include "rm_refine.hpp"
#include "rm_lens.hpp"
#include "rm_accum.hpp"
#include "rm_soft.hpp"
#include "rm_motion.hpp"
#include "rm_motion_shapes.hpp"
#include "rm_converge.hpp"
#include "rm_converge_motion.hpp"
#include "rm_converge_moving.hpp"
#include "rm_camera.hpp"
#include "rm_converge_camera.hpp"
#include "rm_swept_image.hpp"
#include "rm_swept.hpp"
#include "rm_converge_swept.hpp"
#include "rm_camera_swept.hpp"
#include "rm_converge_camera_swept.hpp"
#include "rm_denoise.hpp"
#include "rm_reproject.hpp"
#include "rm_bounce.hpp"

using namespace rmdev;

#ifndef RM_BUILD_FLAVOR
#define RM_BUILD_FLAVOR "fp64 strict+fast"
#endif

// With max_depth == 0 the primary ray itself is capped: every pixel is the
// background (renderer.rs:262-264 with n_recursion = 1 > 0).
__global__ void rm_fill_band_kernel(double *frame, size_t first_px, size_t n_px, double r, double g, double b) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_px) {
        double *p = frame + (first_px + i) * 3;
        p[0] = r; p[1] = g; p[2] = b;
    }
}

// ---------------------------------------------------------------------------
// Post-process kernels: framebuffer.rs:58-77 (normalize) and :40-55,:80-82
// (to_vec / quantize).
// ---------------------------------------------------------------------------

// Global max over all channel values, starting from 0 like the reference's
// `max = Vec3f::zero()`; f64::max ignores NaN, as fmax does.  Values are >= 0
// after max(0, .), so their bit patterns order like unsigned integers.
__global__ __launch_bounds__(256) void rm_max_kernel(const double *__restrict__ v, size_t n, unsigned long long *out_bits) {
    double m = 0.;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        m = __builtin_fmax(m, v[i]);
    for (int off = 32; off > 0; off >>= 1) m = __builtin_fmax(m, __shfl_down(m, off));
    __shared__ double part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = __builtin_fmax(__builtin_fmax(part[0], part[1]), __builtin_fmax(part[2], part[3]));
        atomicMax(out_bits, (unsigned long long)__double_as_longlong(m));
    }
}

// Optional in-place scale by 1/max (framebuffer.rs:69-76) and optional u8 output
// `(255. * f.max(0.).min(1.)) as u8` (truncating, NaN -> 0).
__global__ __launch_bounds__(256) void rm_scale_quantize_kernel(double *__restrict__ v, size_t n, const unsigned long long *max_bits,
                                                               int do_scale, uint8_t *__restrict__ out8) {
    double s = 1.;
    bool scale = false;
    if (do_scale) {
        const double max_val = __longlong_as_double((long long)*max_bits);
        if (max_val > 0.) { s = 1. / max_val; scale = true; }
    }
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        double f = v[i];
        if (scale) { f = f * s; v[i] = f; }
        if (out8) {
            const double c = 255. * __builtin_fmin(__builtin_fmax(f, 0.), 1.);
            out8[i] = (uint8_t)c;
        }
    }
}

// ---------------------------------------------------------------------------
// Context
// ---------------------------------------------------------------------------

// A frame in flight (rm_frame_submit): its own render stream, so that consecutive frames overlap.
struct rm_frame_slot {
    hipStream_t render = nullptr;
    hipEvent_t begun = nullptr, rendered = nullptr, gathered = nullptr;   // stamps of the frame on the slot's stream
    hipEvent_t exchanged = nullptr;   // recorded after the last operation of the slot's frame
    bool used = false;
    bool stamped = false;             // the slot's last frame carries the stamps of rm_frame_timing
};

// Frame-to-frame feedback.  The cost of a tile is known only once it has been rendered -- 1 to
// 18 ray steps on the 256-sphere scene, the incoherent ones thirty times the price of a coherent
// one -- and a launch ends with whatever long tile was dispatched late: there the last 150 of
// 260,000 waves ran for 200 of the launch's 1,600 us on an empty chip.  Frames of a render loop
// resemble their predecessors, so every wave times its tile, the tiles that took long are put on
// a list (one atomic each: they are few) and the next frame ON THE SAME STREAM dispatches the
// list first.  Nothing is carried over but the order of dispatch: every tile of every frame is
// rendered in full, by the same code.  Three rotating sets (list, count, one flag per tile): a
// frame reads one, fills the next and clears the counter of the third.  Kept per stream --
// launches on one stream are ordered, so a set is never read and written at once.
struct rm_feedback {
    hipStream_t stream = nullptr;
    void *block = nullptr;            // one allocation (rm_feedback_layout)
    size_t set_bytes = 0;
    uint64_t used = 0;
    rm_feedback_state s;              // launch geometry and scene the sets belong to; the set the next frame reads
};

struct rm_hostio;   // rm_hostio.inc: staging buffer, row-scatter threads, display frame
struct rm_progressive;   // rm_motion_host.inc: staged tables, sum, mean and bytes of rm_render_progressive*, its count and frame identity
struct rm_tick_swept;    // rm_swept_host.inc: the swept hierarchy of the moving shapes' ticks, and what it was built from
struct rm_converging;    // rm_converge_motion_host.inc: the buffers, resident sequences, pass total and frame identity of rm_render_converging*
struct rm_denoising;     // rm_denoise_host.inc: the workspace, the guide and the outputs of rm_render_denoised

// The classification's output for the render launches on one stream: a mask per tile.  (Launches on a
// stream are ordered: a render launch reads what the classification launch in front of it wrote, and the
// next classification overwrites it only after that render launch is over.  Classifying a frame ahead on
// a stream of its own was measured and dropped: the two cross-stream events cost more than the 3-8 us of
// the classification they hid -- demo scene 1080p 99.8 against 81.2 us per frame.)
struct rm_tile_lists {
    hipStream_t stream = nullptr;
    uint32_t cap = 0;                 // tiles the masks have room for
    void *block = nullptr;            // mask[cap] u64
    uint64_t used = 0;
    // Dispatch order from the launch's own classification (KernelArgs::ord_*), one block per stream (rm_order_layout)
    void *order_block = nullptr;
    uint32_t order_cap = 0;           // patches it has room for
    // sky tail: the first classifying workgroup's word in page-locked memory -- (launch seq << 32) | ordered patches with something
    // to hit --, behind it the word a wave writes when it gives up a wait that cannot fail
    unsigned long long *hint = nullptr;
    rm_stream_state s;                // the bookkeeping of the stream's launches: made into a plan, committed once the launch is out
    unsigned long long *mask() const { return static_cast<unsigned long long *>(block); }
};

struct rm_ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string error;
    hipDeviceProp_t prop{};

    // uploaded scene
    bool have_scene = false;
    rm_image image;                   // the resident image as the host built it (rm_scene_upload skips identical ones); the device's copies:
    double *d_scene = nullptr;
    size_t d_scene_words = 0;
    rm_vec3 camera{0., 0., 0.};
    // The oriented camera (rm_camera_orient / rm_camera_look_at).  Off: the reference's fixed view -- down -z, +y up -- and the
    // kernels that have it built in.  On: `basis` is a real turn (never the fixed view's own nine numbers: setting those turns
    // the state off) and every launch takes the oriented kernels.  The context's, like `camera`: an upload leaves it alone.
    bool oriented = false;
    rm_camera_basis basis{{1., 0., 0.}, {0., 1., 0.}, {0., 0., -1.}};
    uint64_t upload_calls = 0, upload_copies = 0;
    std::vector<unsigned char> desc_bytes;   // the description arrays the resident image was built from, back to back
    size_t desc_sizes[6] = {0, 0, 0, 0, 0, 0};
    const rm_knobs knobs = rm_knobs_from_env();   // A/B knobs and test hooks: the environment as rm_init found it
    // checked numerics (rm_trace.inc RM_CHECKED): the last render launch's verdict (the resident image's: image.exact_only), and
    // the tiles the context's launches rendered again because a lane's guard fired (device word, counted up by the kernels)
    bool last_launch_exact_only = false;
    uint32_t last_launch_scene_sig = 0;   // the scene signature the last render launch's arguments carried (KernelArgs::dead_children, bits 8-15; 0: the body for any scene)
    uint32_t *d_redo = nullptr;
    std::vector<rm_feedback> feedback;
    uint64_t feedback_clock = 0, scene_epoch = 0;
    uint64_t image_epoch = 0;         // counts the changes of the resident image or its pid map: what a swept hierarchy is built from (rm_swept_host.inc)
    std::vector<rm_tile_lists> tile_lists;
    uint32_t last_launch_grid = 0, last_launch_tail = 0;   // rm_launch_stats
    uint32_t last_launch_tiles = 0;   // rm_tile_stats: the last render launch's tiles, and whether they were classified
    bool last_launch_classified = false;
    hipStream_t last_launch_stream = nullptr;

    // device framebuffer of rm_render
    double *d_frame = nullptr;
    size_t frame_bytes = 0;
    uint32_t frame_w = 0, frame_h = 0;

    // multi-GPU frames (rm_exchange.inc)
    void *comm = nullptr;             // ncclComm_t
    void *slot_comm[RM_MAX_FRAME_SLOTS] = {};   // per frame slot: `comm` itself, or (RM_SLOT_COMMS=1) one split off it
    int n_comms = 0;                  // distinct communicators in use
    bool frame_stamps = false;        // rm_frame_timing_enable
    bool exchange_all_ranks = false;  // rm_comm_exchange: all-gather instead of the gather at rank 0
    bool comm_failed = false;         // a frame wait timed out: the communicator is abandoned, not destroyed
    bool comm_local = false;          // rank/world set without a transport (rm_comm_init with id == NULL)
    int rank = 0, world = 1;
    rm_frame_slot slots[RM_MAX_FRAME_SLOTS];

    // backproject tables (per column, per row) of the current frame geometry
    double *d_backproject = nullptr;
    size_t backproject_words = 0;
    double backproject_key[6] = {};

    // the seam into the reference's FrameBuffer (rm_hostio.inc)
    rm_hostio *hostio = nullptr;
    bool comm_stuck = false;          // a timed-out collective could not be aborted: nothing that waits for the device may run

    // ray queries (rm_query_host.inc): pid -> (index into Scene.shapes, triangle index inside the Obj) of the
    // resident image, 2 words per pid -- a buffer of its own, not part of the scene blob (the blob's size decides
    // whether the render kernels copy the scene into LDS) -- and the host variants' staging buffer
    uint32_t *d_pid_map = nullptr;
    size_t pid_map_words = 0;
    void *d_query = nullptr;
    size_t query_bytes = 0;

    // the shading launches (rm_shade_host.inc): the workgroups a compute unit holds of every shading kernel launched so far,
    // by kernel address, asked once a kernel and context
    std::vector<std::pair<const void *, int>> shade_occupancy;

    // adaptive anti-aliasing (rm_refine_host.inc): the workspace of rm_render_antialiased (grown on demand)
    void *d_refine_ws = nullptr;
    size_t refine_ws_bytes = 0;

    // the thin-lens camera (rm_lens_host.inc): the table and the frame rm_render_lens renders with (the frame grown on demand)
    void *d_lens_table = nullptr;
    void *d_lens_frame = nullptr;
    size_t lens_frame_bytes = 0;

    // progressive frames (rm_motion_host.inc): made by the first rm_render_progressive, _soft or _motion
    rm_progressive *progressive = nullptr;

    // converging frames (rm_converge_motion_host.inc): made by the first rm_render_converging, rm_render_converging_motion or rm_render_converging_moving; shares nothing with `progressive`
    rm_converging *converging = nullptr;

    // the variance-guided filter (rm_denoise_host.inc): made by the first rm_render_denoised; it reads `converging`, never writes it
    rm_denoising *denoising = nullptr;

    // swept hierarchies (rm_swept_host.inc): the one the ticks that move a shape walk, built from their velocities and shutter
    rm_tick_swept *tick_swept = nullptr;
    uint32_t swept_walked = 0;               // the last sampled-frame tick's launch walked it (rm_swept_tick_info): set by the launches, cleared by the ticks
    uint32_t swept_builds = 0;               // hierarchies tick_swept_prepare has built
    std::vector<rm_swept *> swept_handles;   // every handle rm_swept_build gave out and rm_swept_free has not taken back

    // post-process scratch
    unsigned long long *d_max = nullptr;
    uint8_t *d_rgb8 = nullptr;
    size_t rgb8_bytes = 0;
};

static void hostio_destroy(rm_ctx *ctx, bool device_ok);
static bool hostio_packs(rm_ctx *ctx, size_t band_bytes);
static void progressive_destroy(rm_ctx *ctx, bool device_ok);
static void converging_destroy(rm_ctx *ctx, bool device_ok);
static void denoising_destroy(rm_ctx *ctx, bool device_ok);
static void tick_swept_destroy(rm_ctx *ctx, bool device_ok);

static rm_status ctx_fail(rm_ctx *ctx, rm_status st, const std::string &msg) {
    if (ctx) ctx->error = msg;
    else rm_set_host_error(msg);
    return st;
}

// Nothing unwinds across the C ABI: what an entry point's body may throw (std::vector / std::function growing: bad_alloc)
// comes back as a status like every other failure.
template <class F>
static rm_status guarded(rm_ctx *ctx, const char *who, F &&body) {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": out of host memory");
    } catch (const std::exception &e) {
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": " + e.what());
    } catch (...) {
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": unexpected exception");
    }
}

// the stream's entry among the context's rm_feedback / rm_tile_lists (NULL: none yet)
template <class T>
static T *entry_of(std::vector<T> &v, hipStream_t stream) {
    T *t = nullptr;
    for (T &g : v)
        if (g.stream == stream) t = &g;
    return t;
}

#define RM_HIP(ctx, call)                                                                          \
    do {                                                                                           \
        hipError_t e__ = (call);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return ctx_fail(ctx, RM_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
    } while (0)

// Makes the context-owned device buffer *d hold `need` bytes (*have: what it holds): a larger one stays, a smaller one is
// freed and replaced, nothing is kept.  A failed allocation leaves *d NULL and *have 0.
static rm_status grow_device_buffer(rm_ctx *ctx, void **d, size_t *have, size_t need) {
    if (*have >= need) return RM_OK;
    if (*d) RM_HIP(ctx, hipFree(*d));
    *d = nullptr;
    *have = 0;
    RM_HIP(ctx, hipMalloc(d, need));
    *have = need;
    return RM_OK;
}

// The kernel instantiations live in rm_kernels.hip, one object per numeric flavour and kernel
// group (STAGED: LDS copy of the scene for the per-lane gathers; BVH: hierarchy walk for wide
// bundles; CULL: bundle culling, EDGES: its edge test for planar primitives, rm_trace.inc;
// FEEDBACK: longest tiles of the previous frame first).
#define RM_DECLARE_GROUP(g) \
    const void *rm_pick_kernel_strict_g##g(bool edges, int order, int stack, int pow_mode); \
    const void *rm_pick_kernel_fast_g##g(bool edges, int order, int stack, int pow_mode);
#define RM_DECL_PICK_O(g) \
    const void *rm_pick_kernel_strict_o_g##g(bool edges, int order, int stack, int pow_mode); \
    const void *rm_pick_kernel_fast_o_g##g(bool edges, int order, int stack, int pow_mode);
RM_DECL_PICK_O(0) RM_DECL_PICK_O(1) RM_DECL_PICK_O(2) RM_DECL_PICK_O(3)
RM_DECLARE_GROUP(0) RM_DECLARE_GROUP(1) RM_DECLARE_GROUP(2) RM_DECLARE_GROUP(3) RM_DECLARE_GROUP(4)
#undef RM_DECLARE_GROUP

const void *rm_pick_kernel(bool fast, bool staged, bool bvh, bool cull, bool edges, int order, bool feedback, int stack, int pow_mode) {
    const int group = staged ? (cull ? 1 : 0) : !bvh ? 2 : feedback ? 4 : 3;
    if (staged && (bvh || feedback)) return nullptr;         // no such kernel: small scenes have no hierarchy
    if (!staged && !cull) return nullptr;                    // scenes in global memory always cull
    switch (group) {
    case 0: return fast ? rm_pick_kernel_fast_g0(edges, order, stack, pow_mode) : rm_pick_kernel_strict_g0(edges, order, stack, pow_mode);
    case 1: return fast ? rm_pick_kernel_fast_g1(edges, order, stack, pow_mode) : rm_pick_kernel_strict_g1(edges, order, stack, pow_mode);
    case 2: return fast ? rm_pick_kernel_fast_g2(edges, order, stack, pow_mode) : rm_pick_kernel_strict_g2(edges, order, stack, pow_mode);
    case 3: return fast ? rm_pick_kernel_fast_g3(edges, order, stack, pow_mode) : rm_pick_kernel_strict_g3(edges, order, stack, pow_mode);
    default: return fast ? rm_pick_kernel_fast_g4(edges, order, stack, pow_mode) : rm_pick_kernel_strict_g4(edges, order, stack, pow_mode);
    }
}

const void *rm_pick_kernel_oriented(bool fast, bool staged, bool bvh, bool cull, bool edges, int stack, int pow_mode) {
    const int group = staged ? (cull ? 1 : 0) : !bvh ? 2 : 3;
    if (staged && bvh) return nullptr;
    if (!staged && !cull) return nullptr;
    switch (group) {
    case 0: return fast ? rm_pick_kernel_fast_o_g0(edges, 1, stack, pow_mode) : rm_pick_kernel_strict_o_g0(edges, 1, stack, pow_mode);
    case 1: return fast ? rm_pick_kernel_fast_o_g1(edges, 1, stack, pow_mode) : rm_pick_kernel_strict_o_g1(edges, 1, stack, pow_mode);
    case 2: return fast ? rm_pick_kernel_fast_o_g2(edges, 1, stack, pow_mode) : rm_pick_kernel_strict_o_g2(edges, 1, stack, pow_mode);
    default: return fast ? rm_pick_kernel_fast_o_g3(edges, 1, stack, pow_mode) : rm_pick_kernel_strict_o_g3(edges, 1, stack, pow_mode);
    }
}

extern "C" {

const char *rm_build_info(void) {
    return "rusty-marcher_amd " RM_BUILD_FLAVOR " gfx950 abi5 queries camera ranges radiance antialias lens progressive soft motion moving-shapes moving-camera swept-hierarchy swept-camera denoise reproject bounce converge-moving converge-motion converge";
}

const char *rm_last_error(const rm_ctx *ctx) {
    return ctx ? ctx->error.c_str() : rm_get_host_error();
}

rm_status rm_init(int device_ordinal, rm_ctx **out) {
    if (!out) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_init: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return ctx_fail(nullptr, RM_ERR_NO_DEVICE,
                        std::string("rm_init: no HIP device visible (") + hipGetErrorString(e) +
                            "); this backend has no CPU fallback");
    if (device_ordinal < 0 || device_ordinal >= n)
        return ctx_fail(nullptr, RM_ERR_NO_DEVICE, "rm_init: device ordinal out of range");
    rm_ctx *ctx = new rm_ctx();
    ctx->device = device_ordinal;
    auto bail = [&](const char *what, hipError_t err) {
        rm_set_host_error(std::string("rm_init: ") + what + ": " + hipGetErrorString(err));
        delete ctx;
        return RM_ERR_HIP;
    };
    if ((e = hipSetDevice(device_ordinal)) != hipSuccess) return bail("hipSetDevice", e);
    if ((e = hipGetDeviceProperties(&ctx->prop, device_ordinal)) != hipSuccess) return bail("hipGetDeviceProperties", e);
    if (std::string(ctx->prop.gcnArchName).rfind("gfx950", 0) != 0) {
        rm_set_host_error(std::string("rm_init: device is ") + ctx->prop.gcnArchName +
                          ", this library carries gfx950 code only");
        delete ctx;
        return RM_ERR_NO_DEVICE;
    }
    if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
    if ((e = hipEventCreate(&ctx->ev0)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = hipEventCreate(&ctx->ev1)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = hipMalloc(&ctx->d_max, sizeof(unsigned long long))) != hipSuccess) return bail("hipMalloc", e);
    if ((e = hipMalloc(&ctx->d_redo, sizeof(uint32_t))) != hipSuccess) return bail("hipMalloc", e);
    if ((e = hipMemset(ctx->d_redo, 0, sizeof(uint32_t))) != hipSuccess) return bail("hipMemset", e);
    *out = ctx;
    return RM_OK;
}

void rm_destroy(rm_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream && !ctx->comm_failed) (void)hipStreamSynchronize(ctx->stream);
    rm_comm_destroy(ctx);
    // A frame wait that timed out left a collective in flight.  Where RCCL could abort its
    // communicator the device drains and everything below is safe; where it could not
    // (ncclCommAbort absent or failing) the collective's kernel never ends, and hipFree /
    // hipStreamSynchronize / hipStreamDestroy -- each waits for the device -- would hang for
    // ever: the hang the timeout was there to remove.  Then nothing device-side is released:
    // the process is about to exit (RM_ERR_TIMEOUT: "report and exit") and takes it along.
    const bool device_ok = !ctx->comm_stuck;
    hostio_destroy(ctx, device_ok);
    progressive_destroy(ctx, device_ok);
    converging_destroy(ctx, device_ok);
    denoising_destroy(ctx, device_ok);
    tick_swept_destroy(ctx, device_ok);
    if (device_ok) {
        for (rm_frame_slot &s : ctx->slots) {
            // after a timed-out collective the slot's stream may never drain: leave it to process exit
            if (s.render && !ctx->comm_failed) { (void)hipStreamSynchronize(s.render); (void)hipStreamDestroy(s.render); }
            for (hipEvent_t e : {s.begun, s.rendered, s.gathered, s.exchanged})
                if (e) (void)hipEventDestroy(e);
        }
        for (rm_feedback &f : ctx->feedback)
            if (f.block) (void)hipFree(f.block);
        for (rm_tile_lists &t : ctx->tile_lists) {
            if (t.block) (void)hipFree(t.block);
            if (t.order_block) (void)hipFree(t.order_block);
            if (t.hint) (void)hipHostFree(t.hint);
        }
        if (ctx->d_scene) (void)hipFree(ctx->d_scene);
        if (ctx->d_frame) (void)hipFree(ctx->d_frame);
        if (ctx->d_backproject) (void)hipFree(ctx->d_backproject);
        if (ctx->d_pid_map) (void)hipFree(ctx->d_pid_map);
        if (ctx->d_query) (void)hipFree(ctx->d_query);
        if (ctx->d_refine_ws) (void)hipFree(ctx->d_refine_ws);
        if (ctx->d_lens_table) (void)hipFree(ctx->d_lens_table);
        if (ctx->d_lens_frame) (void)hipFree(ctx->d_lens_frame);
        if (ctx->d_max) (void)hipFree(ctx->d_max);
        if (ctx->d_redo) (void)hipFree(ctx->d_redo);
        if (ctx->d_rgb8) (void)hipFree(ctx->d_rgb8);
        if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
        if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
        if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    }
    delete ctx;
}

rm_status rm_device_info(rm_ctx *ctx, char *name_buf, size_t buflen, int *n_cus, size_t *lds_bytes) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_device_info: NULL ctx");
    if (name_buf && buflen) std::snprintf(name_buf, buflen, "%s (%s)", ctx->prop.name, ctx->prop.gcnArchName);
    if (n_cus) *n_cus = ctx->prop.multiProcessorCount;
    if (lds_bytes) *lds_bytes = ctx->prop.sharedMemPerBlock;
    return RM_OK;
}

// The queries' pid -> (shape, element) map of a new resident image into its device buffer (the device is idle: the
// caller has synchronised it).
static rm_status upload_pid_map(rm_ctx *ctx, const std::vector<uint32_t> &map) {
    const size_t words = std::max<size_t>(map.size(), 2u);
    if (ctx->pid_map_words < words) {
        if (ctx->d_pid_map) RM_HIP(ctx, hipFree(ctx->d_pid_map));
        ctx->d_pid_map = nullptr;
        ctx->pid_map_words = 0;
        RM_HIP(ctx, hipMalloc(&ctx->d_pid_map, words * sizeof(uint32_t)));
        ctx->pid_map_words = words;
    }
    if (!map.empty()) RM_HIP(ctx, hipMemcpy(ctx->d_pid_map, map.data(), map.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return RM_OK;
}

static rm_status rm_scene_upload_impl(rm_ctx *ctx, const rm_scene_desc *d) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_scene_upload: NULL ctx");
    if (!d) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "rm_scene_upload: NULL desc");
    // (before the comparison below reads the arrays; rm_build_image refuses such a description with the same text)
    if (!rm_desc_arrays_present(d)) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "rm_scene_upload: NULL array with non-zero count");

    // The reference's hosts hand the whole Scene to every render() call (main.rs:331-333).  A
    // description byte-identical to the one the resident image was built from (cameras apart:
    // the camera travels as a kernel argument) needs no work at all.  Identity is decided on
    // the bytes themselves -- the context keeps a copy of the arrays it last built from and
    // compares in place, one pass, no hashing: a digest can collide, and a collision would
    // silently render the old scene.
    ctx->upload_calls++;
    const struct { const void *p; size_t bytes; } parts[6] = {
        {d->shapes, (size_t)d->n_shapes * sizeof(rm_shape_ref)},   {d->spheres, (size_t)d->n_spheres * sizeof(rm_sphere)},
        {d->polygons, (size_t)d->n_polygons * sizeof(rm_polygon)}, {d->polygon_vertices, (size_t)d->n_polygon_vertices * sizeof(rm_vec3)},
        {d->triangles, (size_t)d->n_triangles * sizeof(rm_triangle)}, {d->lights, (size_t)d->n_lights * sizeof(rm_light)}};
    auto same_description = [&]() {
        size_t off = 0;
        for (int i = 0; i < 6; i++) {
            if (ctx->desc_sizes[i] != parts[i].bytes) return false;
            if (parts[i].bytes && std::memcmp(ctx->desc_bytes.data() + off, parts[i].p, parts[i].bytes) != 0) return false;
            off += parts[i].bytes;
        }
        return true;
    };
    auto keep_description = [&]() {
        size_t total = 0;
        for (int i = 0; i < 6; i++) total += parts[i].bytes;
        ctx->desc_bytes.resize(total);
        size_t off = 0;
        for (int i = 0; i < 6; i++) {
            if (parts[i].bytes) std::memcpy(ctx->desc_bytes.data() + off, parts[i].p, parts[i].bytes);
            ctx->desc_sizes[i] = parts[i].bytes;
            off += parts[i].bytes;
        }
    };
    if (ctx->have_scene && same_description()) {
        ctx->camera = d->camera;
        return RM_OK;
    }

    rm_image img;
    std::string refusal;
    if (rm_status bst = rm_build_image(d, rm_image_options{!ctx->knobs.disable_bvh, ctx->knobs.shadow_masks}, img, refusal))
        return ctx_fail(ctx, bst, refusal);
    img.scene_sig = rm_scene_signature(img.H, img.blob.data());   // (the planner's verdict on the image: once per upload)
    rm_image &resident = ctx->image;

    // (a different description that builds the same device image -- an edit undone -- is not copied either)
    if (ctx->have_scene && img.blob == resident.blob && std::memcmp(&img.H, &resident.H, sizeof img.H) == 0) {
        // (the same image can come from another shape list -- one Obj of two triangles, or two of one --: the
        // queries' map is the image's too, and goes across alone where only it differs)
        if (img.pid_map != resident.pid_map) {
            RM_HIP(ctx, hipSetDevice(ctx->device));
            RM_HIP(ctx, hipDeviceSynchronize());          // a query may still be reading the old map
            if (rm_status mst = upload_pid_map(ctx, img.pid_map)) return mst;
            resident.pid_map.swap(img.pid_map);
            ctx->image_epoch++;
        }
        ctx->camera = d->camera;
        keep_description();
        return RM_OK;
    }
    RM_HIP(ctx, hipSetDevice(ctx->device));
    RM_HIP(ctx, hipDeviceSynchronize());   // a render (on any stream: the caller's, a frame slot's) may still be reading the old blob
    ctx->upload_copies++;
    if (ctx->d_scene_words < img.blob.size()) {
        if (ctx->d_scene) RM_HIP(ctx, hipFree(ctx->d_scene));
        ctx->d_scene = nullptr;
        RM_HIP(ctx, hipMalloc(&ctx->d_scene, img.blob.size() * sizeof(double)));
        ctx->d_scene_words = img.blob.size();
    }
    RM_HIP(ctx, hipMemcpy(ctx->d_scene, img.blob.data(), img.blob.size() * sizeof(double), hipMemcpyHostToDevice));
    if (rm_status mst = upload_pid_map(ctx, img.pid_map)) {
        ctx->have_scene = false;                             // (the blob went across, its map did not: no half image)
        return mst;
    }
    std::swap(resident, img);                                // both copies are across: the new image is the resident one
    ctx->camera = d->camera;
    ctx->have_scene = true;
    ctx->scene_epoch++;                                      // (the feedback of another scene's frames is void)
    ctx->image_epoch++;
    keep_description();
    return RM_OK;
}

rm_status rm_scene_upload(rm_ctx *ctx, const rm_scene_desc *d) {
    return guarded(ctx, "rm_scene_upload", [&]() { return rm_scene_upload_impl(ctx, d); });
}

// The tiles the context's render launches have rendered again so far because a lane's guard fired (waits for the device),
// and whether the last render launch was exact only.
extern "C" rm_status rmi_redone_tiles(rm_ctx *ctx, uint64_t *redone, uint32_t *last_exact_only) {
    if (!ctx || !redone) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "rmi_redone_tiles: NULL argument");
    RM_HIP(ctx, hipSetDevice(ctx->device));
    RM_HIP(ctx, hipDeviceSynchronize());
    uint32_t n = 0;
    RM_HIP(ctx, hipMemcpy(&n, ctx->d_redo, sizeof n, hipMemcpyDeviceToHost));
    *redone = n;
    if (last_exact_only) *last_exact_only = ctx->last_launch_exact_only ? 1u : 0u;
    return RM_OK;
}

// Test hook, not part of the ABI (tests/test_gpu_scene_sig.py): the scene signature in the argument block the context's last
// render launch went out with -- what the kernel read, not what a plan made elsewhere says -- and the resident image's.
extern "C" rm_status rmi_last_scene_sig(rm_ctx *ctx, uint32_t *launched, uint32_t *resident) {
    if (!ctx || !launched || !resident) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "rmi_last_scene_sig: NULL argument");
    *launched = ctx->last_launch_scene_sig;
    *resident = ctx->have_scene ? ctx->image.scene_sig : 0u;
    return RM_OK;
}

rm_status rm_scene_uploads(rm_ctx *ctx, uint64_t *calls, uint64_t *copies) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_scene_uploads: NULL ctx");
    if (calls) *calls = ctx->upload_calls;
    if (copies) *copies = ctx->upload_copies;
    return RM_OK;
}

rm_status rm_camera_update(rm_ctx *ctx, rm_vec3 camera) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_camera_update: NULL ctx");
    if (!ctx->have_scene) return ctx_fail(ctx, RM_ERR_NO_SCENE, "rm_camera_update: no scene uploaded");
    ctx->camera = camera;   // the camera travels as a kernel argument
    return RM_OK;
}

// The fixed view: the reference's backproject looks down -z with +y up.
static const rm_camera_basis k_fixed_view{{1., 0., 0.}, {0., 1., 0.}, {0., 0., -1.}};

static void set_basis(rm_ctx *ctx, const rm_camera_basis &b) {
    // (== component by component: a -0 that a cross product leaves counts as 0, and the state then holds the fixed view's own words)
    const bool fixed = b.right.x == 1. && b.right.y == 0. && b.right.z == 0. && b.up.x == 0. && b.up.y == 1. && b.up.z == 0. &&
                       b.forward.x == 0. && b.forward.y == 0. && b.forward.z == -1.;
    ctx->oriented = !fixed;
    ctx->basis = fixed ? k_fixed_view : b;
}

rm_status rm_camera_orient(rm_ctx *ctx, const rm_camera_basis *basis) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_camera_orient: NULL ctx");
    if (!basis) { set_basis(ctx, k_fixed_view); return RM_OK; }
    if (rm_status st = rm_camera_basis_check(basis)) return ctx_fail(ctx, st, std::string("rm_camera_orient: ") + rm_get_host_error());
    set_basis(ctx, *basis);   // the basis travels as kernel arguments
    return RM_OK;
}

rm_status rm_camera_look_at(rm_ctx *ctx, rm_vec3 eye, rm_vec3 target, rm_vec3 up_hint) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_camera_look_at: NULL ctx");
    if (!ctx->have_scene) return ctx_fail(ctx, RM_ERR_NO_SCENE, "rm_camera_look_at: no scene uploaded");
    rm_camera_basis b;
    if (rm_status st = rm_camera_basis_look_at(eye, target, up_hint, &b)) return ctx_fail(ctx, st, std::string("rm_camera_look_at: ") + rm_get_host_error());
    ctx->camera = eye;
    set_basis(ctx, b);
    return RM_OK;
}

rm_status rm_camera_get(rm_ctx *ctx, rm_vec3 *position, rm_camera_basis *basis, int *oriented) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_camera_get: NULL ctx");
    if (position) *position = ctx->camera;
    if (basis) *basis = ctx->basis;
    if (oriented) *oriented = ctx->oriented ? 1 : 0;
    return RM_OK;
}

// Validates params and computes the band; shared by the render entry points.
static rm_status check_params(rm_ctx *ctx, const rm_params *p, rm_band *band) {
    if (!p) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "render: NULL params");
    if (!ctx->have_scene) return ctx_fail(ctx, RM_ERR_NO_SCENE, "render: no scene uploaded (rm_scene_upload)");
    if (p->patch_size != RM_PATCH_SIZE) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "render: patch_size must be 32 (renderer.rs:47)");
    if (p->max_depth > RM_MAX_DEPTH) return ctx_fail(ctx, RM_ERR_DEPTH, "render: max_depth above RM_MAX_DEPTH");
    if (p->frame_width == 0 || p->frame_height == 0) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "render: empty frame");
    if (p->frame_width % RM_PATCH_SIZE != 0)
        return ctx_fail(ctx, RM_ERR_DIMENSIONS,
                        "render: frame width is not a multiple of 32; the reference's scatter "
                        "(renderer.rs:92-108) indexes out of bounds and panics");
    if (!rm_band_of(*p, band)) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "render: patch_row_begin > patch_row_end");
    return RM_OK;
}

// backproject (renderer.rs:128-135): `2 (x / width - 0.5) half_fov ratio` per column and
// `-2 (y / height - 0.5) half_fov` per row, tabulated with the operations the kernel used to
// perform per pixel, in their order (this file is compiled with -ffp-contract=off): the same
// IEEE results.  Rebuilt when the Renderer or the frame geometry changes.
static rm_status backproject_tables(rm_ctx *ctx, const rm_params *p) {
    const double key[6] = {p->width, p->height, p->half_fov, p->ratio, (double)p->frame_width, (double)p->frame_height};
    if (ctx->d_backproject && std::memcmp(key, ctx->backproject_key, sizeof key) == 0) return RM_OK;
    std::vector<double> t((size_t)p->frame_width + p->frame_height);
    for (uint32_t x = 0; x < p->frame_width; x++) t[x] = 2. * ((double)x / p->width - 0.5) * p->half_fov * p->ratio;
    for (uint32_t y = 0; y < p->frame_height; y++) t[p->frame_width + y] = -2. * ((double)y / p->height - 0.5) * p->half_fov;
    RM_HIP(ctx, hipDeviceSynchronize());                       // a launch in flight may still read the old tables
    if (ctx->backproject_words < t.size()) {
        if (ctx->d_backproject) RM_HIP(ctx, hipFree(ctx->d_backproject));
        ctx->d_backproject = nullptr;
        RM_HIP(ctx, hipMalloc(&ctx->d_backproject, t.size() * sizeof(double)));
        ctx->backproject_words = t.size();
    }
    RM_HIP(ctx, hipMemcpy(ctx->d_backproject, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    std::memcpy(ctx->backproject_key, key, sizeof key);
    return RM_OK;
}

static constexpr uint32_t RM_FEEDBACK_STREAMS = 8, RM_CLASSIFY_STREAMS = 8;

// The feedback sets of this stream's launches, as the plan wants them (created, or cleared when the
// geometry or the scene changed: the first frame then has no list).
static rm_status feedback_for(rm_ctx *ctx, hipStream_t stream, const rm_launch_plan &P, rm_feedback **out) {
    rm_feedback *f = entry_of(ctx->feedback, stream);
    if (!f) {
        if (ctx->feedback.size() >= RM_FEEDBACK_STREAMS) {         // forget the stream used longest ago
            size_t old = 0;
            for (size_t i = 1; i < ctx->feedback.size(); i++)
                if (ctx->feedback[i].used < ctx->feedback[old].used) old = i;
            if (ctx->feedback[old].block) RM_HIP(ctx, hipFree(ctx->feedback[old].block));   // (waits for the device)
            ctx->feedback.erase(ctx->feedback.begin() + (long)old);
        }
        ctx->feedback.emplace_back();
        f = &ctx->feedback.back();
        f->stream = stream;
    }
    f->used = ++ctx->feedback_clock;
    if (P.feedback_reset) {
        f->s.valid = false;
        if (!f->block || f->set_bytes != P.feedback_set_bytes) {
            if (f->block) RM_HIP(ctx, hipFree(f->block));
            f->block = nullptr;
            RM_HIP(ctx, hipMalloc(&f->block, P.feedback_bytes));
        }
        f->set_bytes = P.feedback_set_bytes;
        RM_HIP(ctx, hipMemsetAsync(f->block, 0, P.feedback_bytes, stream));
    }
    *out = f;
    return RM_OK;
}

static rm_status tile_lists_for(rm_ctx *ctx, hipStream_t stream, uint32_t n_tiles, rm_tile_lists **out) {
    rm_tile_lists *t = entry_of(ctx->tile_lists, stream);
    if (!t) {
        if (ctx->tile_lists.size() >= RM_CLASSIFY_STREAMS) {       // forget the stream used longest ago
            size_t old = 0;
            for (size_t i = 1; i < ctx->tile_lists.size(); i++)
                if (ctx->tile_lists[i].used < ctx->tile_lists[old].used) old = i;
            if (ctx->tile_lists[old].block) RM_HIP(ctx, hipFree(ctx->tile_lists[old].block));   // (waits for the device)
            if (ctx->tile_lists[old].order_block) RM_HIP(ctx, hipFree(ctx->tile_lists[old].order_block));
            if (ctx->tile_lists[old].hint) RM_HIP(ctx, hipHostFree(ctx->tile_lists[old].hint));
            ctx->tile_lists.erase(ctx->tile_lists.begin() + (long)old);
        }
        ctx->tile_lists.emplace_back();
        t = &ctx->tile_lists.back();
        t->stream = stream;
    }
    t->used = ++ctx->feedback_clock;
    if (!t->block || t->cap < n_tiles) {
        if (t->block) RM_HIP(ctx, hipFree(t->block));             // (waits for the device: nothing reads the old masks any more)
        t->block = nullptr;
        t->cap = n_tiles;
        RM_HIP(ctx, hipMalloc(&t->block, (size_t)n_tiles * sizeof(unsigned long long)));
    }
    *out = t;
    return RM_OK;
}

// A wave that gives up a wait that cannot fail (the dispatch order of its own launch, 10 ms) says so in page-locked memory
// and renders nothing: that frame is void.  Reported once, by the first call that has waited for the device since -- the
// synchronous render calls and rm_frame_wait report the void frame itself -- or by the next launch on the stream.
static rm_status void_frame_check(rm_ctx *ctx, const char *who) {
    for (rm_tile_lists &t : ctx->tile_lists)
        if (t.hint) {
            const unsigned long long e = *(volatile unsigned long long *)(t.hint + 1);
            if (e) {
                *(volatile unsigned long long *)(t.hint + 1) = 0ull;
                return ctx_fail(ctx, RM_ERR_HIP, std::string(who) + ": launch " + std::to_string((uint32_t)(e >> 32)) +
                                                     " of its stream gave up waiting for its own classification (that frame is void)");
            }
        }
    return RM_OK;
}

static rm_plan_scene plan_scene_of(const rm_ctx *ctx) {
    const rm_image &img = ctx->image;
    return rm_plan_scene{&img.H, ctx->scene_epoch, img.occ_camera_limit, img.integer_exponents, ctx->oriented,
                         ctx->camera, &ctx->basis, (uint32_t)ctx->prop.multiProcessorCount, img.exact_only, img.dead_camera_limit, img.scene_sig};
}

static rm_status no_kernel(rm_ctx *ctx) { return ctx_fail(ctx, RM_ERR_INVALID_ARG, "render: no kernel for this scene / depth combination"); }

// Which kernel instantiation a render of the resident scene with these params launches (the first step of plan_launch).
static rm_status choose_kernel(rm_ctx *ctx, const rm_params *p, uint32_t tiles, rm_kernel_choice *k) {
    return choose_kernel(ctx->knobs, plan_scene_of(ctx), *p, tiles, k) ? RM_OK : no_kernel(ctx);
}

// RM_DEBUG_TAIL (diagnostic: waits for the launch): the counters of the launch that has just gone out, and the order it laid out
static rm_status dump_order(rm_ctx *ctx, const rm_launch_plan &P, hipStream_t stream) {
    const KernelArgs &a = P.args;
    uint32_t c[RM_ORD_BUCKETS] = {}, c1[RM_ORD_BUCKETS] = {}, raw[RM_ORD_ARRIVE] = {};
    RM_HIP(ctx, hipStreamSynchronize(stream));
    RM_HIP(ctx, hipMemcpy(raw, a.ord_cnt, sizeof raw, hipMemcpyDeviceToHost));
    for (uint32_t b = 0; b < RM_ORD_BUCKETS; b++)
        for (uint32_t u = 0; u < RM_ORD_SUBS; u++) { c[b] += raw[(b * RM_ORD_SUBS + u) * RM_ORD_LINE]; c1[b] += raw[RM_ORD_FIRST + (b * RM_ORD_SUBS + u) * RM_ORD_LINE]; }
    uint32_t lit = 0;
    for (uint32_t b = 0; b < RM_ORD_SKY; b++) lit += c[b];
    std::fprintf(stderr, "[rm_order] launch %u keys %u: %u classifying workgroups x %u, first round %u waves, %u + %u sky places; tail %u, room to hand on %u, handed on %u; buckets", a.launch_seq, a.key_mode,
                 a.cls_blocks, a.cls_iters, a.n_static, lit, c[RM_ORD_SKY], a.tail_patches, a.ov_cap, a.tail_patches > c[RM_ORD_SKY] ? std::min(a.ov_cap, a.tail_patches - c[RM_ORD_SKY]) : 0u);
    for (uint32_t b = 0; b < RM_ORD_BUCKETS; b++) std::fprintf(stderr, " %u", c[b]);
    std::fprintf(stderr, " | first round's");
    for (uint32_t b = 0; b < RM_ORD_BUCKETS; b++) std::fprintf(stderr, " %u", c1[b]);
    // (the order this launch laid out: every place taken, by a patch of its own)
    const uint32_t n_pat = a.n_tiles / 16u, n_dyn_ = n_pat - a.n_static / 16u;
    std::vector<uint32_t> fl(n_dyn_);
    RM_HIP(ctx, hipMemcpy(fl.data(), a.ord_flat, n_dyn_ * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::vector<uint8_t> seen(n_pat, 0);
    uint32_t untagged = 0, twice = 0, bad = 0;
    for (uint32_t v : fl) {
        if ((v >> RM_ORD_TAG_SHIFT) != a.ord_tag) { untagged++; continue; }
        const uint32_t pch = v & (RM_ORD_SKY_BIT - 1u);
        if (pch >= n_pat) { bad++; continue; }
        twice += seen[pch]; seen[pch] = 1;
    }
    std::fprintf(stderr, " | order laid out: %u places, %u without the tag, %u patches twice, %u out of range; dispatched by %s order; places written %s\n", n_dyn_, untagged, twice, bad,
                 a.ord_read == a.ord_flat ? "its own" : "its predecessor's", a.ord_rec ? "at the grid's end" : "by the classifying workgroups");
    return RM_OK;
}

#if defined(RM_EXP_STAMPS) || defined(RM_EXP_PHASES)
// The diagnostic builds' stamps: 48 bytes a wave, given to the launch, and (RM_DEBUG_STAMPS=path) written out once it is over.
static rm_status stamps_begin(rm_ctx *ctx, rm_launch_plan &P, hipStream_t stream) {
    const size_t n_waves = (size_t)P.grid * P.k.mode.waves;
    RM_HIP(ctx, hipMalloc(&P.args.debug_stamps, n_waves * 48));
    RM_HIP(ctx, hipMemsetAsync(P.args.debug_stamps, 0, n_waves * 48, stream));
    return RM_OK;
}
static rm_status stamps_end(rm_ctx *ctx, const rm_launch_plan &P, hipStream_t stream) {
    const KernelArgs &a = P.args;
    const size_t n_waves = (size_t)P.grid * P.k.mode.waves;
    RM_HIP(ctx, hipStreamSynchronize(stream));
    if (const char *path = std::getenv("RM_DEBUG_STAMPS")) {
        std::fprintf(stderr, "stamps: grid %u cls_blocks %u n_static %u n_tiles %u tail_patches %u tail_q %u ov_cap %u key_mode %u\n", P.grid, a.cls_blocks, a.ord_cnt ? a.n_static : 0u, a.n_tiles, a.tail_patches, a.tail_q, a.ov_cap, a.key_mode);
        std::vector<unsigned long long> h(n_waves * 4);
        RM_HIP(ctx, hipMemcpy(h.data(), a.debug_stamps, n_waves * 32, hipMemcpyDeviceToHost));
        if (FILE *f = std::fopen(path, "wb")) { std::fwrite(h.data(), 8, h.size(), f); std::fclose(f); }
        // (<path>.ext: per wave the tile it rendered and the tile's classification word)
        std::vector<unsigned long long> x(n_waves * 2);
        RM_HIP(ctx, hipMemcpy(x.data(), a.debug_stamps + n_waves * 4, n_waves * 16, hipMemcpyDeviceToHost));
        if (FILE *f = std::fopen((std::string(path) + ".ext").c_str(), "wb")) { std::fwrite(x.data(), 8, x.size(), f); std::fclose(f); }
    }
    RM_HIP(ctx, hipFree(a.debug_stamps));
    return RM_OK;
}
#endif

// One render launch: plan it (rm_plan.cpp decides everything, from the stream's bookkeeping as it stands), do the device work
// the plan lists, launch, and only then store the bookkeeping the plan leaves -- an error on the way leaves the stream's as it was.
static rm_status launch_render(rm_ctx *ctx, const rm_params *p, const rm_band &band, double *d_frame,
                               uint8_t *d_frame8, hipStream_t stream) {
    const uint32_t n_rows = band.count();
    if (n_rows == 0) return RM_OK;
    if (p->max_depth == 0) {
        // one fill per run of consecutive owned rows (a single run unless the band is strided)
        const uint32_t run = band.stride == 1 ? n_rows : 1u;
        for (uint32_t k = 0; k < n_rows; k += run) {
            const size_t first_px = (size_t)((p->flags & RM_FLAG_F64_COMPACT) ? k : band.begin + k * band.stride) * 32u * p->frame_width;
            const size_t n_px = (size_t)run * 32u * p->frame_width;
            hipLaunchKernelGGL(rm_fill_band_kernel, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, stream, d_frame,
                               first_px, n_px, p->background.x, p->background.y, p->background.z);
            RM_HIP(ctx, hipGetLastError());
        }
        return RM_OK;
    }
    rm_status bst = backproject_tables(ctx, p);
    if (bst != RM_OK) return bst;
    static const rm_stream_state no_launches;
    static const rm_feedback_state no_feedback;
    rm_tile_lists *tl = entry_of(ctx->tile_lists, stream);
    rm_feedback *fb = entry_of(ctx->feedback, stream);
    // (the sky tail's hint: page-locked memory, read without a wait)
    const unsigned long long hint = tl && tl->hint ? *(volatile unsigned long long *)tl->hint : 0ull;
    rm_launch_plan P;
    if (!plan_launch(ctx->knobs, plan_scene_of(ctx), *p, band, tl ? tl->s : no_launches, tl ? tl->order_cap : 0u, fb ? fb->s : no_feedback, hint, &P))
        return no_kernel(ctx);
    // (a wave of an earlier launch gave up a wait that cannot fail: that frame is void -- said once)
    if (P.ordered)
        if (rm_status vst = void_frame_check(ctx, "render")) return vst;

    // the buffers the plan wants
    if (P.feedback)
        if (rm_status fst = feedback_for(ctx, stream, P, &fb)) return fst;
    if (P.classify) {
        if (rm_status cst = tile_lists_for(ctx, stream, P.args.n_tiles, &tl)) return cst;
        if (P.clear_masks) RM_HIP(ctx, hipMemsetAsync(tl->block, 0, (size_t)tl->cap * sizeof(unsigned long long), stream));
    }
    if (P.ordered) {
        if (tl->order_cap < P.order_patches) {
            if (tl->order_block) RM_HIP(ctx, hipFree(tl->order_block));     // (waits for the device)
            tl->order_block = nullptr;
            tl->order_cap = 0;
            RM_HIP(ctx, hipMalloc(&tl->order_block, rm_order_layout{P.order_cap}.bytes()));
            tl->order_cap = P.order_cap;
        }
        const rm_order_layout L{tl->order_cap};
        if (P.order_clear == rm_launch_plan::ORDER_CLEAR_ALL)
            RM_HIP(ctx, hipMemsetAsync(tl->order_block, 0, L.bytes(), stream));
        else if (P.order_clear == rm_launch_plan::ORDER_CLEAR_FLAT)
            RM_HIP(ctx, hipMemsetAsync(static_cast<uint32_t *>(tl->order_block) + L.flat(0), 0, 2u * L.cap * sizeof(uint32_t), stream));
        if (!tl->hint) {
            RM_HIP(ctx, hipHostMalloc((void **)&tl->hint, 2u * sizeof(unsigned long long), hipHostMallocDefault));
            tl->hint[0] = tl->hint[1] = 0ull;
        }
    }

    // the arguments' addresses, now that every buffer is there
    KernelArgs &a = P.args;
    char *base[RM_BUF_COUNT] = {};
    if (P.classify) { base[RM_BUF_MASKS] = static_cast<char *>(tl->block); base[RM_BUF_ORDER] = static_cast<char *>(tl->order_block); base[RM_BUF_HINT] = reinterpret_cast<char *>(tl->hint); }
    if (P.feedback) base[RM_BUF_FEEDBACK] = static_cast<char *>(fb->block);
    for (uint32_t i = 0; i < P.n_refs; i++) {
        char *at = base[P.refs[i].buf] + P.refs[i].offset;
        std::memcpy(reinterpret_cast<char *>(&a) + P.refs[i].field, &at, sizeof at);
    }
    a.bp_x = ctx->d_backproject;
    a.bp_y = ctx->d_backproject + p->frame_width;
    a.frame8 = d_frame8;
    a.redo_count = ctx->d_redo;

    if (P.cls_fn) {
        P.cls_args.tile_mask = tl->mask();
        void *cargs[] = {(void *)&ctx->d_scene, (void *)&a, (void *)&P.cls_args};
        RM_HIP(ctx, hipLaunchKernel(P.cls_fn, dim3(P.cls_grid), dim3(64), cargs, 0, stream));
    }
#if defined(RM_EXP_STAMPS) || defined(RM_EXP_PHASES)
    if (rm_status sst = stamps_begin(ctx, P, stream)) return sst;
#endif
    void *args[] = {(void *)&ctx->d_scene, (void *)&a, (void *)&d_frame};
    RM_HIP(ctx, hipLaunchKernel(P.k.fn, dim3(P.grid), dim3(P.block), args, P.lds_bytes, stream));

    // the launch is out: the stream's bookkeeping moves on
    if (P.classify) tl->s = P.after;
    if (P.feedback) fb->s = P.feedback_after;
    ctx->last_launch_tiles = a.n_tiles;
    ctx->last_launch_classified = P.classify;
    ctx->last_launch_stream = stream;
    ctx->last_launch_grid = P.grid;
    ctx->last_launch_tail = a.tail_patches;
    ctx->last_launch_exact_only = P.exact_only;
    ctx->last_launch_scene_sig = (a.dead_children >> RM_SCENE_SIG_SHIFT) & RM_SCENE_SIG_MASK;
    if (ctx->knobs.debug_tail && P.ordered)
        if (rm_status dst = dump_order(ctx, P, stream)) return dst;
#if defined(RM_EXP_STAMPS) || defined(RM_EXP_PHASES)
    if (rm_status sst = stamps_end(ctx, P, stream)) return sst;
#endif
    return RM_OK;
}

static rm_status rm_render_device_impl(rm_ctx *ctx, const rm_params *params, void *device_rgb, void *hip_stream) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_render_device: NULL ctx");
    if (!device_rgb) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "rm_render_device: NULL device buffer");
    rm_band band;
    rm_status st = check_params(ctx, params, &band);
    if (st != RM_OK) return st;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)hip_stream;   // NULL is HIP's default stream, as in any HIP API
    return launch_render(ctx, params, band, (double *)device_rgb, nullptr, s);
}

rm_status rm_render_device(rm_ctx *ctx, const rm_params *params, void *device_rgb, void *hip_stream) {
    return guarded(ctx, "rm_render_device", [&]() { return rm_render_device_impl(ctx, params, device_rgb, hip_stream); });
}

static rm_status rm_render_device_u8_impl(rm_ctx *ctx, const rm_params *params, void *device_rgb, void *device_rgb8,
                              void *hip_stream) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_render_device_u8: NULL ctx");
    if (!device_rgb || !device_rgb8) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "rm_render_device_u8: NULL device buffer");
    rm_band band;
    rm_status st = check_params(ctx, params, &band);
    if (st != RM_OK) return st;
    if (params->max_depth == 0)
        return ctx_fail(ctx, RM_ERR_DEPTH, "rm_render_device_u8: max_depth 0 renders no ray; use rm_render_device + rm_postprocess");
    RM_HIP(ctx, hipSetDevice(ctx->device));
    return launch_render(ctx, params, band, (double *)device_rgb, (uint8_t *)device_rgb8, (hipStream_t)hip_stream);
}

rm_status rm_render_device_u8(rm_ctx *ctx, const rm_params *params, void *device_rgb, void *device_rgb8,
                              void *hip_stream) {
    return guarded(ctx, "rm_render_device_u8", [&]() { return rm_render_device_u8_impl(ctx, params, device_rgb, device_rgb8, hip_stream); });
}

static rm_status rm_render_impl(rm_ctx *ctx, const rm_params *params, double *host_rgb, rm_timing *timing) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_render: NULL ctx");
    const auto t_begin = std::chrono::steady_clock::now();
    rm_band band;
    rm_status st = check_params(ctx, params, &band);
    if (st != RM_OK) return st;
    if (params->flags & (RM_FLAG_F64_COMPACT | RM_FLAG_U8_COMPACT))
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, "rm_render: the packed layouts are for rm_render_device* (caller-owned device buffers)");
    RM_HIP(ctx, hipSetDevice(ctx->device));

    const size_t need = (size_t)params->frame_width * params->frame_height * 3u * sizeof(double);
    if (ctx->frame_bytes != need || ctx->frame_w != params->frame_width || ctx->frame_h != params->frame_height) {
        RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->d_frame) RM_HIP(ctx, hipFree(ctx->d_frame));
        ctx->d_frame = nullptr;
        ctx->frame_bytes = 0;
        RM_HIP(ctx, hipMalloc(&ctx->d_frame, need));
        // create_frame_buffer zero-fills (framebuffer.rs:12-22)
        RM_HIP(ctx, hipMemsetAsync(ctx->d_frame, 0, need, ctx->stream));
        ctx->frame_bytes = need;
        ctx->frame_w = params->frame_width;
        ctx->frame_h = params->frame_height;
    }

    // One launch, then the copy.  The copy IS the call: 48.7 MB of f64 at 1080p take 0.87-0.93 ms
    // at the 52-56 GB/s this PCIe link delivers device -> host, the kernel 0.08 ms.  Rendering
    // in sub-bands and copying each while the next renders was measured and dropped
    // (profiles/r02_host_copy.txt: 0.97-1.04 ms either way).  What does help is not sending the
    // black patches (rm_hostio.inc): frames of 2 MB and more take that path, into flat memory as
    // into rows of rows; smaller ones are copied as they are.
    const size_t row_bytes = (size_t)params->frame_width * 3u * sizeof(double);
    const uint32_t n_rows = band.count();
    if (host_rgb && n_rows > 0 && hostio_packs(ctx, (size_t)n_rows * 32u * row_bytes)) {
        std::vector<double *> rows(params->frame_height);
        for (uint32_t y = 0; y < params->frame_height; y++) rows[y] = host_rgb + (size_t)y * params->frame_width * 3u;
        return rm_render_rows(ctx, params, rows.data(), timing);
    }
    RM_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    st = launch_render(ctx, params, band, ctx->d_frame, nullptr, ctx->stream);
    if (st != RM_OK) return st;
    RM_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));

    double d2h_ms = 0.;
    if (host_rgb && n_rows > 0) {
        // Only the owned rows are copied: rows below the last whole patch row keep the
        // caller's previous contents, as in the reference (renderer.rs:53).
        RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const auto t0 = std::chrono::steady_clock::now();
        const uint32_t run = band.stride == 1 ? n_rows : 1u;               // consecutive owned patch rows per copy
        for (uint32_t k = 0; k < n_rows; k += run) {
            const size_t off = (size_t)(band.begin + k * band.stride) * 32u * row_bytes;
            RM_HIP(ctx, hipMemcpy((char *)host_rgb + off, (const char *)ctx->d_frame + off, (size_t)run * 32u * row_bytes,
                                  hipMemcpyDeviceToHost));
        }
        d2h_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    } else {
        RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (rm_status vst = void_frame_check(ctx, "rm_render")) return vst;
    if (timing) {
        float ms = 0.f;
        RM_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        timing->kernel_ms = ms;
        timing->d2h_ms = d2h_ms;
        timing->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    }
    return RM_OK;
}

rm_status rm_render(rm_ctx *ctx, const rm_params *params, double *host_rgb, rm_timing *timing) {
    return guarded(ctx, "rm_render", [&]() { return rm_render_impl(ctx, params, host_rgb, timing); });
}

rm_status rm_kernel_name(rm_ctx *ctx, const rm_params *params, char *buf, size_t buflen) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_kernel_name: NULL ctx");
    if (!buf || buflen == 0) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "rm_kernel_name: NULL buffer");
    rm_band band;
    rm_status st = check_params(ctx, params, &band);
    if (st != RM_OK) return st;
    if (params->max_depth == 0) { std::snprintf(buf, buflen, "rm_fill_band_kernel"); return RM_OK; }
    rm_kernel_choice k;
    st = choose_kernel(ctx, params, band.count() * (params->frame_width / RM_PATCH_SIZE) * 16u, &k);
    if (st != RM_OK) return st;
    // the name rocprofv3's kernel trace shows (template arguments in declaration order)
    // (the oriented camera's kernels: namespaces of their own, always the instantiation with the dispatch order)
    std::snprintf(buf, buflen, "%s%s::rm_render_static<%d, %d, %d, %d, %s, %s, %s, %s, %s, %s>", k.fast ? "rmdev_fast" : "rmdev_strict", ctx->oriented ? "_o" : "", k.stack,
                  k.pow_mode, k.mode.waves, k.mode.per_wave, k.staged ? "true" : "false", k.bvh ? "true" : "false",
                  k.cull ? "true" : "false", k.edges ? "true" : "false", (k.order || ctx->oriented) ? "true" : "false", k.feedback ? "true" : "false");
    return RM_OK;
}

rm_status rm_launch_stats(rm_ctx *ctx, uint32_t *workgroups, uint32_t *tail_patches) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_launch_stats: NULL ctx");
    if (workgroups) *workgroups = ctx->last_launch_grid;
    if (tail_patches) *tail_patches = ctx->last_launch_tail;
    return RM_OK;
}

static rm_status rm_tile_stats_impl(rm_ctx *ctx, void *hip_stream, uint32_t *tiles, uint32_t *tiles_listed) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_tile_stats: NULL ctx");
    RM_HIP(ctx, hipSetDevice(ctx->device));
    RM_HIP(ctx, hipDeviceSynchronize());
    const uint32_t n = ctx->last_launch_tiles;
    uint32_t listed = n;
    for (const rm_tile_lists &t : ctx->tile_lists)
        if (t.stream == (hip_stream ? (hipStream_t)hip_stream : ctx->last_launch_stream) && t.block && ctx->last_launch_classified && n <= t.cap) {
            std::vector<unsigned long long> m(n);
            RM_HIP(ctx, hipMemcpy(m.data(), t.mask(), (size_t)n * 8u, hipMemcpyDeviceToHost));
            listed = 0;
            uint32_t hist[64] = {};
            uint64_t bits = 0;
            for (unsigned long long v : m) {
                if (t.s.tagged) v &= 0x00FFFFFFFFFFFFFFull;            // (classified at the head of the launch: the top byte is its tag)
                listed += v != 0ull;
                for (int b = 0; b < 64 && v != ~0ull; b++)
                    if (v >> b & 1ull) { hist[b]++; bits++; }
            }
            if (std::getenv("RM_DEBUG_CLASSIFY")) {
                std::fprintf(stderr, "[rm_classify] %u of %u tiles have something to hit, %.2f primitives each; tiles per pid:", listed, n,
                             listed ? (double)bits / listed : 0.);
                for (int b = 0; b < 64; b++)
                    if (hist[b]) std::fprintf(stderr, " %d:%u", b, hist[b]);
                std::fprintf(stderr, "\n");
            }
        }
    if (tiles) *tiles = n;
    if (tiles_listed) *tiles_listed = listed;
    return RM_OK;
}

rm_status rm_tile_stats(rm_ctx *ctx, void *hip_stream, uint32_t *tiles, uint32_t *tiles_listed) {
    return guarded(ctx, "rm_tile_stats", [&]() { return rm_tile_stats_impl(ctx, hip_stream, tiles, tiles_listed); });
}

rm_status rm_device_framebuffer(rm_ctx *ctx, void **device_rgb, size_t *bytes) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_device_framebuffer: NULL ctx");
    if (!ctx->d_frame) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "rm_device_framebuffer: nothing rendered yet");
    if (device_rgb) *device_rgb = ctx->d_frame;
    if (bytes) *bytes = ctx->frame_bytes;
    return RM_OK;
}

static rm_status rm_postprocess_impl(rm_ctx *ctx, void *device_rgb, uint32_t w, uint32_t h, int normalize, uint8_t *host_rgb8,
                         double *max_out) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_postprocess: NULL ctx");
    RM_HIP(ctx, hipSetDevice(ctx->device));
    double *v = (double *)device_rgb;
    if (!v) {
        if (!ctx->d_frame) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "rm_postprocess: nothing rendered yet");
        if (w != ctx->frame_w || h != ctx->frame_h)
            return ctx_fail(ctx, RM_ERR_INVALID_ARG, "rm_postprocess: size differs from the rendered frame");
        v = ctx->d_frame;
    }
    const size_t n = (size_t)w * h * 3u;
    if (n == 0) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "rm_postprocess: empty frame");
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 2048);
    RM_HIP(ctx, hipMemsetAsync(ctx->d_max, 0, sizeof(unsigned long long), ctx->stream));
    if (normalize) {
        hipLaunchKernelGGL(rm_max_kernel, dim3(blocks), dim3(256), 0, ctx->stream, v, n, ctx->d_max);
        RM_HIP(ctx, hipGetLastError());
    }
    uint8_t *d8 = nullptr;
    if (host_rgb8) {
        if (ctx->rgb8_bytes < n) {
            RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (ctx->d_rgb8) RM_HIP(ctx, hipFree(ctx->d_rgb8));
            ctx->d_rgb8 = nullptr;
            ctx->rgb8_bytes = 0;
            RM_HIP(ctx, hipMalloc(&ctx->d_rgb8, n));
            ctx->rgb8_bytes = n;
        }
        d8 = ctx->d_rgb8;
    }
    if (normalize || d8) {
        hipLaunchKernelGGL(rm_scale_quantize_kernel, dim3(blocks), dim3(256), 0, ctx->stream, v, n, ctx->d_max,
                           normalize ? 1 : 0, d8);
        RM_HIP(ctx, hipGetLastError());
    }
    RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (host_rgb8) RM_HIP(ctx, hipMemcpy(host_rgb8, d8, n, hipMemcpyDeviceToHost));
    if (max_out) {
        unsigned long long bits = 0;
        RM_HIP(ctx, hipMemcpy(&bits, ctx->d_max, sizeof bits, hipMemcpyDeviceToHost));
        std::memcpy(max_out, &bits, sizeof bits);
    }
    return RM_OK;
}

rm_status rm_postprocess(rm_ctx *ctx, void *device_rgb, uint32_t w, uint32_t h, int normalize, uint8_t *host_rgb8,
                         double *max_out) {
    return guarded(ctx, "rm_postprocess", [&]() { return rm_postprocess_impl(ctx, device_rgb, w, h, normalize, host_rgb8, max_out); });
}

}  // extern "C"

#include "rm_exchange.inc"
#include "rm_hostio.inc"
#include "rm_query_host.inc"
#include "rm_shade_host.inc"
#include "rm_radiance_host.inc"
#include "rm_refine_host.inc"
#include "rm_lens_host.inc"
#include "rm_accum_host.inc"
#include "rm_soft_host.inc"
#include "rm_motion_host.inc"
#include "rm_motion_shapes_host.inc"
#include "rm_converge_host.inc"
#include "rm_converge_motion_host.inc"
#include "rm_converge_moving_host.inc"
#include "rm_swept_host.inc"
#include "rm_camera_host.inc"
#include "rm_camera_swept_host.inc"
#include "rm_denoise_host.inc"
#include "rm_reproject_host.inc"
#include "rm_bounce_host.inc"
