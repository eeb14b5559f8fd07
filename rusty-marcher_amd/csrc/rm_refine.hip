// rm_refine.hip -- adaptive anti-aliasing of a rendered frame (include/rusty_marcher_amd.h, "adaptive anti-aliasing").
//
// Two launches behind a render, nothing in between goes through the host:
//
//   mark     one lane per pixel of the rows the render wrote.  The lane reads its pixel and its up-to-four neighbours, forms the
//            contrast -- the largest channel difference, on the radiance as rendered -- and is listed iff that is > threshold.
//            The wave compacts its listed lanes: ballot, rank by mbcnt, ONE atomic add on the workspace's counter for the
//            wave's slots, then every listed lane stores its pixel index.  The frame is only read here, so the mask is the
//            unrefined frame's for every pixel.
//   shade    the radiance ray step (radiance_steps, rm_radiance_step.inc -- the radiance kernels' own, not a copy) over the
//            listed pixels, n x n samples each.  A wave takes groups of P = 64 / (n n) listed pixels; lane l < P n n casts
//            sample l % (n n) of the group's pixel l / (n n), so the samples of a pixel sit in neighbouring lanes and walk the
//            scene together.  The other lanes, and lanes past the list's end, have their `on` off from the start, as the
//            radiance kernel's tail lanes.  After the ray steps every lane puts its answer into LDS (64 x 24 B); the lane of
//            sample 0 adds its pixel's n n entries in the order j outer, i inner, divides once and stores the pixel.  No
//            sample ever reaches global memory.
//            The list's length is known on the device only, so the grid is the host's guess (what the device holds at once,
//            at most what a full list needs) and a wave loops over the groups g = wave, wave + waves, ... while g P < count.
//
// Strict flavour, scene in global memory, occluder masks off: a sample is what rm_radiance_samples returns for its position.
#define RM_KERNEL_FAST 0
#include "rm_render_kernel.hpp"
#include "rm_refine.hpp"

using namespace rmdev;
using namespace rmdev_strict;

#include "rm_radiance_step.inc"

namespace rmrefine {

using namespace rmradiance;

// max(c, |a - b| over the channels); a NaN makes its comparison false
__device__ __forceinline__ double contrast_with(double c, const double *a, const double *b) {
    for (int k = 0; k < 3; k++) {
        const double d = __builtin_fabs(a[k] - b[k]);
        c = d > c ? d : c;
    }
    return c;
}

__global__ __launch_bounds__(RM_REFINE_MARK_LANES) void rm_refine_mark(RefineArgs q) {
    const uint32_t total = q.rows * q.frame_width;                       // (below 2^31: the frame itself is 24 bytes a pixel)
    const uint32_t idx = blockIdx.x * (uint32_t)RM_REFINE_MARK_LANES + threadIdx.x;
    const bool in = idx < total;                                         // (no early return: the wave votes below)
    bool listed = false;
    if (in) {
        const uint32_t x = idx % q.frame_width, y = idx / q.frame_width;
        const double *f = q.frame + (size_t)idx * 3u;
        const size_t row = (size_t)q.frame_width * 3u;
        double c = 0.;                                                   // a pixel without a neighbour: contrast 0
        if (x > 0u) c = contrast_with(c, f, f - 3);
        if (x + 1u < q.frame_width) c = contrast_with(c, f, f + 3);
        if (y > 0u) c = contrast_with(c, f, f - row);
        if (y + 1u < q.rows) c = contrast_with(c, f, f + row);           // row `rows - 1` never looks at row `rows`
        listed = c > q.threshold;
        if (q.mask) q.mask[idx] = listed ? 1 : 0;
    }
    const unsigned long long m = __ballot(listed);
    if (m == 0ull) return;                                               // wave-uniform
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    uint32_t base = 0u;
    if ((threadIdx.x & 63u) == 0u) base = atomicAdd(q.ws, (uint32_t)__popcll(m));
    base = uniform_u32(base);                                            // lane 0's
    // (the counter starts at zero and every pixel is listed once, so the bound cannot bite: it keeps the store in the list)
    if (listed && base + rank < total) q.ws[1u + base + rank] = idx;
}

template <bool BVH, int POW, int STACK>
__global__ __launch_bounds__(64) void rm_refine_shade_t(const double *__restrict__ scene_blob, RefineArgs q) {
    __shared__ uint32_t bstack[64];
    __shared__ double sums[64 * 3];
    const SceneView sc = global_scene_view(scene_blob, q.H, bstack);

    const uint32_t total = q.rows * q.frame_width;
    const uint32_t count = min(uniform_u32(q.ws[0]), total);             // clamped: a damaged workspace lists nothing outside the frame
    const uint32_t nn = q.n * q.n, P = 64u / nn;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t slot = lane / nn, s = lane % nn;                      // the lane's pixel within the group, its sample
    const double si = (double)(s % q.n) / (double)q.n, sj = (double)(s / q.n) / (double)q.n;   // i / n, j / n: one rounding each
    const V3 bg = mk(q.bg_x, q.bg_y, q.bg_z);
    const V3 cam = mk(q.cam_x, q.cam_y, q.cam_z);

    for (uint32_t g = blockIdx.x; (unsigned long long)g * P < count; g += gridDim.x) {
        const uint32_t k = g * P + slot;                                 // (g P < count <= 2^31)
        bool on = (slot < P) & (k < count);
        uint32_t pix = on ? q.ws[1u + k] : 0u;
        on = on & (pix < total);                                         // (a damaged list, again)
        pix = on ? pix : 0u;
        V3 orig = mk(0., 0., 0.), dir = mk(0., 0., -1.);                 // (a lane without a sample holds a harmless ray it never casts)
        if (on) {
            const double sx = (double)(pix % q.frame_width) + si, sy = (double)(pix / q.frame_width) + sj;
            dir = normalized(sample_direction(q, q.oriented != 0u, sx, sy));
            orig = cam;
        }
        // renderer.rs:262-264 at n_recursion = 1: no ray is cast under a cap of 0 (wave-uniform)
        const V3 acc = q.max_depth == 0u ? bg : radiance_steps<BVH, POW, STACK>(sc, orig, dir, on, bg, q.max_depth);
        sums[lane * 3u] = acc.x; sums[lane * 3u + 1u] = acc.y; sums[lane * 3u + 2u] = acc.z;
        __syncthreads();
        if (on & (s == 0u)) {
            double rx = sums[lane * 3u], ry = sums[lane * 3u + 1u], rz = sums[lane * 3u + 2u];
            for (uint32_t t = 1u; t < nn; t++) {                         // sample t = j n + i: j outer, i inner
                rx = rx + sums[(lane + t) * 3u]; ry = ry + sums[(lane + t) * 3u + 1u]; rz = rz + sums[(lane + t) * 3u + 2u];
            }
            const double div = (double)nn;
            double *out = q.frame + (size_t)pix * 3u;
            out[0] = rx / div; out[1] = ry / div; out[2] = rz / div;
        }
        __syncthreads();                                                 // the next group's answers overwrite `sums`
    }
}

}  // namespace rmrefine

using namespace rmrefine;

const void *rm_refine_mark_kernel() { return (const void *)rm_refine_mark; }

const void *rm_refine_shade_kernel(bool bvh, int pow_mode, int stack) {
    RM_SHADING_TABLE(RM_SHADING_KERNEL, rm_refine_shade_t)
    return nullptr;
}
