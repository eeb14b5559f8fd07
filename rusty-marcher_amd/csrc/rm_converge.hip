// rm_converge.hip -- converging frames: progressive frames that sample only the pixels still noisy
// (include/rusty_marcher_amd.h, "converging frames").
//
// Two launches a pass behind a memset of the list's length, nothing in between goes through the host:
//
//   select   one lane per pixel of [0, rows).  The lane reads its pixel's count and (Y, Q) and those of its up-to-four
//            neighbours, decides `noisy` for each of the five by the header's rule -- plain operations, each rounded once -- and
//            is listed iff it is not capped and one of the five is noisy.  The wave compacts its listed lanes as
//            rm_refine_mark does: ballot, rank by mbcnt, ONE atomic add on the list's length, then every listed lane stores
//            its pixel index.  Nothing is written here but the list and the mask, so the rule is complete before any pixel
//            is sampled.
//   shade    rm_accum_body.inc's pass over the LISTED pixels.  A wave takes groups of P = 64 / n_samples list entries; lane
//            l < P n_samples casts sample l % n_samples of the group's pixel l / n_samples -- and that sample is table row
//            count[pixel] + l % n_samples: every pixel continues the sequence where it stopped.  So the table row, the
//            sub-pixel offset, the lens point and the row of light offsets are the lane's per group, inside the loop, where
//            rm_accum_body.inc has them in front of it.  The fold lane adds the pixel's samples to the sum in table order,
//            forms y = (r + g) + b of each and adds y and y y to (Y, Q) in the same order, stores the three and the new count,
//            the mean and the bytes.
//            Every lane reads the list's length once, before the loop: the trip count and the barriers inside are the
//            workgroup's.  The grid is the host's (what the device holds at once, at most what a list of every pixel needs);
//            workgroups beyond the list's end leave at once.
//
// A row is always inside the table: the select kernel lists a pixel only with count + n_samples <= max_samples, whatever the
// count buffer holds, max_samples <= table_rows is the host's check (the tick hands over the rows resident, which cover
// min(N + n_samples, max_samples) with N a bound on every count), and a lane without a sample takes row s < n_samples.  So
// neither fetch needs a predicate.  Three clamps stand on top of that, against one thing only: the workspace or the count buffer
// being written by someone else between the select launch and the shade launch (another stream, a stray store) -- the list's
// length is held to the frame's pixels, an entry that is no pixel of the frame is dropped, and the count as read is held to
// table_rows - n_samples.  With buffers that only these two launches write none of them changes a value; with damaged ones the
// pixels are unspecified and no address leaves the buffers.
//
// The shade body is rm_converge_body.inc's, which rm_converge_motion.hip shares (spheres moved as well).  It is text of its own,
// not rm_accum_body.inc generalised: there the row, the lens point and the lights are hoisted out of the loop over the groups
// and the divisor is the launch's, and making those per pixel in that body would change the kernels of rm_accum.hip and
// rm_soft.hip (profiles/converge_resource_usage.txt has all three side by side).
//
// Strict flavour, scene in global memory, occluder masks off, contraction off: as rm_accum.hip.
#define RM_KERNEL_FAST 0
#include "rm_render_kernel.hpp"
#include "rm_converge.hpp"

using namespace rmdev;
using namespace rmdev_strict;

#include "rm_radiance_step.inc"

namespace rmconverge {

using namespace rmradiance;

// The pixel's count as the pass sees it
__device__ __forceinline__ uint32_t count_of(const ConvergeArgs &a, uint32_t pix) { return a.fresh ? 0u : a.count[pix]; }

// noisy(p) = !capped(p) && unsettled(p), the header's rule word for word; nothing of the buffers is read where fresh
__device__ __forceinline__ bool noisy_at(const ConvergeArgs &a, uint32_t pix) {
    const uint32_t n = count_of(a, pix);
    if ((unsigned long long)n + a.L.n_samples > a.max_samples) return false;   // capped
    if (a.tolerance < 0.) return true;
    if (n < max(a.min_samples, 2u)) return true;
    const double Y = a.stats[(size_t)pix * 2u], Q = a.stats[(size_t)pix * 2u + 1u];
    const double nd = (double)n;
    const double m2 = Q - (Y * Y) / nd;
    return !(m2 <= (a.tolerance * a.tolerance) * (nd * (nd - 1.)));      // a NaN: unsettled
}

__global__ __launch_bounds__(RM_CONVERGE_SELECT_LANES) void rm_converge_select(ConvergeArgs a) {
    const LensArgs &q = a.L;
    const uint32_t total = q.rows * q.frame_width;                       // (below 2^31: the host checked)
    const uint32_t idx = blockIdx.x * (uint32_t)RM_CONVERGE_SELECT_LANES + threadIdx.x;
    const bool in = idx < total;                                         // (no early return: the wave votes below)
    bool listed = false;
    if (in) {
        const uint32_t x = idx % q.frame_width, y = idx / q.frame_width;
        const bool capped = (unsigned long long)count_of(a, idx) + q.n_samples > a.max_samples;
        bool any = noisy_at(a, idx);
        if (x > 0u) any = any | noisy_at(a, idx - 1u);
        if (x + 1u < q.frame_width) any = any | noisy_at(a, idx + 1u);
        if (y > 0u) any = any | noisy_at(a, idx - q.frame_width);
        if (y + 1u < q.rows) any = any | noisy_at(a, idx + q.frame_width);   // row `rows - 1` never looks at row `rows`
        listed = !capped & any;
        if (a.mask) a.mask[idx] = listed ? 1 : 0;
    }
    const unsigned long long m = __ballot(listed);
    if (m == 0ull) return;                                               // wave-uniform
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    uint32_t base = 0u;
    if ((threadIdx.x & 63u) == 0u) base = atomicAdd(a.ws, (uint32_t)__popcll(m));
    base = uniform_u32(base);                                            // lane 0's
    // (the length starts at zero and every pixel is listed once, so the bound cannot bite: it keeps the store in the list)
    if (listed && base + rank < total) a.ws[1u + base + rank] = idx;
}

template <bool BVH, int POW, int STACK, bool OFFSET>
__global__ __launch_bounds__(64) void rm_converge_shade_t(const double *__restrict__ scene_blob, ConvergeArgs a) {
    __shared__ uint32_t bstack[64];
    __shared__ double sums[64 * 3];
    const uint32_t words = 3u * a.L.H.n_lights;                          // (r words < table_rows x 3 x n_lights: inside the table)
    const auto lights_of = [&](uint32_t r) {
        if constexpr (OFFSET) return OffsetLights{a.offsets + (size_t)r * words};
        else return StoredLights();
    };
    const auto spheres_of = [](uint32_t) { return StoredSpheres(); };
#include "rm_converge_body.inc"
}

}  // namespace rmconverge

using namespace rmconverge;

const void *rm_converge_select_kernel() { return (const void *)rm_converge_select; }

const void *rm_converge_shade_kernel(bool bvh, int pow_mode, int stack, bool offset) {
#define RM_CONVERGE_KERNEL(K, B, S) (offset ? RM_SHADING_KERNEL(K, B, S, true) : RM_SHADING_KERNEL(K, B, S, false))
    RM_SHADING_TABLE(RM_CONVERGE_KERNEL, rm_converge_shade_t)
#undef RM_CONVERGE_KERNEL
    return nullptr;
}
