// rm_accum.hip -- progressive frames: lens samples added to a running per-pixel sum (include/rusty_marcher_amd.h,
// "progressive frames").
//
// The launch is the thin-lens camera's (rm_lens.hip) in everything but its last step: the same groups of P = 64 / n_samples
// pixels, lane l casting table row l % n_samples of pixel l / n_samples, idle lanes off from the start, the same lens ray,
// the same ray step (radiance_steps, rm_radiance_step.inc -- not a copy), the same 64 x 24 B of LDS, the same grid-stride loop
// over the groups and no early return in front of a vote or barrier.
//
//   resolve  the lane of row 0 continues the pixel's sum instead of starting one: S is the 24 B of `sum` where n_before > 0
//            (wave-uniform, a kernel argument), else the first sample itself -- never 0. + sample, which would turn a -0 into
//            +0 and is not what the lens kernel does.  The other entries are added in table order, S goes back to `sum`,
//            S / (double)(n_before + n_samples) to `mean` and its display bytes -- to_vec, (uint8_t)(255. * fmin(fmax(m, 0.),
//            1.)) -- to `rgb8`, the last two where given (wave-uniform).  With n_before == 0 the mean is the lens frame, byte
//            for byte; passes over consecutive slices of one table are one lens launch's left fold.
//
// The bytes leave as three byte stores a pixel from the lane that holds the mean: see DESIGN.md section 6h for the
// resource-usage lines that decided it.
//
// Strict flavour, scene in global memory, occluder masks off, contraction off: as rm_lens.hip.  The body is
// rm_accum_body.inc's, shared with the area lights' kernel (rm_soft.hip); here every light stands where the scene image says.
#define RM_KERNEL_FAST 0
#include "rm_render_kernel.hpp"
#include "rm_accum.hpp"

using namespace rmdev;
using namespace rmdev_strict;

#include "rm_radiance_step.inc"

#include "rm_accum_body.inc"

namespace rmaccum {

template <bool BVH, int POW, int STACK>
__global__ __launch_bounds__(64) void rm_accum_shade_t(const double *__restrict__ scene_blob, AccumArgs a) {
    __shared__ uint32_t bstack[64];
    __shared__ double sums[64 * 3];
    accum_shade<BVH, POW, STACK>(scene_blob, a, bstack, sums, [](uint32_t) { return StoredLights(); });
}

}  // namespace rmaccum

using namespace rmaccum;

const void *rm_accum_kernel(bool bvh, int pow_mode, int stack) {
    RM_SHADING_TABLE(RM_SHADING_KERNEL, rm_accum_shade_t)
    return nullptr;
}
