// rm_bounce.hip -- diffuse bounce: progressive frames whose samples each add one bounce of indirect light behind the camera ray's
// first hit (include/rusty_marcher_amd.h, "diffuse bounce").
//
// The launch is rm_soft.hip's in everything -- groups, lens rays, moved lights, LDS, fold, mean and bytes are rm_accum_body.inc's,
// not a copy -- but one rule in the ray step (rm_radiance_step.inc, behind RM_BOUNCE_ROWS, which this unit and
// rm_converge_bounce.hip alone define): a lane whose camera ray first hits a surface that is not glass has no children, so
// behind that step it turns into the bounce ray -- weight strength x diffusion x k, depth 2 --, leaves what it has summed (A) and
// the hit's diffuse colour (tint) in six doubles of LDS of its own, sums the bounce's subtree from zero and answers
// A + tint x sum.  Held in registers the six values would be alive across every walk of the subtree; in LDS they cost the
// walk nothing (3 KiB a workgroup, far from what bounds the occupancy).  radiance_steps keeps its scalar weight and its stack:
// the rays such a lane parks have depths 3 .. max_depth, within the max_depth - 1 entries rm_plan.cpp sizes the stack for.
//
// The lane's row of the bounce table is fetched in the step that bounces, from the row index and the pixel the lane carries
// (two words), not in front of the walk: rm_camera.hip's lesson.  Every lane holds a valid row (s < n_samples, idle lanes
// too).  Nothing read from the table and nothing of the hash forms an address: a non-finite entry is a non-finite colour.
//
// strength == 0 is wave-uniform: the step never enters the rule and no lane parks anything, so every operation on a value
// is rm_soft.hip's and the frame is its frame byte for byte.
//
// Strict flavour, scene in global memory, occluder masks off, contraction off: as rm_soft.hip.
#define RM_KERNEL_FAST 0
#define RM_BOUNCE_ROWS 1
#include "rm_render_kernel.hpp"
#include "rm_bounce.hpp"

using namespace rmdev;
using namespace rmdev_strict;

#include "rm_radiance_step.inc"
#include "rm_accum_body.inc"

namespace rmbounce {

using namespace rmaccum;

template <bool BVH, int POW, int STACK>
__global__ __launch_bounds__(64) void rm_bounce_shade_t(const double *__restrict__ scene_blob, BounceArgs a) {
    __shared__ uint32_t bstack[64];
    __shared__ double sums[64 * 3];
    __shared__ double park[64 * 6];                                      // a bounce lane's first-hit sum and tint (radiance_steps)
    const double *offsets = a.S.offsets;
    const uint32_t words = 3u * a.S.A.L.H.n_lights;                      // (s words < 64 x 3 x n_lights: inside the table)
    accum_shade<BVH, POW, STACK>(scene_blob, a.S.A, bstack, sums, a.bounce, a.strength, park,   // (2 s + 1 < 2 n_samples: inside the table)
                                 [=](uint32_t s) { return OffsetLights{offsets + (size_t)s * words}; });
}

}  // namespace rmbounce

using namespace rmbounce;

const void *rm_bounce_kernel(bool bvh, int pow_mode, int stack) {
    RM_SHADING_TABLE(RM_SHADING_KERNEL, rm_bounce_shade_t)
    return nullptr;
}
