// rm_soft.hip -- area lights: progressive frames whose samples each see the lights at positions of their own
// (include/rusty_marcher_amd.h, "area lights").
//
// The launch is rm_accum.hip's in everything -- groups, lens rays, ray step, LDS, fold, mean and bytes are rm_accum_body.inc's,
// not a copy -- but one rule: where a light stands.  Lane l casts table row s = l % n_samples, and for that lane light i stands
// at P_i + offsets[s][i], one addition a component, at every step of its ray: the primary hit and the children alike
// (radiance_steps hands the rule to shade_direct, rm_trace.inc).  With occluder masks off and CULL = false nothing else in
// these kernels is keyed on a light's position, and the pair walk decides per lane whether two lights share an origin side.
//
// The lane's offsets are fetched where a light is shaded (three loads beside the light's record), not held in registers: the
// number of lights is the scene's, so a lane's n_lights x 3 values would be an indexed array -- scratch -- and live across both
// shadow walks.  A wave reads at most 64 distinct rows, again and again: they stay in the vector L1.  See DESIGN.md section 6i
// for the resource-usage lines beside rm_accum.hip's.
//
// Every lane holds a valid row (s < n_samples, idle lanes too), so the fetch needs no predicate; a scene without lights never
// fetches.  A non-finite offset is a non-finite colour, never an address.
//
// Strict flavour, scene in global memory, occluder masks off, contraction off: as rm_accum.hip.
#define RM_KERNEL_FAST 0
#include "rm_render_kernel.hpp"
#include "rm_soft.hpp"

using namespace rmdev;
using namespace rmdev_strict;

#include "rm_radiance_step.inc"
#include "rm_accum_body.inc"

namespace rmsoft {

using namespace rmaccum;

template <bool BVH, int POW, int STACK>
__global__ __launch_bounds__(64) void rm_soft_shade_t(const double *__restrict__ scene_blob, SoftArgs a) {
    __shared__ uint32_t bstack[64];
    __shared__ double sums[64 * 3];
    const double *offsets = a.offsets;
    const uint32_t words = 3u * a.A.L.H.n_lights;                        // (s words < 64 x 3 x n_lights: inside the table)
    accum_shade<BVH, POW, STACK>(scene_blob, a.A, bstack, sums, [=](uint32_t s) { return OffsetLights{offsets + (size_t)s * words}; });
}

}  // namespace rmsoft

using namespace rmsoft;

const void *rm_soft_kernel(bool bvh, int pow_mode, int stack) {
    RM_SHADING_TABLE(RM_SHADING_KERNEL, rm_soft_shade_t)
    return nullptr;
}
