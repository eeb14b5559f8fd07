// rm_converge_bounce.hip -- converging frames with a diffuse bounce (include/rusty_marcher_amd.h, "diffuse bounce").
//
// The select kernel is rm_converge.hip's, unchanged and not compiled here; the shade body is rm_converge_body.inc's with the
// bounce rule of the ray step behind RM_BOUNCE_ROWS (rm_radiance_step.inc; rm_bounce.hip, the head of the file, has the rule's
// shape and the stack's bound).  The lane's bounce row is its table row r = count[pixel] + sample, which rm_converge.hip's
// argument keeps inside the table in every lane: the host demands table_rows rows of the bounce table as of the lens table.
//
// strength == 0 is wave-uniform and leaves rm_converge.hip's bytes: sum, stats, count, list, mean and display bytes.
//
// Strict flavour, scene in global memory, occluder masks off, contraction off: as rm_converge.hip.
#define RM_KERNEL_FAST 0
#define RM_BOUNCE_ROWS 1
#include "rm_render_kernel.hpp"
#include "rm_bounce.hpp"

using namespace rmdev;
using namespace rmdev_strict;

#include "rm_radiance_step.inc"

namespace rmconvergebounce {

using namespace rmradiance;

template <bool BVH, int POW, int STACK, bool OFFSET>
__global__ __launch_bounds__(64) void rm_converge_bounce_shade_t(const double *__restrict__ scene_blob, ConvergeBounceArgs b) {
    __shared__ uint32_t bstack[64];
    __shared__ double sums[64 * 3];
    __shared__ double bounce_park[64 * 6];                               // a bounce lane's first-hit sum and tint (radiance_steps)
    const ConvergeArgs &a = b.C;
    const double *bounce_table = b.bounce;                               // (2 r + 1 < 2 table_rows: inside the table)
    const double bounce_strength = b.strength;
    const uint32_t words = 3u * a.L.H.n_lights;                          // (r words < table_rows x 3 x n_lights: inside the table)
    const auto lights_of = [&](uint32_t r) {
        if constexpr (OFFSET) return OffsetLights{a.offsets + (size_t)r * words};
        else return StoredLights();
    };
    const auto spheres_of = [](uint32_t) { return StoredSpheres(); };
#include "rm_converge_body.inc"
}

}  // namespace rmconvergebounce

using namespace rmconvergebounce;

const void *rm_converge_bounce_kernel(bool bvh, int pow_mode, int stack, bool offset) {
#define RM_CONVERGE_BOUNCE_KERNEL(K, B, S) (offset ? RM_SHADING_KERNEL(K, B, S, true) : RM_SHADING_KERNEL(K, B, S, false))
    RM_SHADING_TABLE(RM_CONVERGE_BOUNCE_KERNEL, rm_converge_bounce_shade_t)
#undef RM_CONVERGE_BOUNCE_KERNEL
    return nullptr;
}
