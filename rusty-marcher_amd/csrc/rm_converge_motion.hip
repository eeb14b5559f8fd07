// rm_converge_motion.hip -- converging frames with moving spheres: the pixels still noisy alone are sampled, and each sample sees
// the spheres at positions of its own (include/rusty_marcher_amd.h, "converging frames with moving spheres").
//
// A pass is rm_converge.hip's in everything -- the select launch is that unit's kernel, unchanged, and the shade body (list,
// groups, per-pixel rows, lens rays, ray step, moved lights, LDS, fold, stats, count, mean and bytes) is rm_converge_body.inc's,
// not a copy -- with rm_motion.hip's one more rule: where a sphere stands.  The lane that casts sample s of a listed pixel with
// count n holds table row r = n + s, and for that lane the sphere that is shape k of the scene stands at
// C_k + shape_offsets[r][k], one addition a component, at every step of its ray: in the closest-hit walk, in both shadow walks
// and in the normal of a hit (OffsetSpheres::at, rm_trace.inc, is the one place the addition stands).  The table is in shape
// order and read through the queries' pid map, as in rm_motion.hip.
//
// The family is the motion family's: flat walk only (BVH = false whatever the scene image holds; a scene with a hierarchy is
// walked flat through the permuted device order), always OffsetLights + OffsetSpheres, POW x STACK in {4, 32}.  What is keyed on
// a sphere's position, and why none of it is in these kernels, is rm_motion.hip's audit: the same radiance_steps with the same
// arguments stands here.
//
// Bounds.  The three tables hold table_rows rows each (the host's precondition, and what the tick keeps resident).
//   - every lane's r is < table_rows, idle lanes included: a listed pixel has count + n_samples <= max_samples <= table_rows, the
//     count as read is held to last_first = table_rows - n_samples (the body's clamp min(count, last_first)), and a lane without
//     a sample takes n = 0, r = s < n_samples <= table_rows.  So r shape_words + 3 k + 2 < table_rows x n_shapes x 3 for k < n_shapes.
//   - every device sphere's map word is a shape of the scene, k < n_shapes: the host checked the count against the resident
//     scene's, whose image the map was built from.
//   - a scene without spheres takes a NULL table and never fetches: OffsetSpheres is asked for spheres the walks visit and for
//     sphere 0 in surface_at, and the latter only where some lane has a sphere hit.
//   - a non-finite offset is a non-finite colour, never an address: offsets are added to centres and nothing else.
//
// Strict flavour, scene in global memory, occluder masks off, contraction off: as rm_converge.hip.
#define RM_KERNEL_FAST 0
#include "rm_render_kernel.hpp"
#include "rm_converge_motion.hpp"

using namespace rmdev;
using namespace rmdev_strict;

#include "rm_radiance_step.inc"

namespace rmconvergemotion {

using namespace rmradiance;

template <int POW, int STACK>
__global__ __launch_bounds__(64) void rm_converge_motion_shade_t(const double *__restrict__ scene_blob, ConvergeMotionArgs m) {
    __shared__ uint32_t bstack[64];
    __shared__ double sums[64 * 3];
    constexpr bool BVH = false;                                          // the family walks flat
    const ConvergeArgs &a = m.C;
    const uint32_t words = 3u * a.L.H.n_lights;                          // (r words < table_rows x 3 x n_lights: inside the table)
    const uint32_t shape_words = 3u * m.n_shapes;                        // (r shape_words < table_rows x 3 x n_shapes: inside the table)
    const auto lights_of = [&](uint32_t r) { return OffsetLights{a.offsets + (size_t)r * words}; };
    const auto spheres_of = [&](uint32_t r) { return OffsetSpheres{m.shape_offsets + (size_t)r * shape_words, m.pid_map}; };
#include "rm_converge_body.inc"
}

}  // namespace rmconvergemotion

using namespace rmconvergemotion;

const void *rm_converge_motion_kernel(bool bvh, int pow_mode, int stack) {
    (void)bvh;                                                           // the family walks flat
    if (stack == 4)
        return pow_mode == POW_INTEGER ? (const void *)rm_converge_motion_shade_t<POW_INTEGER, 4> : (const void *)rm_converge_motion_shade_t<POW_GENERIC, 4>;
    if (stack == 32)
        return pow_mode == POW_INTEGER ? (const void *)rm_converge_motion_shade_t<POW_INTEGER, 32> : (const void *)rm_converge_motion_shade_t<POW_GENERIC, 32>;
    return nullptr;
}
