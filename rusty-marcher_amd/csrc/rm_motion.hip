// rm_motion.hip -- moving spheres: progressive frames whose samples each see the spheres at positions of their own, so that the
// mean is blurred along their motion (include/rusty_marcher_amd.h, "moving spheres").
//
// The launch is rm_soft.hip's in everything -- groups, lens rays, ray step, moved lights, LDS, fold, mean and bytes are
// rm_accum_body.inc's, not a copy -- but one more rule: where a sphere stands.  Lane l casts table row s = l % n_samples, and
// for that lane the sphere that is shape k of the scene stands at C_k + shape_offsets[s][k], one addition a component, at every
// step of its ray: in the closest-hit walk, in both shadow walks and in the normal of a hit (radiance_steps hands the rule to
// closest_hit, surface_at and shade_direct, rm_trace.inc; OffsetSpheres::at is the one place the addition stands, so the normal
// sees the centre the hit test saw).
//
// The table is in shape order, the device's spheres need not be (a scene with a sphere hierarchy is permuted at upload): the
// queries' pid map, word 0 of device sphere i, names the shape.  In the walks i is wave-uniform and so are the record and the
// map word (scalar loads, as before); the row is the lane's, so the three offsets are per-lane loads and the centre, a scalar
// operand of the plain kernels, becomes three VGPR pairs a sphere of the batch of four.  A wave reads at most 64 distinct rows,
// again and again: they stay in the vector L1.  See DESIGN.md section 6n for the resource-usage lines beside rm_soft.hip's.
//
// What is keyed on a sphere's position, and why none of it is in these kernels -- the audit:
//   - the hierarchy over the spheres (boxes about the uploaded centres): the family is instantiated with BVH = false alone,
//     whatever the scene image holds, and the flat walk visits every primitive of any scene (as RM_DISABLE_BVH=1 does).  The
//     triangles' hierarchy goes with it: one template argument decides both.  Such scenes pay the flat walk.
//   - the bundle cull (bounds, planar records, groups) and the shadow rays' rho: CULL = false in radiance_steps.
//   - the occluder masks: the host's header says there are none (shading_header), and shade_direct does not look where the
//     rule moves spheres.
//   - the classified tiles' primary masks: radiance_steps passes have_mask = false.
//   - the glass words' dead sides: the render kernel's, radiance_steps does not read them.
//   - ties between equal distances: decided by the list key of a pid (closer, prim_key), not by a position.
//   - closest_hit, any_hit and any_hit2 refuse at compile time to walk a hierarchy or cull with a rule that moves spheres.
// Polygon and triangle records are not moved here: rm_motion_shapes.hip moves them, with one more rule.
//
// Every lane holds a valid row (s < n_samples, idle lanes too) and every device sphere's map word is a shape of the scene
// (< n_shapes, the host checked the count), so the fetch needs no predicate; surface_at asks for sphere 0 in lanes without a
// sphere hit, and only where some lane has one: then sphere 0 exists.  A scene without spheres never fetches.  A non-finite
// offset is a non-finite colour, never an address.
//
// Strict flavour, scene in global memory, occluder masks off, contraction off: as rm_accum.hip.
#define RM_KERNEL_FAST 0
#include "rm_render_kernel.hpp"
#include "rm_motion.hpp"

using namespace rmdev;
using namespace rmdev_strict;

#include "rm_radiance_step.inc"
#include "rm_accum_body.inc"

namespace rmmotion {

using namespace rmaccum;

template <int POW, int STACK>
__global__ __launch_bounds__(64) void rm_motion_shade_t(const double *__restrict__ scene_blob, MotionArgs a) {
    __shared__ uint32_t bstack[64];
    __shared__ double sums[64 * 3];
    const double *offsets = a.S.offsets;
    const uint32_t words = 3u * a.S.A.L.H.n_lights;                      // (s words < 64 x 3 x n_lights: inside the table)
    const double *shape_offsets = a.shape_offsets;
    const uint32_t *pid_map = a.pid_map;
    const uint32_t shape_words = 3u * a.n_shapes;                        // (s shape_words < 64 x 3 x n_shapes: inside the table)
    accum_shade<false, POW, STACK>(
        scene_blob, a.S.A, bstack, sums, [=](uint32_t s) { return OffsetLights{offsets + (size_t)s * words}; },
        [=](uint32_t s) { return OffsetSpheres{shape_offsets + (size_t)s * shape_words, pid_map}; });
}

}  // namespace rmmotion

using namespace rmmotion;

const void *rm_motion_kernel(bool bvh, int pow_mode, int stack) {
    (void)bvh;                                                           // the family walks flat
    if (stack == 4) return pow_mode == POW_INTEGER ? (const void *)rm_motion_shade_t<POW_INTEGER, 4> : (const void *)rm_motion_shade_t<POW_GENERIC, 4>;
    if (stack == 32) return pow_mode == POW_INTEGER ? (const void *)rm_motion_shade_t<POW_INTEGER, 32> : (const void *)rm_motion_shade_t<POW_GENERIC, 32>;
    return nullptr;
}
