// rm_motion_shapes.hip -- moving shapes: progressive frames whose samples each see every shape -- sphere, polygon or mesh -- at a
// position of its own, so that the mean is blurred along their motion (include/rusty_marcher_amd.h, "moving shapes").
//
// The launch is rm_motion.hip's in everything -- groups, lens rays, ray step, moved lights, moved spheres, LDS, fold, mean and
// bytes are rm_accum_body.inc's, not a copy -- but one more rule: where a polygon or a triangle stands.  Lane l casts table row
// s = l % n_samples, and for that lane the primitive whose shape is k stands at its record + shape_offsets[s][k]: the plane
// point (the centre) and x and y of every vertex, one addition a component, the normal as stored -- polygon.rs:44-49,
// triangle.rs:19-24 and, a mesh being its triangles, obj.rs:24-29.  The hit tests then form (p + off) - orig and (v + off) - a,
// what the reference forms after offset(): contraction is off, so the pass is the reference's operation for operation, as it
// is for the spheres.  surface_at needs nothing: the point is o + d t and the normal is the record's.
//
// The records stay scalar operands.  A walk holds the lane's three offsets of the shape it is at (OffsetShapes::Planar,
// rm_radiance_step.inc) and adds them at each use; the map word of a primitive is wave-uniform, so "another shape than the last"
// is a scalar branch and the triangles of a mesh, consecutive in list order, fetch their offset once a mesh and walk (a triangle
// hierarchy permutes the device order and the map follows: where it interleaves meshes the offset is fetched more often,
// never wrongly).  See DESIGN.md section 6q for the resource-usage lines beside rm_motion.hip's.
//
// What is keyed on a primitive's position, and why none of it is in these kernels -- rm_motion.hip's audit, extended to the
// polygons and triangles:
//   - the hierarchies over the spheres and over the triangles (boxes about the uploaded centres and vertices): BVH = false
//     alone, whatever the scene image holds; the flat walk visits every primitive in device order.
//   - the bundle cull -- bounds, the planar records of the edge tests, the groups -- and the shadow rays' rho: CULL = false in
//     radiance_steps, and cull_planar is never read.
//   - the occluder masks, the floor's cell-wise ones among them: the host's header says there are none (shading_header), and
//     shade_direct does not look where the rule moves (SPHERES::moves).
//   - the classified tiles' primary masks: radiance_steps passes have_mask = false.
//   - the dead-children and glass words: the render kernels', radiance_steps does not read them.
//   - ties between equal distances: decided by the list key of a pid (closer, prim_key), not by a position.
//   - closest_hit and any_hit refuse at compile time to walk a hierarchy or cull with a rule that moves.
//
// Every lane holds a valid row (s < n_samples, idle lanes too) and every pid's map word is a shape of the scene (< n_shapes,
// the host checked the count), so no fetch needs a predicate.  A scene without shapes never fetches.  A non-finite offset is a
// non-finite colour, never an address.
//
// Strict flavour, scene in global memory, occluder masks off, contraction off: as rm_accum.hip.
#define RM_KERNEL_FAST 0
#include "rm_render_kernel.hpp"
#include "rm_motion_shapes.hpp"

using namespace rmdev;
using namespace rmdev_strict;

#include "rm_radiance_step.inc"
#include "rm_accum_body.inc"

namespace rmmotionshapes {

using namespace rmaccum;

template <int POW, int STACK>
__global__ __launch_bounds__(64) void rm_motion_shapes_shade_t(const double *__restrict__ scene_blob, MotionArgs a) {
    __shared__ uint32_t bstack[64];
    __shared__ double sums[64 * 3];
    const double *offsets = a.S.offsets;
    const uint32_t words = 3u * a.S.A.L.H.n_lights;                      // (s words < 64 x 3 x n_lights: inside the table)
    const double *shape_offsets = a.shape_offsets;
    const uint32_t *pid_map = a.pid_map;
    const uint32_t shape_words = 3u * a.n_shapes;                        // (s shape_words < 64 x 3 x n_shapes: inside the table)
    const uint32_t ns = a.S.A.L.H.n_spheres, np = a.S.A.L.H.n_polygons;
    accum_shade<false, POW, STACK>(
        scene_blob, a.S.A, bstack, sums, [=](uint32_t s) { return OffsetLights{offsets + (size_t)s * words}; },
        [=](uint32_t s) { return OffsetShapes{shape_offsets + (size_t)s * shape_words, pid_map, ns, np}; });
}

}  // namespace rmmotionshapes

using namespace rmmotionshapes;

const void *rm_motion_shapes_kernel(bool bvh, int pow_mode, int stack) {
    (void)bvh;                                                           // the family walks flat
    if (stack == 4)
        return pow_mode == POW_INTEGER ? (const void *)rm_motion_shapes_shade_t<POW_INTEGER, 4> : (const void *)rm_motion_shapes_shade_t<POW_GENERIC, 4>;
    if (stack == 32)
        return pow_mode == POW_INTEGER ? (const void *)rm_motion_shapes_shade_t<POW_INTEGER, 32> : (const void *)rm_motion_shapes_shade_t<POW_GENERIC, 32>;
    return nullptr;
}
