// rm_swept.hip -- swept hierarchies: the moving shapes' pass (rm_motion_shapes.hip) through a hierarchy whose boxes were refitted
// to every position the pass's offsets can give a primitive (include/rusty_marcher_amd.h, "swept hierarchies").
//
// The launch is rm_motion_shapes.hip's in everything -- the body is rm_accum_body.inc's, the rule OffsetShapes' additions -- but
// BVH = true, and the scene blob it is handed is a swept one (rm_swept_image.cpp): the resident image's words with the nodes at
// off_bvh_spheres and off_bvh_triangles holding boxes that contain each primitive at record + off for every off within the extents
// the swept blob was built with.  bvh_walk is unchanged and reads those nodes; closest_hit and any_hit apply the lane's rule inside
// the leaves (rm_trace.inc, `if constexpr (SPHERES::moves)`) exactly as the flat loops do, so a primitive is tested with the same
// operations in either walk and the hierarchy only decides which primitives are tested: the pass writes the flat pass's bytes.
//
// rm_motion_shapes.hip's audit of what is keyed on a primitive's position, as it stands here:
//   - the hierarchies: entered, because the boxes hold for every row within the extents (SweptShapes::swept admits the rule
//     past the static asserts).  Pruning by prune_at against best_t stays valid: a box contains every lane's moved primitive,
//     and the distance compared is the lane's own.
//   - the bundle cull: CULL = false in radiance_steps, as before.
//   - the occluder masks: the host's header says there are none, and BVH = true never looks (shade_direct).
//   - the classified tiles' primary masks: have_mask = false.
//   - ties between equal distances: decided by the list key of a pid (closer<false>), never by a position or a visiting order.
//   - polygons have no hierarchy and are walked flat.
//
// Bounds.  rm_motion_shapes.hip's: every lane holds a valid row and every pid's map word is a shape of the scene.  One more
// reader of the map: a leaf.  The leaves fetch records first + 1 .. first + 3 unconditionally (the blob is padded) but ask the
// rule -- which reads pid_map[2 pid] and through it the offset row -- only for primitives the leaf holds (cnt > j, wave-uniform),
// so no map word beyond the scene's pids is read.  A row outside the extents can make a box miss its primitive: a wrong pixel,
// never an address -- nothing read from a row or a box forms one.
//
// Strict flavour, scene in global memory, occluder masks off, contraction off: as rm_accum.hip.
#define RM_KERNEL_FAST 0
#include "rm_render_kernel.hpp"
#include "rm_swept.hpp"

using namespace rmdev;
using namespace rmdev_strict;

#include "rm_radiance_step.inc"
#include "rm_accum_body.inc"

namespace rmswept {

using namespace rmaccum;

template <int POW, int STACK>
__global__ __launch_bounds__(64) void rm_swept_shade_t(const double *__restrict__ scene_blob, MotionArgs a) {
    __shared__ uint32_t bstack[64];
    __shared__ double sums[64 * 3];
    const double *offsets = a.S.offsets;
    const uint32_t words = 3u * a.S.A.L.H.n_lights;                      // (s words < 64 x 3 x n_lights: inside the table)
    const double *shape_offsets = a.shape_offsets;
    const uint32_t *pid_map = a.pid_map;
    const uint32_t shape_words = 3u * a.n_shapes;                        // (s shape_words < 64 x 3 x n_shapes: inside the table)
    const uint32_t ns = a.S.A.L.H.n_spheres, np = a.S.A.L.H.n_polygons;
    accum_shade<true, POW, STACK>(
        scene_blob, a.S.A, bstack, sums, [=](uint32_t s) { return OffsetLights{offsets + (size_t)s * words}; },
        [=](uint32_t s) { return SweptShapes{{shape_offsets + (size_t)s * shape_words, pid_map, ns, np}}; });
}

}  // namespace rmswept

using namespace rmswept;

const void *rm_swept_kernel(bool bvh, int pow_mode, int stack) {
    if (!bvh) return rm_motion_shapes_kernel(false, pow_mode, stack);    // nothing to walk: the flat pass itself
    if (stack == 4)
        return pow_mode == POW_INTEGER ? (const void *)rm_swept_shade_t<POW_INTEGER, 4> : (const void *)rm_swept_shade_t<POW_GENERIC, 4>;
    if (stack == 32)
        return pow_mode == POW_INTEGER ? (const void *)rm_swept_shade_t<POW_INTEGER, 32> : (const void *)rm_swept_shade_t<POW_GENERIC, 32>;
    return nullptr;
}
