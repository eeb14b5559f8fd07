// rm_camera_swept.hip -- swept hierarchies under a moving camera: the moving-scene family of rm_camera.hip (camera rule + moved
// lights + moved shapes) through a hierarchy whose boxes were refitted to every position the pass's offsets can give a primitive
// (include/rusty_marcher_amd.h, "swept hierarchies under a moving camera").
//
// The launch is rm_camera.hip's rm_camera_moving_shade_t in everything -- the body is rm_accum_body.inc's with the camera rule
// behind RM_CAMERA_ROWS, which this unit defines as rm_camera.hip does; the lights' rule is OffsetLights, the shapes' rule
// OffsetShapes' additions -- but BVH = true and SweptShapes in place of OffsetShapes, and the scene blob it is handed is a swept
// one (rm_swept_image.cpp), as rm_swept.hip's is.  bvh_walk is unchanged and reads the refitted nodes; closest_hit and any_hit
// apply the lane's rule inside the leaves (rm_trace.inc, `if constexpr (SPHERES::moves)`) exactly as the flat loops do, so a
// primitive is tested with the same operations in either walk and the hierarchy only decides which primitives are tested: the
// pass writes the flat camera pass's bytes.
//
// The camera's row is fetched inside the loop over the groups, in front of the group's rays (rm_accum_body.inc; rm_camera.hip's
// header has the reason: twelve doubles alive across the walk cost a wave a SIMD).  Kept: the row is dead before the walk begins.
//
// What is keyed on a primitive's POSITION, as it stands here (rm_swept.hip's audit, unchanged by the camera):
//   - the hierarchies: entered, because the boxes hold for every row within the extents (SweptShapes::swept admits the rule
//     past the static asserts).  The boxes are in world space and bound the primitives, not the rays: they hold wherever a ray
//     starts and whichever way it looks, so a handle of rm_swept_build serves every camera row.  Pruning by prune_at against
//     best_t stays valid: a box contains every lane's moved primitive, and the distance compared is the lane's own ray's.
//   - the bundle cull: CULL = false in radiance_steps, as before.
//   - the occluder masks: the host's header says there are none, and BVH = true never looks (shade_direct).
//   - the classified tiles' primary masks: have_mask = false.
//   - ties between equal distances: decided by the list key of a pid (closer<false>), never by a position or a visiting order.
//   - polygons have no hierarchy and are walked flat.
// What is keyed on the CAMERA's position, and why none of it is in these kernels (rm_camera.hip's audit): the classified tiles'
// primary masks and the dispatch order (the render kernels'; have_mask = false here), the bundle cull's cones (CULL = false),
// the occluder masks (none, above), the checked numerics' camera limits (the render kernels' alone).  The hierarchies are not
// among them: a walk starts from the lane's own origin and direction, whatever row gave them.
//
// Bounds.  Every lane holds a valid row s < n_samples of all four tables, idle lanes too: 4 s + 3 < 4 n_samples (lens),
// s words < n_samples x 3 x n_lights (lights), s shape_words < n_samples x 3 x n_shapes (shapes), 12 s + 11 < 12 n_samples (camera;
// the fetch stands behind `on` all the same).  Every pid's map word is a shape of the scene (< n_shapes, the host checked the
// count).  One more reader of the map than the flat family has: a leaf.  The leaves fetch records first + 1 .. first + 3
// unconditionally (the blob is padded) but ask the rule -- which reads pid_map[2 pid] and through it the offset row -- only for
// primitives the leaf holds (cnt > j, wave-uniform), so no map word beyond the scene's pids is read.  A row outside the extents
// can make a box miss its primitive: a wrong pixel, never an address -- nothing read from an offset row, a box or a camera row
// forms one.
//
// Strict flavour, scene in global memory, occluder masks off, contraction off: as rm_accum.hip.
#define RM_KERNEL_FAST 0
#define RM_CAMERA_ROWS 1
#include "rm_render_kernel.hpp"
#include "rm_camera_swept.hpp"

using namespace rmdev;
using namespace rmdev_strict;

#include "rm_radiance_step.inc"
#include "rm_camera_ray.inc"
#include "rm_accum_body.inc"

namespace rmcameraswept {

using namespace rmaccum;

template <int POW, int STACK>
__global__ __launch_bounds__(64) void rm_camera_swept_shade_t(const double *__restrict__ scene_blob, CameraArgs a) {
    __shared__ uint32_t bstack[64];
    __shared__ double sums[64 * 3];
    const SoftArgs &S = a.M.S;
    const double *offsets = S.offsets;
    const uint32_t words = 3u * S.A.L.H.n_lights;                        // (s words < 64 x 3 x n_lights: inside the table)
    const double *shape_offsets = a.M.shape_offsets;
    const uint32_t *pid_map = a.M.pid_map;
    const uint32_t shape_words = 3u * a.M.n_shapes;                      // (s shape_words < 64 x 3 x n_shapes: inside the table)
    const uint32_t ns = S.A.L.H.n_spheres, np = S.A.L.H.n_polygons;
    accum_shade<true, POW, STACK>(
        scene_blob, S.A, bstack, sums, a.camera_rows, [=](uint32_t s) { return OffsetLights{offsets + (size_t)s * words}; },
        [=](uint32_t s) { return SweptShapes{{shape_offsets + (size_t)s * shape_words, pid_map, ns, np}}; });
}

}  // namespace rmcameraswept

using namespace rmcameraswept;

const void *rm_camera_swept_kernel(bool bvh, int pow_mode, int stack) {
    if (!bvh) return rm_camera_moving_kernel(false, pow_mode, stack);    // nothing to walk: the flat pass itself
    if (stack == 4)
        return pow_mode == POW_INTEGER ? (const void *)rm_camera_swept_shade_t<POW_INTEGER, 4> : (const void *)rm_camera_swept_shade_t<POW_GENERIC, 4>;
    if (stack == 32)
        return pow_mode == POW_INTEGER ? (const void *)rm_camera_swept_shade_t<POW_INTEGER, 32> : (const void *)rm_camera_swept_shade_t<POW_GENERIC, 32>;
    return nullptr;
}
