// rm_camera.hip -- moving camera: progressive frames whose samples each see the scene from a camera of their own, so that the
// mean is blurred along the camera's motion during the shutter (include/rusty_marcher_amd.h, "moving camera").
//
// The launch is rm_soft.hip's (static scene) or rm_motion_shapes.hip's (moving scene) in everything -- groups, ray step, moved
// lights, moved shapes, LDS, fold, mean and bytes are rm_accum_body.inc's, not a copy -- but one rule: where a sample's ray
// starts.  Lane l casts table row s = l % n_samples, and for that lane the camera stands at cam + camera_rows[s][0..2], one
// addition a component, and looks along the row's own basis, camera_rows[s][3..11]; steps 1-4 of the thin-lens camera take both
// in place of the context's (camera_row_ray, rm_camera_ray.inc).  The body takes the rule where RM_CAMERA_ROWS is defined, which
// this unit and rm_converge_camera.hip alone do.
//
// The row is fetched inside the loop over the groups, in front of the group's rays, not once a lane in front of the loop where
// the lights' and shapes' rules are asked: twelve doubles alive across the ray walk took the integer-power kernel of the moving
// scene from 3 waves a SIMD to 2.  Fetched a group at a time the row is dead before the walk begins: twelve per-lane loads and
// three additions in front of hundreds of instructions, from at most 64 distinct rows a wave that stay in the vector L1.  See
// DESIGN.md section 6s for the resource-usage lines beside rm_soft.hip's and rm_motion_shapes.hip's.
//
// Two families:
//   static scene   camera rule + OffsetLights + StoredSpheres, BVH in {false, true}.  Nothing keyed on a primitive's position
//                  depends on where a ray starts: the hierarchies' boxes, the pid map and the records hold for every camera,
//                  so the hierarchy stays and the records stay scalar.  The kernel is rm_soft.hip's with the ray of the row.
//   moving scene   camera rule + OffsetLights + OffsetShapes, the flat walk.  rm_motion_shapes.hip's audit of what is keyed
//                  on a primitive's position holds unchanged: the same radiance_steps with the same arguments stands here.
// What is keyed on the CAMERA's position, and why none of it is in these kernels: the classified tiles' primary masks and the
// dispatch order (the render kernels'; radiance_steps passes have_mask = false), the bundle cull's cones (CULL = false), the
// occluder masks (the host's header says there are none), the checked numerics' camera limits (the render kernels' alone).
//
// Every lane holds a valid row (s < n_samples, idle lanes too; the fetch stands behind `on` all the same).  Nothing read from a
// camera row forms an address: a non-finite entry is a non-finite colour.
//
// Strict flavour, scene in global memory, occluder masks off, contraction off: as rm_soft.hip.
#define RM_KERNEL_FAST 0
#define RM_CAMERA_ROWS 1
#include "rm_render_kernel.hpp"
#include "rm_camera.hpp"

using namespace rmdev;
using namespace rmdev_strict;

#include "rm_radiance_step.inc"
#include "rm_camera_ray.inc"
#include "rm_accum_body.inc"

namespace rmcamerashade {

using namespace rmaccum;

template <bool BVH, int POW, int STACK>
__global__ __launch_bounds__(64) void rm_camera_shade_t(const double *__restrict__ scene_blob, CameraArgs a) {
    __shared__ uint32_t bstack[64];
    __shared__ double sums[64 * 3];
    const SoftArgs &S = a.M.S;
    const double *offsets = S.offsets;
    const uint32_t words = 3u * S.A.L.H.n_lights;                        // (s words < 64 x 3 x n_lights: inside the table)
    accum_shade<BVH, POW, STACK>(scene_blob, S.A, bstack, sums, a.camera_rows,   // (12 s + 11 < 12 n_samples: inside the table)
                                 [=](uint32_t s) { return OffsetLights{offsets + (size_t)s * words}; });
}

template <int POW, int STACK>
__global__ __launch_bounds__(64) void rm_camera_moving_shade_t(const double *__restrict__ scene_blob, CameraArgs a) {
    __shared__ uint32_t bstack[64];
    __shared__ double sums[64 * 3];
    const SoftArgs &S = a.M.S;
    const double *offsets = S.offsets;
    const uint32_t words = 3u * S.A.L.H.n_lights;                        // (s words < 64 x 3 x n_lights: inside the table)
    const double *shape_offsets = a.M.shape_offsets;
    const uint32_t *pid_map = a.M.pid_map;
    const uint32_t shape_words = 3u * a.M.n_shapes;                      // (s shape_words < 64 x 3 x n_shapes: inside the table)
    const uint32_t ns = S.A.L.H.n_spheres, np = S.A.L.H.n_polygons;
    accum_shade<false, POW, STACK>(
        scene_blob, S.A, bstack, sums, a.camera_rows, [=](uint32_t s) { return OffsetLights{offsets + (size_t)s * words}; },
        [=](uint32_t s) { return OffsetShapes{shape_offsets + (size_t)s * shape_words, pid_map, ns, np}; });
}

}  // namespace rmcamerashade

using namespace rmcamerashade;

const void *rm_camera_kernel(bool bvh, int pow_mode, int stack) {
    RM_SHADING_TABLE(RM_SHADING_KERNEL, rm_camera_shade_t)
    return nullptr;
}

const void *rm_camera_moving_kernel(bool bvh, int pow_mode, int stack) {
    (void)bvh;                                                           // the family walks flat
    if (stack == 4)
        return pow_mode == POW_INTEGER ? (const void *)rm_camera_moving_shade_t<POW_INTEGER, 4> : (const void *)rm_camera_moving_shade_t<POW_GENERIC, 4>;
    if (stack == 32)
        return pow_mode == POW_INTEGER ? (const void *)rm_camera_moving_shade_t<POW_INTEGER, 32> : (const void *)rm_camera_moving_shade_t<POW_GENERIC, 32>;
    return nullptr;
}
