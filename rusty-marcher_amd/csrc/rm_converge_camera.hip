// rm_converge_camera.hip -- converging frames with a moving camera: the pixels still noisy alone are sampled, and each sample
// sees the scene from a camera of its own (include/rusty_marcher_amd.h, "converging frames with a moving camera").
//
// A pass is rm_converge.hip's (static scene) or rm_converge_moving.hip's (moving scene) in everything -- the select launch is
// rm_converge.hip's kernel, unchanged, and the shade body (list, groups, per-pixel rows, ray step, moved lights and shapes, LDS,
// fold, stats, count, mean and bytes) is rm_converge_body.inc's, not a copy -- with rm_camera.hip's rule for where a sample's
// ray starts.  The lane that casts sample s of a listed pixel with count n holds table row r = n + s of all four tables, and
// its camera is cam + camera_rows[r][0..2] with the basis camera_rows[r][3..11] (camera_row_ray, rm_camera_ray.inc).  The body
// fetches its lens row per group already; the camera row is fetched beside it.
//
// The two families and what is keyed on a position are rm_camera.hip's: a static scene keeps its hierarchy and its scalar
// records (OffsetLights + StoredSpheres, BVH in {false, true}, rm_converge.hip's kernels with moved lights), a moving scene
// walks flat (OffsetLights + OffsetShapes, rm_converge_moving.hip's kernels and its audit).
//
// Bounds.  The camera table holds table_rows rows, as the other three (the host's precondition, and what the tick keeps
// resident).  Every lane's r is < table_rows, idle lanes included (rm_converge_moving.hip, the head of the file, has the
// argument; the body's clamps are unchanged), so 12 r + 11 < 12 table_rows.  Nothing read from a camera row forms an address.
//
// Strict flavour, scene in global memory, occluder masks off, contraction off: as rm_converge.hip.
#define RM_KERNEL_FAST 0
#define RM_CAMERA_ROWS 1
#include "rm_render_kernel.hpp"
#include "rm_converge_camera.hpp"

using namespace rmdev;
using namespace rmdev_strict;

#include "rm_radiance_step.inc"
#include "rm_camera_ray.inc"

namespace rmconvergecamera {

using namespace rmradiance;

template <bool BVH, int POW, int STACK>
__global__ __launch_bounds__(64) void rm_converge_camera_shade_t(const double *__restrict__ scene_blob, ConvergeCameraArgs m) {
    __shared__ uint32_t bstack[64];
    __shared__ double sums[64 * 3];
    const ConvergeArgs &a = m.M.C;
    const double *camera_rows = m.camera_rows;
    const uint32_t words = 3u * a.L.H.n_lights;                          // (r words < table_rows x 3 x n_lights: inside the table)
    const auto lights_of = [&](uint32_t r) { return OffsetLights{a.offsets + (size_t)r * words}; };
    const auto spheres_of = [](uint32_t) { return StoredSpheres(); };
#include "rm_converge_body.inc"
}

template <int POW, int STACK>
__global__ __launch_bounds__(64) void rm_converge_camera_moving_shade_t(const double *__restrict__ scene_blob, ConvergeCameraArgs m) {
    __shared__ uint32_t bstack[64];
    __shared__ double sums[64 * 3];
    constexpr bool BVH = false;                                          // the family walks flat
    const ConvergeArgs &a = m.M.C;
    const double *camera_rows = m.camera_rows;
    const uint32_t words = 3u * a.L.H.n_lights;                          // (r words < table_rows x 3 x n_lights: inside the table)
    const uint32_t shape_words = 3u * m.M.n_shapes;                      // (r shape_words < table_rows x 3 x n_shapes: inside the table)
    const uint32_t n_spheres = a.L.H.n_spheres, n_polygons = a.L.H.n_polygons;
    const auto lights_of = [&](uint32_t r) { return OffsetLights{a.offsets + (size_t)r * words}; };
    const auto spheres_of = [&](uint32_t r) {
        return OffsetShapes{m.M.shape_offsets + (size_t)r * shape_words, m.M.pid_map, n_spheres, n_polygons};
    };
#include "rm_converge_body.inc"
}

}  // namespace rmconvergecamera

using namespace rmconvergecamera;

const void *rm_converge_camera_kernel(bool bvh, int pow_mode, int stack) {
    RM_SHADING_TABLE(RM_SHADING_KERNEL, rm_converge_camera_shade_t)
    return nullptr;
}

const void *rm_converge_camera_moving_kernel(bool bvh, int pow_mode, int stack) {
    (void)bvh;                                                           // the family walks flat
    if (stack == 4)
        return pow_mode == POW_INTEGER ? (const void *)rm_converge_camera_moving_shade_t<POW_INTEGER, 4>
                                       : (const void *)rm_converge_camera_moving_shade_t<POW_GENERIC, 4>;
    if (stack == 32)
        return pow_mode == POW_INTEGER ? (const void *)rm_converge_camera_moving_shade_t<POW_INTEGER, 32>
                                       : (const void *)rm_converge_camera_moving_shade_t<POW_GENERIC, 32>;
    return nullptr;
}
