// rm_converge_camera_swept.hip -- converging frames with a moving camera over a swept hierarchy: the moving-scene family of
// rm_converge_camera.hip through a hierarchy whose boxes were refitted to every position the pass's offsets can give a primitive
// (include/rusty_marcher_amd.h, "swept hierarchies under a moving camera").
//
// A pass is rm_converge_camera.hip's rm_converge_camera_moving_shade_t in everything -- the select launch is rm_converge.hip's
// kernel, unchanged, the shade body is rm_converge_body.inc's with the camera rule behind RM_CAMERA_ROWS (the camera row is
// fetched per group, beside the lens row), the lane's row is r = n + s of all four tables, the shapes' rule is OffsetShapes'
// additions -- but BVH = true and SweptShapes, and the scene blob it is handed is a swept one (rm_swept_image.cpp), as
// rm_converge_swept.hip's is.  What that changes in the walks, why the bytes are the flat pass's, and both audits -- what is keyed
// on a primitive's position (the hierarchies, entered because the boxes hold for every row within the extents and, being in
// world space, for every camera row; nothing else) and what is keyed on the camera's position (nothing in these kernels) --
// are rm_camera_swept.hip's: the same radiance_steps with the same arguments stands here.
//
// Bounds: rm_converge_camera.hip's -- every lane's r < table_rows of all four tables, idle lanes included, so 12 r + 11 <
// 12 table_rows; every map word a shape of the scene -- and rm_swept.hip's for the leaves: the rule is asked only for primitives a
// leaf holds (cnt > j), so no map word beyond the scene's pids is read.  Nothing read from an offset row, a box or a camera row
// forms an address: a row outside the extents is a wrong pixel.
//
// Strict flavour, scene in global memory, occluder masks off, contraction off: as rm_converge.hip.
#define RM_KERNEL_FAST 0
#define RM_CAMERA_ROWS 1
#include "rm_render_kernel.hpp"
#include "rm_converge_camera_swept.hpp"

using namespace rmdev;
using namespace rmdev_strict;

#include "rm_radiance_step.inc"
#include "rm_camera_ray.inc"

namespace rmconvergecameraswept {

using namespace rmradiance;

template <int POW, int STACK>
__global__ __launch_bounds__(64) void rm_converge_camera_swept_shade_t(const double *__restrict__ scene_blob, ConvergeCameraArgs m) {
    __shared__ uint32_t bstack[64];
    __shared__ double sums[64 * 3];
    constexpr bool BVH = true;                                           // the blob's hierarchies are swept over the offsets
    const ConvergeArgs &a = m.M.C;
    const double *camera_rows = m.camera_rows;
    const uint32_t words = 3u * a.L.H.n_lights;                          // (r words < table_rows x 3 x n_lights: inside the table)
    const uint32_t shape_words = 3u * m.M.n_shapes;                      // (r shape_words < table_rows x 3 x n_shapes: inside the table)
    const uint32_t n_spheres = a.L.H.n_spheres, n_polygons = a.L.H.n_polygons;
    const auto lights_of = [&](uint32_t r) { return OffsetLights{a.offsets + (size_t)r * words}; };
    const auto spheres_of = [&](uint32_t r) {
        return SweptShapes{{m.M.shape_offsets + (size_t)r * shape_words, m.M.pid_map, n_spheres, n_polygons}};
    };
#include "rm_converge_body.inc"
}

}  // namespace rmconvergecameraswept

using namespace rmconvergecameraswept;

const void *rm_converge_camera_swept_kernel(bool bvh, int pow_mode, int stack) {
    if (!bvh) return rm_converge_camera_moving_kernel(false, pow_mode, stack);   // nothing to walk: the flat pass itself
    if (stack == 4)
        return pow_mode == POW_INTEGER ? (const void *)rm_converge_camera_swept_shade_t<POW_INTEGER, 4>
                                       : (const void *)rm_converge_camera_swept_shade_t<POW_GENERIC, 4>;
    if (stack == 32)
        return pow_mode == POW_INTEGER ? (const void *)rm_converge_camera_swept_shade_t<POW_INTEGER, 32>
                                       : (const void *)rm_converge_camera_swept_shade_t<POW_GENERIC, 32>;
    return nullptr;
}
