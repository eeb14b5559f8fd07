// rm_converge_swept.hip -- converging frames over a swept hierarchy: rm_converge_moving.hip's pass through a hierarchy whose boxes
// were refitted to every position the pass's offsets can give a primitive (include/rusty_marcher_amd.h, "swept hierarchies").
//
// A pass is rm_converge_moving.hip's in everything -- select launch, shade body (rm_converge_body.inc), the lane's row r = n + s,
// OffsetShapes' additions -- but BVH = true, and the scene blob it is handed is a swept one (rm_swept_image.cpp).  What that
// changes in the walks, why the bytes are the flat pass's, and the audit of what is keyed on a primitive's position, are
// rm_swept.hip's: the same radiance_steps with the same arguments stands here.
//
// Bounds: rm_converge_moving.hip's -- every lane's r < table_rows, every map word a shape of the scene -- and rm_swept.hip's for
// the leaves: the rule is asked only for primitives a leaf holds, so no map word beyond the scene's pids is read.
//
// Strict flavour, scene in global memory, occluder masks off, contraction off: as rm_converge.hip.
#define RM_KERNEL_FAST 0
#include "rm_render_kernel.hpp"
#include "rm_converge_swept.hpp"

using namespace rmdev;
using namespace rmdev_strict;

#include "rm_radiance_step.inc"

namespace rmconvergeswept {

using namespace rmradiance;

template <int POW, int STACK>
__global__ __launch_bounds__(64) void rm_converge_swept_shade_t(const double *__restrict__ scene_blob, ConvergeMotionArgs m) {
    __shared__ uint32_t bstack[64];
    __shared__ double sums[64 * 3];
    constexpr bool BVH = true;                                           // the blob's hierarchies are swept over the offsets
    const ConvergeArgs &a = m.C;
    const uint32_t words = 3u * a.L.H.n_lights;                          // (r words < table_rows x 3 x n_lights: inside the table)
    const uint32_t shape_words = 3u * m.n_shapes;                        // (r shape_words < table_rows x 3 x n_shapes: inside the table)
    const uint32_t n_spheres = a.L.H.n_spheres, n_polygons = a.L.H.n_polygons;
    const auto lights_of = [&](uint32_t r) { return OffsetLights{a.offsets + (size_t)r * words}; };
    const auto spheres_of = [&](uint32_t r) {
        return SweptShapes{{m.shape_offsets + (size_t)r * shape_words, m.pid_map, n_spheres, n_polygons}};
    };
#include "rm_converge_body.inc"
}

}  // namespace rmconvergeswept

using namespace rmconvergeswept;

const void *rm_converge_swept_kernel(bool bvh, int pow_mode, int stack) {
    if (!bvh) return rm_converge_moving_kernel(false, pow_mode, stack);  // nothing to walk: the flat pass itself
    if (stack == 4)
        return pow_mode == POW_INTEGER ? (const void *)rm_converge_swept_shade_t<POW_INTEGER, 4> : (const void *)rm_converge_swept_shade_t<POW_GENERIC, 4>;
    if (stack == 32)
        return pow_mode == POW_INTEGER ? (const void *)rm_converge_swept_shade_t<POW_INTEGER, 32> : (const void *)rm_converge_swept_shade_t<POW_GENERIC, 32>;
    return nullptr;
}
