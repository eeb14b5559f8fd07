// rm_converge_moving.hip -- converging frames with moving shapes: the pixels still noisy alone are sampled, and each sample sees
// every shape -- sphere, polygon or mesh -- at a position of its own (include/rusty_marcher_amd.h, "converging frames with moving
// shapes").
//
// A pass is rm_converge_motion.hip's in everything -- the select launch is rm_converge.hip's kernel, unchanged, and the shade body
// (list, groups, per-pixel rows, lens rays, ray step, moved lights, LDS, fold, stats, count, mean and bytes) is
// rm_converge_body.inc's, not a copy -- with rm_motion_shapes.hip's rule in place of rm_motion.hip's: where a shape stands.  The
// lane that casts sample s of a listed pixel with count n holds table row r = n + s, and for that lane the primitive whose shape
// is k stands at its record + shape_offsets[r][k]: a sphere's centre, a polygon's plane point and every vertex (the pool's
// included), a triangle's centre and vertices, one addition a component, normals and materials as stored -- in the closest-hit
// walk, in both shadow walks and for the children (OffsetShapes, rm_radiance_step.inc, is the one place the additions stand).
// The table is in shape order and read through the queries' pid map.
//
// The family is the moving shapes': flat walk only (BVH = false whatever the scene image holds; a scene with a hierarchy is
// walked flat through the permuted device order), always OffsetLights + OffsetShapes, POW x STACK in {4, 32}.  What is keyed on
// a primitive's position, and why none of it is in these kernels, is rm_motion_shapes.hip's audit: the same radiance_steps with
// the same arguments stands here.
//
// Bounds.  The three tables hold table_rows rows each (the host's precondition, and what the tick keeps resident).
//   - every lane's r is < table_rows, idle lanes included: a listed pixel has count + n_samples <= max_samples <= table_rows, the
//     count as read is held to last_first = table_rows - n_samples (the body's clamp min(count, last_first)), and a lane without
//     a sample takes n = 0, r = s < n_samples <= table_rows.  So r shape_words + 3 k + 2 < table_rows x n_shapes x 3 for k < n_shapes.
//   - every pid's map word is a shape of the scene, k < n_shapes: the host checked the count against the resident scene's, whose
//     image the map was built from.  With the line above no fetch needs a predicate.
//   - a scene without shapes takes a NULL table and never fetches: the rule is asked for primitives the walks visit.  A scene
//     with any shape has a table (the host refuses a NULL one): rows of polygons and triangles are read, not of spheres alone.
//   - nothing read from an offset table ever forms an address: offsets are added to centres, plane points and vertices and to
//     nothing else, so a non-finite offset is a non-finite colour.
//
// Strict flavour, scene in global memory, occluder masks off, contraction off: as rm_converge.hip.
#define RM_KERNEL_FAST 0
#include "rm_render_kernel.hpp"
#include "rm_converge_moving.hpp"

using namespace rmdev;
using namespace rmdev_strict;

#include "rm_radiance_step.inc"

namespace rmconvergemoving {

using namespace rmradiance;

template <int POW, int STACK>
__global__ __launch_bounds__(64) void rm_converge_moving_shade_t(const double *__restrict__ scene_blob, ConvergeMotionArgs m) {
    __shared__ uint32_t bstack[64];
    __shared__ double sums[64 * 3];
    constexpr bool BVH = false;                                          // the family walks flat
    const ConvergeArgs &a = m.C;
    const uint32_t words = 3u * a.L.H.n_lights;                          // (r words < table_rows x 3 x n_lights: inside the table)
    const uint32_t shape_words = 3u * m.n_shapes;                        // (r shape_words < table_rows x 3 x n_shapes: inside the table)
    const uint32_t n_spheres = a.L.H.n_spheres, n_polygons = a.L.H.n_polygons;
    const auto lights_of = [&](uint32_t r) { return OffsetLights{a.offsets + (size_t)r * words}; };
    const auto spheres_of = [&](uint32_t r) {
        return OffsetShapes{m.shape_offsets + (size_t)r * shape_words, m.pid_map, n_spheres, n_polygons};
    };
#include "rm_converge_body.inc"
}

}  // namespace rmconvergemoving

using namespace rmconvergemoving;

const void *rm_converge_moving_kernel(bool bvh, int pow_mode, int stack) {
    (void)bvh;                                                           // the family walks flat
    if (stack == 4)
        return pow_mode == POW_INTEGER ? (const void *)rm_converge_moving_shade_t<POW_INTEGER, 4> : (const void *)rm_converge_moving_shade_t<POW_GENERIC, 4>;
    if (stack == 32)
        return pow_mode == POW_INTEGER ? (const void *)rm_converge_moving_shade_t<POW_INTEGER, 32> : (const void *)rm_converge_moving_shade_t<POW_GENERIC, 32>;
    return nullptr;
}
