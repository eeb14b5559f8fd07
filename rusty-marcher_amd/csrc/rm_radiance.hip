// rm_radiance.hip -- radiance queries against the resident scene (include/rusty_marcher_amd.h, "radiance queries").
//
// cast_ray (renderer.rs:254-309) for rays of the caller's own and for real-valued sample positions of a frame: closest hit,
// direct lighting, reflected and refracted children, from the render's own pieces (rm_trace.inc) in the strict flavour --
// every operation one rounding, in the reference's order, so every hit / miss / side decision is the reference's.
//
// One lane per answer, 64 a wave.  The ray-step loop -- radiance_steps of rm_radiance_step.inc, which rm_refine.hip includes
// too -- is render_tile's without the tiles: in a step every lane that holds a ray
// finds its closest hit, shades it and turns into the refracted (else the reflected) child; where both exist the reflected one
// is parked on the lane's own stack, and a lane whose ray ended takes its deepest parked ray.  Radiance is linear in the
// children (renderer.rs:219,249), so a ray carries the product of the factors above it.  No LDS scene copy, no classification,
// no bundle cull (a ray list has no common apex), no hand-over of parked rays.
//
// Divergence.  The rays of a wave are unrelated and finish at different steps, while the walks vote and -- the hierarchy's --
// share one stack per wave in LDS.  So the loop is wave-uniform: it ends when no lane holds a ray, every block is entered on a
// vote and predicated inside (where<false> of rm_trace.inc, as the render's kernels with the bundle cull have it), and a lane
// without a ray walks along with its `on` off.  Lanes past the last answer are such lanes from the start.
//
// Four things differ from the render on purpose:
//   ray length        a caller's direction is unit only within the reference's assert, and the hierarchy's boxes and pruning
//                     distance hold for unit rays: a step whose wave holds a ray that is not takes the complete walk
//                     (rm_radiance_step.inc, complete_walk_view).
//   viewer direction  direct_lighting takes normalize(origin - point) (renderer.rs:149).  The render hands shade_direct -dir,
//                     sound for its unit rays from a camera that stands clear of every surface; a caller's ray may be off
//                     unit length within the reference's assert, and it may START on a surface, where origin - point is the
//                     zero vector or a few ulps of rounding: here it is normalized(orig - point) at every step, as the
//                     reference has it.  Everything else takes dir as the reference does.
//   occluder masks    the per-primitive shadow masks hold for hit points of rays cast from near the scene (rm_plan.cpp);
//                     a ray list has no such bound: the host hands these kernels a header with off_occ = 0.
//   sample rays       formed here from (sx, sy) with the operations backproject_tables performs on the host, exact divisions.
#define RM_KERNEL_FAST 0
#include "rm_render_kernel.hpp"
#include "rm_radiance.hpp"

using namespace rmdev;
using namespace rmdev_strict;

#include "rm_radiance_step.inc"

namespace rmradiance {

template <bool BVH, int POW, int STACK>
__global__ __launch_bounds__(64) void rm_radiance_kernel_t(const double *__restrict__ scene_blob, RadianceArgs q) {
    __shared__ uint32_t bstack[64];
    const SceneView sc = global_scene_view(scene_blob, q.H, bstack);

    const size_t i = (size_t)blockIdx.x * 64u + (threadIdx.x & 63u);     // (64-bit: 2^32 answers x 24 B)
    bool on = i < (size_t)q.n;
    const V3 bg = mk(q.bg_x, q.bg_y, q.bg_z);
    if (q.max_depth == 0u) {                                             // renderer.rs:262-264 at n_recursion = 1
        if (on) q.rgb[i] = rm_vec3{bg.x, bg.y, bg.z};
        return;
    }

    V3 orig = mk(0., 0., 0.), dir = mk(0., 0., -1.);                     // (a tail lane holds a harmless ray it never casts)
    if (q.mode == RM_RADIANCE_RAYS) {                                    // wave-uniform
        if (on) {
            const rm_vec3 ro = q.origins[i], rd = q.directions[i];
            orig = mk(ro.x, ro.y, ro.z);
            dir = mk(rd.x, rd.y, rd.z);
        }
    } else {
        if (on) {
            // renderer.rs:128-135 at a real-valued position (sample_direction, rm_radiance_step.inc)
            const V3 d = sample_direction(q, q.mode == RM_RADIANCE_SAMPLES_ORIENTED, q.xy[2u * i], q.xy[2u * i + 1u]);
            dir = normalized(d);
            orig = mk(q.cam_x, q.cam_y, q.cam_z);
        }
    }

    // (ADMIT: a caller's ray may be off unit length within the assert; the sample rays are normalised and pass its vote)
    const V3 acc = radiance_steps<BVH, POW, STACK, StoredLights, StoredSpheres, true>(sc, orig, dir, on, bg, q.max_depth);   // rm_radiance_step.inc

    // (the index formed again rather than held across the ray steps)
    const size_t at = (size_t)blockIdx.x * 64u + (threadIdx.x & 63u);
    if (at < (size_t)q.n) q.rgb[at] = rm_vec3{acc.x, acc.y, acc.z};
}

}  // namespace rmradiance

using namespace rmradiance;

const void *rm_radiance_kernel(bool bvh, int pow_mode, int stack) {
    RM_SHADING_TABLE(RM_SHADING_KERNEL, rm_radiance_kernel_t)
    return nullptr;
}
