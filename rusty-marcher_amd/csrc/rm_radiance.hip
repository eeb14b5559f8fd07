// rm_radiance.hip -- radiance queries against the resident scene (include/rusty_marcher_amd.h, "radiance queries").
//
// cast_ray (renderer.rs:254-309) for rays of the caller's own and for real-valued sample positions of a frame: closest hit,
// direct lighting, reflected and refracted children, from the render's own pieces (rm_trace.inc) in the strict flavour --
// every operation one rounding, in the reference's order, so every hit / miss / side decision is the reference's.
//
// One lane per answer, 64 a wave.  The ray-step loop is render_tile's without the tiles: in a step every lane that holds a ray
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
// Three things differ from the render on purpose:
//   viewer direction  direct_lighting takes normalize(origin - point) (renderer.rs:149).  The render hands shade_direct -dir,
//                     sound for its unit rays; a caller's direction is unit only within the reference's assert and reflect()
//                     does not renormalise (optics.rs:4-6), so here it is neg(normalized(dir)) at every step.  Everything
//                     else takes dir as the reference does.
//   occluder masks    the per-primitive shadow masks hold for hit points of rays cast from near the scene (rm_plan.cpp);
//                     a ray list has no such bound: the host hands these kernels a header with off_occ = 0.
//   sample rays       formed here from (sx, sy) with the operations backproject_tables performs on the host, exact divisions.
#define RM_KERNEL_FAST 0
#include "rm_render_kernel.hpp"
#include "rm_radiance.hpp"

using namespace rmdev;
using namespace rmdev_strict;

namespace rmradiance {

template <bool BVH, int POW, int STACK>
__global__ __launch_bounds__(64) void rm_radiance_kernel_t(const double *__restrict__ scene_blob, RadianceArgs q) {
    __shared__ uint32_t bstack[64];
    SceneView sc;
    sc.S = scene_blob;                // no LDS copy: the rays of a wave gather from all over the scene anyway
    sc.G = scene_blob;
    sc.cull_bounds = scene_blob + q.H.off_bounds;
    sc.cull_planar = scene_blob + q.H.off_planar;
    sc.bstack = bstack;
    sc.cull_cos = 2.;                 // (never narrow: compiled without the cull)
    sc.H = q.H;

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
            // renderer.rs:128-135 at a real-valued position: the host's backproject_tables, operation for operation
            const double sx = q.xy[2u * i], sy = q.xy[2u * i + 1u];
            const double bx = 2. * (sx / q.width - 0.5) * q.half_fov * q.ratio;
            const double by = -2. * (sy / q.height - 0.5) * q.half_fov;
            const V3 d = q.mode == RM_RADIANCE_SAMPLES_ORIENTED
                             ? mk((bx * q.cam_rx + by * q.cam_ux) + q.cam_fx, (bx * q.cam_ry + by * q.cam_uy) + q.cam_fy,
                                  (bx * q.cam_rz + by * q.cam_uz) + q.cam_fz)
                             : mk(bx, by, -1.);
            dir = normalized(d);
            orig = mk(q.cam_x, q.cam_y, q.cam_z);
        }
    }

    double weight = 1.;
    uint32_t depth = 1;                                                  // renderer.rs:83
    V3 acc = mk(0., 0., 0.);
    // Parked rays: a lane works depth-first on one tree, so its parked rays have distinct depths 2 .. max_depth -- at most
    // max_depth - 1 <= STACK of them (the host picks STACK by that rule).
    StackEntry deep[STACK];
    uint32_t n_deep = 0;

    while (__any(on)) {                                                  // one ray step; the loop itself is wave-uniform
        Hit h{0., 0u};
        const bool got = closest_hit<BVH, false, false>(sc, orig, dir, on, h, false, 0ull) & on;
        // what this step adds to the lane's answer: weight x (background + direct light) on a hit (renderer.rs:272-275),
        // weight x background where a child leaves the scene (:302-303), nothing where the caller's ray does (:305), + the
        // children beyond the cap (:262-264).  Lanes without a ray add zero.
        V3 L = bg;
        const double w_add = (on & (got | (depth > 1u))) ? weight : 0.;
        double w_cap = 0.;
        bool next = false;                                               // the lane goes on with a child of its ray
        if (__any(got)) {
            const Surface s = surface_at<false>(sc, orig, dir, h, got);
            L = pick(got, bg + shade_direct<POW, BVH, false, false>(sc, neg(normalized(dir)), s, got, h.pid), bg);
            const bool glass = got & (s.mat[8] != 0.);                   // is_glass_like, renderer.rs:277
            if (__any(glass)) {
                const double reflection = s.mat[6], ri = s.mat[7], inv_ri = s.mat[9];
                V3 ro, rd, to, td;
                const bool has_r = glass & reflect_child<false>(dir, s, ri, inv_ri, ro, rd);   // renderer.rs:195-222
                const bool has_t = glass & refract_child(dir, s, ri, inv_ri, glass, to, td);   // renderer.rs:225-252
                const double wr = weight * reflection, wt = weight * (1. - reflection);
                const bool capped = depth + 1u > q.max_depth;            // such a child returns the background
                w_cap = ((capped & has_r) ? wr : 0.) + ((capped & has_t) ? wt : 0.);
                const bool live_r = has_r & !capped, live_t = has_t & !capped;
                // both children: park the reflected sibling (the bound cannot bite -- see above -- and keeps a store in its array)
                const bool park = live_r & live_t & (n_deep < (uint32_t)STACK);
                if (park) {
                    StackEntry &e = deep[n_deep];
                    e.ox = ro.x; e.oy = ro.y; e.oz = ro.z;
                    e.dx = rd.x; e.dy = rd.y; e.dz = rd.z;
                    e.w = wr; e.depth = depth + 1u;
                }
                n_deep += park ? 1u : 0u;
                // walk into the refracted child, else the reflected one
                next = live_r | live_t;
                orig = pick(live_t, to, pick(live_r, ro, orig));
                dir = pick(live_t, td, pick(live_r, rd, dir));
                weight = live_t ? wt : live_r ? wr : weight;
                depth += next ? 1u : 0u;
            }
        }
        acc = acc + mk(__builtin_fma(bg.x, w_cap, L.x * w_add), __builtin_fma(bg.y, w_cap, L.y * w_add),
                       __builtin_fma(bg.z, w_cap, L.z * w_add));
        // a lane whose ray ended takes its deepest parked ray
        const bool pop = on & !next & (n_deep > 0u);
        if (__any(pop)) {
            n_deep -= pop ? 1u : 0u;
            const StackEntry &e = deep[pop ? n_deep : 0u];
            orig = pick(pop, mk(e.ox, e.oy, e.oz), orig);
            dir = pick(pop, mk(e.dx, e.dy, e.dz), dir);
            weight = pop ? e.w : weight;
            depth = pop ? e.depth : depth;
        }
        on = on & (next | pop);
    }

    // (the index formed again rather than held across the ray steps)
    const size_t at = (size_t)blockIdx.x * 64u + (threadIdx.x & 63u);
    if (at < (size_t)q.n) q.rgb[at] = rm_vec3{acc.x, acc.y, acc.z};
}

}  // namespace rmradiance

using namespace rmradiance;

const void *rm_radiance_kernel(bool bvh, int pow_mode, int stack) {
#define RM_ROW(B, S)                                                                                         \
    if (bvh == B && stack == S)                                                                              \
        return pow_mode == POW_INTEGER ? (const void *)rm_radiance_kernel_t<B, POW_INTEGER, S>               \
                                       : (const void *)rm_radiance_kernel_t<B, POW_GENERIC, S>;
    RM_ROW(false, 4) RM_ROW(false, 32) RM_ROW(true, 4) RM_ROW(true, 32)
#undef RM_ROW
    return nullptr;
}
