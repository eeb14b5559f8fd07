// rm_query.hip -- ray queries against the resident scene (include/rusty_marcher_amd.h, "ray queries").
//
// The render's own intersection engine (rm_trace.inc) without the shading:
//   closest hit : find_closest_intersect (shapes.rs:110-143) -- closest_hit + surface_at
//   occlusion   : intersect_shape_set (shapes.rs:92-108)     -- any_hit
// compiled once, in the strict flavour (every operation one rounding, in the reference's order):
// hit / miss / shape decisions are the reference's bit for bit whatever flavour the frames use.
//
// Ray lists: one lane per ray, 64 rays a wave.  The walks are wave-uniform (votes, scalar record
// loads, the wave's hierarchy stack in LDS), so incoherent rays are answered correctly, only with
// less sharing per wave.  Lanes past the last ray stay in the wave with their `on` off: a walk's
// votes need all 64 lanes.  No bundle cull: the shadow rays' cull (bundle_through) assumes that
// every ray passes near one light, and the primary rays' (bundle_of_rays) pays only for rays
// leaving one point; the hierarchy (where the upload built one) does the pruning.
//
// Pixels: one wave per 16x4 tile of the render (TILE_W x TILE_H), so the rays of a wave stay
// coherent.  The direction of pixel (x, y) is normalized(bp_x[x], bp_y[y], -1) from the render's
// own tables with the strict flavour's normalized(): bit for bit the ray the strict render casts
// there (rm_render_kernel.inc render_tile).  The render's tile classification and dispatch order
// are neither used nor touched.
#define RM_KERNEL_FAST 0
#include "rm_render_kernel.hpp"
#include "rm_query.hpp"

using namespace rmdev;
using namespace rmdev_strict;

namespace rmquery {

__device__ __forceinline__ SceneView query_view(const double *__restrict__ blob, const rm_dev_header &H, uint32_t *bstack) {
    SceneView sc;
    sc.S = blob;                      // no LDS copy: the per-lane gathers of a query are few
    sc.G = blob;
    sc.cull_bounds = blob + H.off_bounds;
    sc.cull_planar = blob + H.off_planar;
    sc.bstack = bstack;
    sc.cull_cos = 2.;                 // (never narrow: the kernels below are compiled without the cull anyway)
    sc.H = H;
    return sc;
}

// One rm_hit: the point and normal of surface_at (sphere.rs:58, polygon.rs:95, triangle.rs:80), the
// pid mapped back to Scene.shapes.  Every field of a miss is 0.
__device__ __forceinline__ void store_hit(const QueryArgs &q, const SceneView &sc, rm_hit *dst, V3 o, V3 d, const Hit &h,
                                          bool got) {
    const Surface s = surface_at<true>(sc, o, d, h, got);
    rm_hit r;
    r.t = got ? h.t : 0.;
    r.point = rm_vec3{got ? s.point.x : 0., got ? s.point.y : 0., got ? s.point.z : 0.};
    r.normal = rm_vec3{got ? s.normal.x : 0., got ? s.normal.y : 0., got ? s.normal.z : 0.};
    r.shape = got ? q.pid_map[2u * h.pid] : 0u;
    r.element = got ? q.pid_map[2u * h.pid + 1u] : 0u;
    r.hit = got ? 1 : 0;
    r._pad = 0u;
    *dst = r;
}

template <bool BVH, bool OCCLUSION>
__global__ __launch_bounds__(64) void rm_query_rays_kernel(const double *__restrict__ scene_blob, QueryArgs q) {
    __shared__ uint32_t bstack[64];
    const SceneView sc = query_view(scene_blob, q.H, bstack);
    const size_t i = (size_t)blockIdx.x * 64u + (threadIdx.x & 63u);     // (64-bit: 60 M rays x 72 B is past 4 GB)
    const bool on = i < (size_t)q.n_rays;
    V3 o = mk(0., 0., 0.), d = mk(0., 0., -1.);                          // (a tail lane holds a harmless ray it never reports)
    if (on) {
        const rm_vec3 ro = q.origins[i], rd = q.directions[i];
        o = mk(ro.x, ro.y, ro.z);
        d = mk(rd.x, rd.y, rd.z);
    }
    if (OCCLUSION) {
        // (through / rho feed the shadow cull only, which these kernels do not carry)
        const bool occ = any_hit<BVH, false, false>(sc, o, d, !on, o, 0.);
        if (on) q.occluded[i] = occ ? 1u : 0u;
    } else {
        Hit h{0., 0u};
        const bool got = closest_hit<BVH, false, false>(sc, o, d, on, h, false, 0ull);
        if (on) store_hit(q, sc, q.hits + i, o, d, h, got);
    }
}

template <bool BVH, bool ORIENTED>
__global__ __launch_bounds__(64) void rm_query_pixels_kernel(const double *__restrict__ scene_blob, QueryArgs q) {
    __shared__ uint32_t bstack[64];
    const SceneView sc = query_view(scene_blob, q.H, bstack);
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t x, y;
    bool on;
    if (q.n_tiles == 0u) {                                               // one pixel (rm_pick): lane 0 holds its ray
        x = q.pick_x; y = q.pick_y; on = lane == 0u;
    } else {                                                             // tiles of whole patch rows: every lane in the frame
        const uint32_t tile = blockIdx.x;
        x = (tile % q.tiles_per_row) * TILE_W + lane % TILE_W;
        y = (tile / q.tiles_per_row) * TILE_H + lane / TILE_W;
        on = true;
    }
    // renderer.rs:80 / :128-135, exactly as the strict render kernel forms it
    // (ORIENTED: ... and as the oriented one does, (bx right + by up) + forward, every operation rounded once)
    const double bx = q.bp_x[x], by = q.bp_y[y];
    const V3 d = normalized(ORIENTED ? mk((bx * q.cam_rx + by * q.cam_ux) + q.cam_fx, (bx * q.cam_ry + by * q.cam_uy) + q.cam_fy, (bx * q.cam_rz + by * q.cam_uz) + q.cam_fz)
                                     : mk(bx, by, -1.));
    const V3 o = mk(q.cam_x, q.cam_y, q.cam_z);
    Hit h{0., 0u};
    const bool got = closest_hit<BVH, false, false>(sc, o, d, on, h, false, 0ull);
    if (on) store_hit(q, sc, q.hits + (q.n_tiles == 0u ? (size_t)0 : (size_t)y * q.frame_width + x), o, d, h, got);
}

}  // namespace rmquery

using namespace rmquery;

const void *rm_query_kernel(int kind, bool bvh, bool oriented) {
    switch (kind) {
    case RM_QUERY_CLOSEST: return bvh ? (const void *)rm_query_rays_kernel<true, false> : (const void *)rm_query_rays_kernel<false, false>;
    case RM_QUERY_OCCLUDED: return bvh ? (const void *)rm_query_rays_kernel<true, true> : (const void *)rm_query_rays_kernel<false, true>;
    case RM_QUERY_PIXELS:
        if (oriented) return bvh ? (const void *)rm_query_pixels_kernel<true, true> : (const void *)rm_query_pixels_kernel<false, true>;
        return bvh ? (const void *)rm_query_pixels_kernel<true, false> : (const void *)rm_query_pixels_kernel<false, false>;
    default: return nullptr;
    }
}
