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
//
// Ranged queries (rm_*_ranged, rm_visible_segments, rm_lights_visible): the ray-list walks once more with a closed range of
// the ray parameter on every lane, in kernels of their own below the two above; segments and (point, light) pairs form their
// rays in registers.  A bounded ray prunes the hierarchy by the end of its range from the first node.
#define RM_KERNEL_FAST 0
#include "rm_render_kernel.hpp"
#include "rm_query.hpp"

using namespace rmdev;
using namespace rmdev_strict;

#include "rm_radiance_step.inc"   // global_scene_view: the scene in global memory, no LDS copy (the per-lane gathers of a query are few)

namespace rmquery {

using rmradiance::global_scene_view;
using rmradiance::off_unit;
using rmradiance::complete_walk_view;

// One rm_hit: the point and normal of surface_at (sphere.rs:58, polygon.rs:95, triangle.rs:80), the
// pid mapped back to Scene.shapes.  Every field of a miss is 0.
template <class Args>
__device__ __forceinline__ void store_hit(const Args &q, const SceneView &sc, rm_hit *dst, V3 o, V3 d, const Hit &h,
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
    const SceneView stored = global_scene_view(scene_blob, q.H, bstack);
    const size_t i = (size_t)blockIdx.x * 64u + (threadIdx.x & 63u);     // (64-bit: 60 M rays x 72 B is past 4 GB)
    const bool on = i < (size_t)q.n_rays;
    V3 o = mk(0., 0., 0.), d = mk(0., 0., -1.);                          // (a tail lane holds a harmless ray it never reports)
    if (on) {
        const rm_vec3 ro = q.origins[i], rd = q.directions[i];
        o = mk(ro.x, ro.y, ro.z);
        d = mk(rd.x, rd.y, rd.z);
    }
    // a caller's ray may be off unit length within the assert: its wave takes the complete walk (rm_radiance_step.inc)
    const SceneView sc = BVH ? complete_walk_view(stored, __any(on & off_unit(d))) : stored;
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
    const SceneView sc = global_scene_view(scene_blob, q.H, bstack);
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


// ---- ranged queries (include/rusty_marcher_amd.h, "ranged ray queries") -----------------------------------------
// The same walks with a closed range [lo, hi] of the ray parameter on every lane.  Each primitive offers the candidates the
// reference forms -- the two roots of sphere.rs:43-45, the one dist of polygon.rs:71-76 / triangle.rs:62-67 -- from
// rm_trace.inc's own pieces; only the acceptance differs.  With [0, +inf] on a lane every decision below is the unranged
// walk's, bit for bit.
struct Range { double lo, hi; };
// Closed; written so that a parameter that is not a number lies in every range, as it passes the reference's `t < 0`.
__device__ __forceinline__ bool in_range(double t, const Range &r) { return !(t < r.lo) & !(t > r.hi); }
// Where a box may still be entered: the margin of closest_hit's prune_at (for rays unit within RM_UNIT_SLACK: a wave that
// holds another walks without boxes; +inf stays +inf).
__device__ __forceinline__ double range_cap(const Range &r) { return r.hi * (1. + 1e-7) + 1e-12; }

// sphere.rs:43-52 with the range: the near root if it lies in the range, else the far one if that does.
template <bool ORDERED_WALK>
__device__ __forceinline__ void ranged_sphere(const SceneView &sc, ClosestState &c, const SphereRec &s, uint32_t pid, V3 o, V3 d,
                                              bool on, const Range &r) {
    double tca, d2;
    sphere_setup(s, o, d, tca, d2);
    const bool in = on & !(d2 > s.r2);                               // sphere.rs:37
    if (!__any(in)) return;
    const double thc = __builtin_sqrt(s.r2 - d2);                   // (the strict flavour's RM_SQRT_DISCRIMINANT, as closest_sphere here)
    const double t0 = tca - thc;
    const double t1 = tca + thc;
    const bool near = in_range(t0, r);
    const double t = near ? t0 : t1;
    const bool valid = in & (near | in_range(t1, r));
    const V3 p = o + scaled(d, t);
    const V3 dp = p - o;
    const double dist = dot(dp, dp);                                 // shapes.rs:128
    closest_update(c, closer<ORDERED_WALK>(sc, valid, c.hit, dist, c.best, pid, c.best_pid), dist, t, pid);
}

template <bool ORDERED_WALK>
__device__ __forceinline__ void ranged_polygon(const SceneView &sc, ClosestState &c, uint32_t g, V3 o, V3 d, bool on, const Range &r) {
    const PolyRec pg = load_polygon(sc.G, sc.H, g);
    double dist = 0.;
    V3 p;
    const bool inside = polygon_hit(sc.G, sc.H, pg, pg.q, o, d, on, dist, p);
    const bool valid = inside & in_range(dist, r);
    if (!__any(valid)) return;
    const V3 dp = p - o;
    const double dh = dot(dp, dp);
    const uint32_t pid = sc.H.n_spheres + g;
    closest_update(c, closer<ORDERED_WALK>(sc, valid, c.hit, dh, c.best, pid, c.best_pid), dh, dist, pid);
}

template <bool ORDERED_WALK>
__device__ __forceinline__ void ranged_triangle(const SceneView &sc, ClosestState &c, const TriRec &t, uint32_t k, V3 o, V3 d, bool on,
                                                const Range &r) {
    double dist = 0.;
    V3 p;
    const bool inside = triangle_hit(t, o, d, on, dist, p);
    const bool valid = inside & in_range(dist, r);
    if (!__any(valid)) return;
    const V3 dp = p - o;
    const double dh = dot(dp, dp);
    const uint32_t pid = sc.H.n_spheres + sc.H.n_polygons + k;
    closest_update(c, closer<ORDERED_WALK>(sc, valid, c.hit, dh, c.best, pid, c.best_pid), dh, dist, pid);
}

// closest_hit's plain / hierarchy walk (no bundle cull, no mask), the range on every test; a box is entered only where it
// begins before the lane's best hit AND before the end of its range.
template <bool BVH>
__device__ __forceinline__ bool closest_hit_ranged(const SceneView &sc, V3 o, V3 d, bool on, const Range &r, Hit &out) {
    const double *__restrict__ S = sc.G;
    const rm_dev_header &H = sc.H;
    ClosestState c{false, 0., 0., 0u};
    RayBox rb{};
    if (BVH) rb = ray_box(o, d);
    // (the end of the range formed at every node rather than held: two registers less, and with them 8 waves a SIMD)
    auto limit = [&]() { return __builtin_fmin(c.hit ? c.best_t : __builtin_inf(), r.hi) * (1. + 1e-7) + 1e-12; };
    auto off_lane = [&]() { return !on; };

    uint32_t i = 0;
    if (BVH && H.off_bvh_spheres) {
        bvh_walk(sc, H.off_bvh_spheres, rb, limit, off_lane, [&](uint32_t first, uint32_t cnt) {
            const SphereRec s0 = load_sphere(S, H, first), s1 = load_sphere(S, H, first + 1u);
            const SphereRec s2 = load_sphere(S, H, first + 2u), s3 = load_sphere(S, H, first + 3u);
            ranged_sphere<false>(sc, c, s0, first, o, d, on, r);
            if (cnt > 1u) ranged_sphere<false>(sc, c, s1, first + 1u, o, d, on, r);
            if (cnt > 2u) ranged_sphere<false>(sc, c, s2, first + 2u, o, d, on, r);
            if (cnt > 3u) ranged_sphere<false>(sc, c, s3, first + 3u, o, d, on, r);
        });
        i = H.n_spheres;
    }
    for (; i + 4u <= H.n_spheres; i += 4u) {
        const SphereRec s0 = load_sphere(S, H, i), s1 = load_sphere(S, H, i + 1u);
        const SphereRec s2 = load_sphere(S, H, i + 2u), s3 = load_sphere(S, H, i + 3u);
        ranged_sphere<true>(sc, c, s0, i, o, d, on, r);
        ranged_sphere<true>(sc, c, s1, i + 1u, o, d, on, r);
        ranged_sphere<true>(sc, c, s2, i + 2u, o, d, on, r);
        ranged_sphere<true>(sc, c, s3, i + 3u, o, d, on, r);
    }
    for (; i < H.n_spheres; i++) ranged_sphere<true>(sc, c, load_sphere(S, H, i), i, o, d, on, r);

    for (uint32_t g = 0; g < H.n_polygons; g++) ranged_polygon<true>(sc, c, g, o, d, on, r);

    uint32_t k = 0;
    if (BVH && H.off_bvh_triangles) {
        bvh_walk(sc, H.off_bvh_triangles, rb, limit, off_lane, [&](uint32_t first, uint32_t cnt) {
            const TriRec t0 = load_triangle(S, H, first), t1 = load_triangle(S, H, first + 1u);
            ranged_triangle<false>(sc, c, t0, first, o, d, on, r);
            if (cnt > 1u) ranged_triangle<false>(sc, c, t1, first + 1u, o, d, on, r);
        });
        k = H.n_triangles;
    }
    for (; k + 2u <= H.n_triangles; k += 2u) {
        const TriRec t0 = load_triangle(S, H, k), t1 = load_triangle(S, H, k + 1u);
        ranged_triangle<true>(sc, c, t0, k, o, d, on, r);
        ranged_triangle<true>(sc, c, t1, k + 1u, o, d, on, r);
    }
    for (; k < H.n_triangles; k++) ranged_triangle<true>(sc, c, load_triangle(S, H, k), k, o, d, on, r);

    out.t = c.best_t;
    out.pid = c.best_pid;
    return c.hit;
}

// A sphere occludes when either root lies in the range.  `full`: the lane's range is [0, +inf] -- then tca >= 0 already gives
// t1 = tca + thc >= 0 without the square root, as shadow_sphere has it.
__device__ __forceinline__ bool ranged_shadow_sphere(const SphereRec &s, V3 o, V3 d, bool occ, const Range &r, bool full) {
    double tca, d2;
    sphere_setup(s, o, d, tca, d2);
    const bool in = !(d2 > s.r2);
    const bool quick = full & !(tca < 0.);
    bool hit = in & quick;
    const bool need = in & !quick & !occ;
    if (__any(need)) {
        const double thc = __builtin_sqrt(s.r2 - d2);
        const double t0 = tca - thc;
        const double t1 = tca + thc;
        hit = hit | (need & (in_range(t0, r) | in_range(t1, r)));
    }
    return hit;
}

// any_hit's plain / hierarchy walk with the range; `decided` lanes (no ray, an empty range) come back as occluded.  The hierarchy
// is pruned by the end of the range alone.
template <bool BVH>
__device__ __forceinline__ bool any_hit_ranged(const SceneView &sc, V3 o, V3 d, bool decided, const Range &r) {
    const double *__restrict__ S = sc.G;
    const rm_dev_header &H = sc.H;
    bool occ = decided;
    if (__all(occ)) return occ;
    const bool full = (r.lo == 0.) & (r.hi == __builtin_inf());
    RayBox rb{};
    if (BVH) rb = ray_box(o, d);
    const double cap = range_cap(r);
    auto limit = [&]() { return cap; };
    auto occluded = [&]() { return occ; };
    // (the test first, then its dist: two statements at every call, the order of a call's arguments being unspecified)
    auto planar = [&](bool hit, double dist) { occ = occ | (hit & in_range(dist, r)); };

    uint32_t i = 0;
    if (BVH && H.off_bvh_spheres) {
        bvh_walk(sc, H.off_bvh_spheres, rb, limit, occluded, [&](uint32_t first, uint32_t cnt) {
            const SphereRec s0 = load_sphere(S, H, first), s1 = load_sphere(S, H, first + 1u);
            const SphereRec s2 = load_sphere(S, H, first + 2u), s3 = load_sphere(S, H, first + 3u);
            occ = occ | ranged_shadow_sphere(s0, o, d, occ, r, full);
            if (cnt > 1u) occ = occ | ranged_shadow_sphere(s1, o, d, occ, r, full);
            if (cnt > 2u) occ = occ | ranged_shadow_sphere(s2, o, d, occ, r, full);
            if (cnt > 3u) occ = occ | ranged_shadow_sphere(s3, o, d, occ, r, full);
        });
        if (__all(occ)) return occ;
        i = H.n_spheres;
    }
    for (; i + 4u <= H.n_spheres; i += 4u) {
        const SphereRec s0 = load_sphere(S, H, i), s1 = load_sphere(S, H, i + 1u);
        const SphereRec s2 = load_sphere(S, H, i + 2u), s3 = load_sphere(S, H, i + 3u);
        occ = occ | ranged_shadow_sphere(s0, o, d, occ, r, full);
        occ = occ | ranged_shadow_sphere(s1, o, d, occ, r, full);
        occ = occ | ranged_shadow_sphere(s2, o, d, occ, r, full);
        occ = occ | ranged_shadow_sphere(s3, o, d, occ, r, full);
        if (__all(occ)) return occ;
    }
    for (; i < H.n_spheres; i++) occ = occ | ranged_shadow_sphere(load_sphere(S, H, i), o, d, occ, r, full);
    if (__all(occ)) return occ;

    for (uint32_t g = 0; g < H.n_polygons; g++) {
        const PolyRec pg = load_polygon(S, H, g);
        double dist = 0.;
        V3 p;
        const bool inside = polygon_hit(S, H, pg, pg.q, o, d, !occ, dist, p);
        planar(inside, dist);
        if (__all(occ)) return occ;
    }

    uint32_t k = 0;
    if (BVH && H.off_bvh_triangles) {
        bvh_walk(sc, H.off_bvh_triangles, rb, limit, occluded, [&](uint32_t first, uint32_t cnt) {
            const TriRec t0 = load_triangle(S, H, first), t1 = load_triangle(S, H, first + 1u);
            double dist = 0.;
            V3 p;
            const bool in0 = triangle_hit(t0, o, d, !occ, dist, p);
            planar(in0, dist);
            if (cnt > 1u) {
                const bool in1 = triangle_hit(t1, o, d, !occ, dist, p);
                planar(in1, dist);
            }
        });
        return occ;
    }
    for (; k + 2u <= H.n_triangles; k += 2u) {
        const TriRec t0 = load_triangle(S, H, k), t1 = load_triangle(S, H, k + 1u);
        double dist = 0.;
        V3 p;
        const bool in0 = triangle_hit(t0, o, d, !occ, dist, p);
        planar(in0, dist);
        const bool in1 = triangle_hit(t1, o, d, !occ, dist, p);
        planar(in1, dist);
        if (__all(occ)) return occ;
    }
    for (; k < H.n_triangles; k++) {
        double dist = 0.;
        V3 p;
        const bool inside = triangle_hit(load_triangle(S, H, k), o, d, !occ, dist, p);
        planar(inside, dist);
    }
    return occ;
}

// geometry.rs:104-109 as the strict normalized() forms it, with the norm it computes handed back: sqrt, then the reciprocal of
// the ROUNDED norm, then three products.
__device__ __forceinline__ V3 normalized_norm(V3 a, double &norm) {
    norm = __builtin_sqrt(dot(a, a));
    const double inv = 1. / norm;
    return scaled(a, (norm > 0.) ? inv : 1.);
}

// One lane per answer, 64 a wave; lanes past the last stay in the wave with their `on` off (a harmless ray they never report).
template <bool BVH, int KIND>
__global__ __launch_bounds__(64) void rm_ranged_kernel_t(const double *__restrict__ scene_blob, RangedArgs q) {
    __shared__ uint32_t bstack[64];
    const SceneView stored = global_scene_view(scene_blob, q.H, bstack);
    const size_t i = (size_t)blockIdx.x * 64u + (threadIdx.x & 63u);
    const bool on = i < (size_t)q.n;
    V3 o = mk(0., 0., 0.), d = mk(0., 0., -1.);
    Range r{0., __builtin_inf()};
    if (KIND == RM_RANGED_CLOSEST || KIND == RM_RANGED_OCCLUDED) {
        if (on) {
            const rm_vec3 ro = q.a[i], rd = q.b[i];
            const rm_range rr = q.ranges[i];
            o = mk(ro.x, ro.y, ro.z);
            d = mk(rd.x, rd.y, rd.z);
            r = Range{rr.t_min, rr.t_max};
        }
        // a caller's ray may be off unit length within the assert: neither the boxes nor the cap of its range (a ray parameter
        // against the reference's t) hold for it, and its wave takes the complete walk (rm_radiance_step.inc)
        const SceneView sc = BVH ? complete_walk_view(stored, __any(on & off_unit(d))) : stored;
        if (KIND == RM_RANGED_OCCLUDED) {
            const bool occ = any_hit_ranged<BVH>(sc, o, d, !on, r);
            if (on) q.out[i] = occ ? 1u : 0u;
        } else {
            Hit h{0., 0u};
            const bool got = closest_hit_ranged<BVH>(sc, o, d, on, r, h);
            // (the index formed again rather than held across the walk: 66 -> 64 registers in the hierarchy kernel, 8 waves a SIMD)
            if (on) store_hit(q, sc, q.hits + ((size_t)blockIdx.x * 64u + (threadIdx.x & 63u)), o, d, h, got);
        }
    } else if (KIND == RM_RANGED_SEGMENTS) {
        const SceneView &sc = stored;                                     // (rays normalised here)
        // from[i] along normalized(to[i] - from[i]), the range [skin, L - skin]; an empty range sees
        bool empty = false;
        if (on) {
            const rm_vec3 fa = q.a[i], fb = q.b[i];
            o = mk(fa.x, fa.y, fa.z);
            double len;
            d = normalized_norm(mk(fb.x, fb.y, fb.z) - o, len);
            r = Range{q.skin, len - q.skin};
            empty = r.hi < r.lo;
        }
        const bool occ = any_hit_ranged<BVH>(sc, o, d, !on | empty, r);
        if (on) q.out[i] = (empty | !occ) ? 1u : 0u;
    } else {
        const SceneView &sc = stored;
        // renderer.rs:166-174 for point i / n_lights and light i % n_lights
        if (on) {
            const size_t pt = i / q.n_lights;
            const uint32_t l = (uint32_t)(i - pt * q.n_lights);
            const rm_vec3 pp = q.a[pt], pn = q.b[pt];
            const V3 point = mk(pp.x, pp.y, pp.z), normal = mk(pn.x, pn.y, pn.z);
            const double *lt = sc.S + sc.H.off_lights + RM_LIGHT_WORDS * l;
            double len;
            d = normalized_norm(mk(lt[0], lt[1], lt[2]) - point, len);                       // :166
            o = point + scaled(normal, (dot(d, normal) < 0.) ? -1e-3 : 1e-3);                  // :168-172 (p - n k == p + n (-k) bit for bit)
            r = Range{0., q.mode == RM_LIGHTS_CLIPPED ? len : __builtin_inf()};
        }
        const bool occ = any_hit_ranged<BVH>(sc, o, d, !on, r);                               // :174
        if (on) q.out[i] = occ ? 0u : 1u;
    }
}

}  // namespace rmquery

using namespace rmquery;

const void *rm_ranged_kernel(int kind, bool bvh) {
    switch (kind) {
    case RM_RANGED_CLOSEST: return bvh ? (const void *)rm_ranged_kernel_t<true, RM_RANGED_CLOSEST> : (const void *)rm_ranged_kernel_t<false, RM_RANGED_CLOSEST>;
    case RM_RANGED_OCCLUDED: return bvh ? (const void *)rm_ranged_kernel_t<true, RM_RANGED_OCCLUDED> : (const void *)rm_ranged_kernel_t<false, RM_RANGED_OCCLUDED>;
    case RM_RANGED_SEGMENTS: return bvh ? (const void *)rm_ranged_kernel_t<true, RM_RANGED_SEGMENTS> : (const void *)rm_ranged_kernel_t<false, RM_RANGED_SEGMENTS>;
    case RM_RANGED_LIGHTS: return bvh ? (const void *)rm_ranged_kernel_t<true, RM_RANGED_LIGHTS> : (const void *)rm_ranged_kernel_t<false, RM_RANGED_LIGHTS>;
    default: return nullptr;
    }
}

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
