// rm_radiance_step.inc -- the radiance ray step, for the kernels that shade rays of their own making: rm_radiance.hip (one lane
// per answer of a ray or sample list) and rm_refine.hip (the samples of the pixels an anti-aliased frame refines).  Included
// behind rm_render_kernel.hpp in a strict-flavour unit, with `using namespace rmdev; using namespace rmdev_strict;` in force.
//
// cast_ray (renderer.rs:254-309) from the render's own pieces (rm_trace.inc): in a step every lane that holds a ray finds its
// closest hit, shades it and turns into the refracted (else the reflected) child; where both exist the reflected one is parked
// on the lane's own stack, and a lane whose ray ended takes its deepest parked ray.  Radiance is linear in the children
// (renderer.rs:219,249), so a ray carries the product of the factors above it.
//
// The loop is wave-uniform: it ends when no lane holds a ray, every block is entered on a vote and predicated inside
// (where<false> of rm_trace.inc), and a lane without a ray walks along with its `on` off -- see rm_radiance.hip, "Divergence".
// How a lane comes by its ray is the including kernel's business; sample_direction below is the one way to form a sample's.
//
// Also here, once, what the including kernels share beside the step: their view of the scene (global_scene_view, rm_query.hip's
// too), the display byte of a mean (to_byte) and the rules of the moved lights (OffsetLights), spheres (OffsetSpheres) and shapes (OffsetShapes).

namespace rmradiance {

// The scene as the kernels outside the render see it: read from global memory (no LDS copy: the rays of a wave gather from all
// over the scene anyway), never narrow (they are compiled without the cull).  `bstack`: the workgroup's 64 words of LDS.
__device__ __forceinline__ SceneView global_scene_view(const double *__restrict__ scene_blob, const rm_dev_header &H, uint32_t *bstack) {
    SceneView sc;
    sc.S = scene_blob;
    sc.G = scene_blob;
    sc.cull_bounds = scene_blob + H.off_bounds;
    sc.cull_planar = scene_blob + H.off_planar;
    sc.bstack = bstack;
    sc.cull_cos = 2.;
    sc.H = H;
    return sc;
}

// A caller's direction is admitted with |d.d - 1| < 1e-4 (include/rusty_marcher_amd.h), and the reference's sphere rule
// (sphere.rs:27-45: tca = L.d, d2 = L.L - tca^2) is a geometric test only where d.d = 1: with d.d = 1 + e a sphere answers as
// one of r^2 + e tca^2, and its t is not the parameter the slab test works in.  The hierarchy's boxes hold the true sphere
// and the pruning distance compares the two, so neither is valid for such a ray: a wave that holds one takes the complete
// walk -- the flat loops over the primitives in leaf order, ties by the list-order keys -- which is what this view selects
// (closest_hit, any_hit and their ranged forms enter a hierarchy only where the header names one).  Wave-uniform: `any_off_unit`
// is a vote.  RM_UNIT_SLACK: normalising in doubles leaves |d.d - 1| below 1e-15; within 1e-14 the boxes' margin of 2e-7 r
// still holds for every sphere wider than 1.6e-4 of its distance (3e-5 for a ray unit to rounding), and the pruning margin
// of 1e-7 is far off.
#define RM_UNIT_SLACK 1e-14
__device__ __forceinline__ bool off_unit(V3 d) { return __builtin_fabs(dot(d, d) - 1.) > RM_UNIT_SLACK; }
__device__ __forceinline__ SceneView complete_walk_view(const SceneView &sc, bool any_off_unit) {
    SceneView v = sc;
    v.H.off_bvh_spheres = any_off_unit ? 0u : sc.H.off_bvh_spheres;
    v.H.off_bvh_triangles = any_off_unit ? 0u : sc.H.off_bvh_triangles;
    return v;
}

__device__ __forceinline__ uint8_t to_byte(double v) {                   // framebuffer.rs:80-82, the render epilogue's rule
    return (uint8_t)(255. * __builtin_fmin(__builtin_fmax(v, 0.), 1.));
}

// Light i of a sample whose lights are moved: the scene's position plus the sample's row of an offset table, rounded once a
// component (the area lights, rm_soft.hip; StoredLights of rm_trace.inc is the rule without).
struct OffsetLights {
    const double *row;                                                   // n_lights x 3 doubles
    __device__ __forceinline__ V3 operator()(const double *lt, uint32_t i) const {
        const double *o = row + 3u * i;
        return mk(lt[0] + o[0], lt[1] + o[1], lt[2] + o[2]);
    }
};

// Device sphere i of a sample whose spheres are moved: the record's centre plus the sample's row of a shape offset table, rounded
// once a component (the moving spheres, rm_motion.hip; StoredSpheres of rm_trace.inc is the rule without).  The table is in the
// order of the scene's shape list and the device order of the spheres need not be (a scene with a sphere hierarchy is permuted):
// the queries' pid map leads from i to the shape, a wave-uniform load in the walks.  `at` is the one place the addition stands.
struct OffsetSpheres {
    static constexpr bool moves = true;
    static constexpr bool swept = false;
    const double *row;                                                   // n_shapes x 3 doubles
    const uint32_t *pid_map;                                             // 2 words a pid; word 0: the shape
    __device__ __forceinline__ V3 at(double cx, double cy, double cz, uint32_t i) const {
        const double *o = row + 3u * pid_map[2u * i];
        return mk(cx + o[0], cy + o[1], cz + o[2]);
    }
    __device__ __forceinline__ SphereRec operator()(const SphereRec &s, uint32_t i) const {
        const V3 c = at(s.cx, s.cy, s.cz, i);
        return SphereRec{c.x, c.y, c.z, s.r2};
    }
    __device__ __forceinline__ V3 centre(const double *sp, uint32_t i) const { return at(sp[0], sp[1], sp[2], i); }
    using Planar = StoredPlanar;                                         // polygons and triangles stand still
    __device__ __forceinline__ Planar planar() const { return Planar(); }
};

// ... and every shape moved (the moving shapes, rm_motion_shapes.hip): the spheres as OffsetSpheres moves them, and a polygon or
// a triangle by the row's entry of its shape -- for a triangle that is its Obj.  polygon.rs:44-49 and triangle.rs:19-24 add the
// offset to the plane point (the centre) and to every vertex and leave the normal alone; the records hold those same quantities
// (x and y of a vertex: the inside test reads no z), so record + offset, rounded once a component, is the reference's moved
// primitive.  The records stay the wave's (scalar operands): a Planar holds only the lane's three offsets of the shape the
// walk is at, and the hit tests form record + offset at each use (StoredPlanar of rm_trace.inc is the rule without).  The pid
// of polygon g is n_spheres + g, of triangle k n_spheres + n_polygons + k; the map word is wave-uniform in the walks, so
// whether the shape changed is a scalar branch: the triangles of a mesh are consecutive and fetch their offset once.
struct OffsetShapes {
    static constexpr bool moves = true;
    static constexpr bool swept = false;
    const double *row;                                                   // n_shapes x 3 doubles
    const uint32_t *pid_map;                                             // 2 words a pid; word 0: the shape
    uint32_t n_spheres, n_polygons;
    __device__ __forceinline__ V3 at(double cx, double cy, double cz, uint32_t i) const {
        const double *o = row + 3u * pid_map[2u * i];
        return mk(cx + o[0], cy + o[1], cz + o[2]);
    }
    __device__ __forceinline__ SphereRec operator()(const SphereRec &s, uint32_t i) const {
        const V3 c = at(s.cx, s.cy, s.cz, i);
        return SphereRec{c.x, c.y, c.z, s.r2};
    }
    __device__ __forceinline__ V3 centre(const double *sp, uint32_t i) const { return at(sp[0], sp[1], sp[2], i); }
    struct Planar {
        const double *row;
        const uint32_t *pid_map;
        uint32_t n_spheres, n_polygons;
        uint32_t shape;                                                  // whose offsets these are; ~0: none yet
        double ox, oy, oz;
        __device__ __forceinline__ void seek(uint32_t pid) {
            const uint32_t k = pid_map[2u * pid];
            if (k != shape) {
                const double *o = row + 3u * k;
                ox = o[0]; oy = o[1]; oz = o[2];
                shape = k;
            }
        }
        __device__ __forceinline__ const Planar &polygon(uint32_t g) { seek(n_spheres + g); return *this; }
        __device__ __forceinline__ const Planar &triangle(uint32_t k) { seek(n_spheres + n_polygons + k); return *this; }
        __device__ __forceinline__ double x(double v) const { return v + ox; }
        __device__ __forceinline__ double y(double v) const { return v + oy; }
        __device__ __forceinline__ double z(double v) const { return v + oz; }
    };
    __device__ __forceinline__ Planar planar() const { return Planar{row, pid_map, n_spheres, n_polygons, ~0u, 0., 0., 0.}; }
};

// ... and the same rule admitted into a swept hierarchy (rm_swept.hip, rm_converge_swept.hip): the scene blob those kernels are
// handed holds boxes refitted to every position the rule can give a primitive (rm_swept.cpp), so closest_hit and any_hit let it
// enter them and apply it inside the leaves.  Nothing else differs.
struct SweptShapes : OffsetShapes {
    static constexpr bool swept = true;
};

#ifdef RM_BOUNCE_ROWS
// The diffuse bounce of a sample (include/rusty_marcher_amd.h, "diffuse bounce"; rm_bounce.hip and rm_converge_bounce.hip alone
// define RM_BOUNCE_ROWS, every other unit sees the tokens it always saw).  What a lane carries into its walk is two words and
// three wave-uniform values: the row's address is formed from `row`, the shift from `pix`; the row itself is fetched where the
// camera ray's hit is shaded, so nothing of it is alive across the first step's walks.
struct Bounce {
    const double *table;                                                 // [rows][2], wave-uniform
    double strength;                                                     // wave-uniform, finite and >= 0 (the host checked)
    double *park;                                                        // the workgroup's 64 x 6 doubles of LDS (radiance_steps)
    uint32_t row;                                                        // the lane's row, inside the table in every lane
    uint32_t pix;                                                        // y * frame_width + x: hashed, never an address
};

// lowbias32
__device__ __forceinline__ uint32_t bounce_hash(uint32_t h) {
    h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
    return h;
}

// Steps 1-3 of the rule for the camera ray `dir` that hit `s`: the bounce ray (o, w) and the weight k of its direction
__device__ __forceinline__ void bounce_ray(const Bounce &b, V3 dir, const Surface &s, V3 &o, V3 &w, double &k) {
    const double *t = b.table + 2u * (size_t)b.row;
    const uint32_t h = bounce_hash(b.pix);
    double x = t[0] + (double)(h & 0xffffu) / 65536.;
    x = x - __builtin_floor(x);
    double y = t[1] + (double)(h >> 16) / 65536.;
    y = y - __builtin_floor(y);
    const double a = 2. * x - 1., c = 2. * y - 1.;
    const double sA = __builtin_sqrt(1. - a * a / 2.), sB = __builtin_sqrt(1. - c * c / 2.);
    const double u = a * sB, v = c * sA;
    const double z = __builtin_sqrt(__builtin_fmax(1. - (u * u + v * v), 0.));
    k = 1.2732395447351628 * (sA * sB - (a * a * c * c) / (4. * sA * sB));
    const V3 N = s.normal;
    const V3 Nf = dot(dir, N) < 0. ? N : neg(N);
    const double sg = Nf.z < 0. ? -1. : 1.;
    const double q = -1. / (sg + Nf.z);
    const double e = Nf.x * Nf.y * q;
    const V3 T = mk(1. + sg * Nf.x * Nf.x * q, sg * e, -sg * Nf.x);
    const V3 B = mk(e, sg + Nf.y * Nf.y * q, -Nf.y);
    w = normalized((scaled(T, u) + scaled(B, v)) + scaled(Nf, z));
    o = s.point + scaled(Nf, 1e-3);
}
#endif

// The un-normalised direction of the sample (sx, sy): renderer.rs:128-135 at a real-valued position, the host's
// backproject_tables operation for operation.  A: an argument block with the params' Renderer (width, height, half_fov,
// ratio) and the context's basis (cam_r*, cam_u*, cam_f*; read where oriented).
template <class A>
__device__ __forceinline__ V3 sample_direction(const A &q, bool oriented, double sx, double sy) {
    const double bx = 2. * (sx / q.width - 0.5) * q.half_fov * q.ratio;
    const double by = -2. * (sy / q.height - 0.5) * q.half_fov;
    return oriented ? mk((bx * q.cam_rx + by * q.cam_ux) + q.cam_fx, (bx * q.cam_ry + by * q.cam_uy) + q.cam_fy,
                         (bx * q.cam_rz + by * q.cam_uz) + q.cam_fz)
                    : mk(bx, by, -1.);
}

// What comes back along the lane's ray (orig, dir), cast as a primary ray (n_recursion = 1) with the cap max_depth >= 1; zero
// for a lane whose `on` is off.  Called by whole waves.  `lights`: where the lane's lights stand at every step of its ray, the
// children's included (rm_trace.inc, StoredLights: as the scene image says).  `spheres`: where the lane's spheres stand, in the
// same way (StoredSpheres).  ADMIT: the rays are the caller's own (rm_radiance_rays): a step whose wave holds a ray that is
// not unit -- the caller's, or a child of it: reflect() keeps the length (optics.rs:4-6) -- finds its closest hit by the
// complete walk (complete_walk_view above).  The shadow rays are normalised and keep the hierarchy.
template <bool BVH, int POW, int STACK, class LIGHTS = StoredLights, class SPHERES = StoredSpheres, bool ADMIT = false>
__device__ __forceinline__ V3 radiance_steps(const SceneView &sc, V3 orig, V3 dir, bool on, const V3 bg, const uint32_t max_depth,
                                             const LIGHTS &lights = LIGHTS(), const SPHERES &spheres = SPHERES()
#ifdef RM_BOUNCE_ROWS
                                             , const Bounce &bounce = Bounce{nullptr, 0., nullptr, 0u, 0u}
#endif
                                             ) {
    double weight = 1.;
    uint32_t depth = 1;                                                  // renderer.rs:83
    V3 acc = mk(0., 0., 0.);
    // Parked rays: a lane works depth-first on one tree, so its parked rays have distinct depths 2 .. max_depth -- at most
    // max_depth - 1 <= STACK of them (the host picks STACK by that rule).
    StackEntry deep[STACK];
    uint32_t n_deep = 0;
#ifdef RM_BOUNCE_ROWS
    // A camera ray whose first hit is not glass has no children, so behind step 1 such a lane's whole tree is the bounce's
    // subtree: the lane turns into the bounce ray with weight strength x diffusion x k at depth 2.  What it had added until then
    // (A: background + direct light of the first hit) and the hit's diffuse colour (tint) it leaves in its own six doubles of
    // LDS -- twelve registers that would be alive across every walk of the subtree otherwise --, begins its sum again, and
    // answers A + tint x sum behind the loop.  A lane reads only what it stored itself: no barrier.  A lane that never
    // bounced returns its sum as every other unit does.  The rays a bounce lane parks have distinct depths 3 .. max_depth,
    // fewer than the max_depth - 1 the stack is sized for.
    bool bounced = false;
    const bool bouncing = bounce.strength != 0.;                         // wave-uniform
    double *parked = bounce.park + 6u * (threadIdx.x & 63u);
#endif

    while (__any(on)) {                                                  // one ray step; the loop itself is wave-uniform
        Hit h{0., 0u};
        // (two calls rather than one on `ADMIT && BVH ? complete_walk_view(...) : sc`: the conditional copies the view in every
        // instantiation, and the objects of the families that do not admit -- refine, lens, accumulate, converge -- then differ)
        bool got;
        if (ADMIT && BVH) got = closest_hit<BVH, false, false>(complete_walk_view(sc, __any(on & off_unit(dir))), orig, dir, on, h, false, 0ull, spheres) & on;
        else got = closest_hit<BVH, false, false>(sc, orig, dir, on, h, false, 0ull, spheres) & on;
        // what this step adds to the lane's answer: weight x (background + direct light) on a hit (renderer.rs:272-275),
        // weight x background where a child leaves the scene (:302-303), nothing where the caller's ray does (:305), + the
        // children beyond the cap (:262-264).  Lanes without a ray add zero.
        V3 L = bg;
        const double w_add = (on & (got | (depth > 1u))) ? weight : 0.;
        double w_cap = 0.;
        bool next = false;                                               // the lane goes on with a child of its ray
#ifdef RM_BOUNCE_ROWS
        double w_bounce_cap = 0.;
        bool bnc = false;
#endif
        if (__any(got)) {
            const Surface s = surface_at<false>(sc, orig, dir, h, got, spheres);
            // renderer.rs:149 as it stands, normalize(origin - point), not the ray's own direction turned round: for a ray that
            // starts ON a surface the two differ -- point == origin gives the zero vector (no specular light at all), and a hit
            // an ulp or two down the ray gives whatever the rounding of origin + dir * t left (tests/test_gpu_second_reading.py)
            L = pick(got, bg + shade_direct<POW, BVH, false, false>(sc, normalized(orig - s.point), s, got, h.pid, lights, spheres), bg);
            const bool glass = got & (s.mat[8] != 0.);                   // is_glass_like, renderer.rs:277
            if (__any(glass)) {
                const double reflection = s.mat[6], ri = s.mat[7], inv_ri = s.mat[9];
                V3 ro, rd, to, td;
                const bool has_r = glass & reflect_child<false>(dir, s, ri, inv_ri, ro, rd);   // renderer.rs:195-222
                const bool has_t = glass & refract_child(dir, s, ri, inv_ri, glass, to, td);   // renderer.rs:225-252
                const double wr = weight * reflection, wt = weight * (1. - reflection);
                const bool capped = depth + 1u > max_depth;              // such a child returns the background
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
#ifdef RM_BOUNCE_ROWS
            bnc = bouncing & got & !glass & (depth == 1u);               // the camera ray's hit alone holds depth 1
            if (__any(bnc)) {
                V3 bo, bw;
                double k;
                bounce_ray(bounce, dir, s, bo, bw, k);
                const double wb = (bounce.strength * s.mat[0]) * k;
                const bool live_b = bnc & !(2u > max_depth);             // beyond the cap the bounce returns the background
                w_bounce_cap = (bnc & !live_b) ? wb : 0.;
                if (bnc) { parked[3] = s.mat[1]; parked[4] = s.mat[2]; parked[5] = s.mat[3]; }
                next = next | live_b;
                orig = pick(live_b, bo, orig);
                dir = pick(live_b, bw, dir);
                weight = live_b ? wb : weight;
                depth += live_b ? 1u : 0u;
            }
#endif
        }
        acc = acc + mk(__builtin_fma(bg.x, w_cap, L.x * w_add), __builtin_fma(bg.y, w_cap, L.y * w_add),
                       __builtin_fma(bg.z, w_cap, L.z * w_add));
#ifdef RM_BOUNCE_ROWS
        if (__any(bnc)) {                                                // the first hit's share is complete: the bounce's sum begins
            if (bnc) { parked[0] = acc.x; parked[1] = acc.y; parked[2] = acc.z; }
            acc = pick(bnc, mk(bg.x * w_bounce_cap, bg.y * w_bounce_cap, bg.z * w_bounce_cap), acc);
            bounced = bounced | bnc;
        }
#endif
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
#ifdef RM_BOUNCE_ROWS
    if (bounced)                                                         // per-lane: the other lanes' slots hold nothing of theirs
        acc = mk(parked[0] + parked[3] * acc.x, parked[1] + parked[4] * acc.y, parked[2] + parked[5] * acc.z);
#endif
    return acc;
}

}  // namespace rmradiance

// The instantiations every family of these kernels carries, written once: without and with a hierarchy, 4 or 32 parked rays a
// lane (rm_plan.cpp rm_shading_variant_of never asks for another), each with both powers.  In a picker of (bool bvh, int
// pow_mode, int stack), RM_SHADING_TABLE(RM_SHADING_KERNEL, K) returns the K<BVH, POW, STACK> that matches and falls through
// where none does.  A family with a template argument more hands the table a macro of its own that forms a row's kernel from
// RM_SHADING_KERNEL(K, B, S, the argument): the kernels of a row then stay together in the object, as they always have.
#define RM_SHADING_KERNEL(K, B, S, ...)                                                                   \
    (pow_mode == POW_INTEGER ? (const void *)K<B, POW_INTEGER, S, ##__VA_ARGS__> : (const void *)K<B, POW_GENERIC, S, ##__VA_ARGS__>)
#define RM_SHADING_TABLE(ROW, K)                                                                          \
    if (!bvh && stack == 4) return ROW(K, false, 4);                                                      \
    if (!bvh && stack == 32) return ROW(K, false, 32);                                                    \
    if (bvh && stack == 4) return ROW(K, true, 4);                                                        \
    if (bvh && stack == 32) return ROW(K, true, 32);
