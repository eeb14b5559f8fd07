// rm_trace.inc -- device functions of the render path (gfx950, FP64).
//
// What each function replaces in the reference (engine/src):
//   closest_hit   : find_closest_intersect (shapes.rs:110-143) over
//                   Sphere::intersect (sphere.rs:27-61), ConvexPolygon::intersect
//                   (polygon.rs:60-98), Obj/Triangle::intersect (obj.rs:185-221,
//                   triangle.rs:49-83)
//   any_hit       : intersect_shape_set (shapes.rs:92-108)
//   shade_direct  : direct_lighting + diffusion_factor + specular_factor
//                   (renderer.rs:138-193)
//   reflect_child / refract_child : reflect_ray / refract_ray (optics.rs:8-89)
//
// Execution model.  Every lane owns one ray -- or none: the render loop is WAVE-UNIFORM
// and all 64 lanes execute every instruction; a lane without a ray (or a lane the current
// step does not concern) is switched off by a predicate that feeds selects, never by a
// divergent branch.  Branches are taken on wave votes only.  That keeps the scalar unit
// out of the inner loops (a divergent branch costs EXEC bookkeeping on it), makes the wave
// votes, lane reads and reductions below well defined, and lets idle lanes take over parked
// rays of other lanes (rm_render_kernel.inc).  Lanes that are switched off compute on
// whatever their registers hold; nothing they compute is stored or voted on.
//
// All lanes of a wave walk the same primitive list (wave-uniform loop counters, records
// fetched with scalar loads); the per-lane state is the ray and the best hit so far.
// Arithmetic is IEEE binary64 in the reference's operation order; the file is compiled
// without FMA contraction unless the build says otherwise.
//
// This file has no include guard: rm_render_kernel.hpp includes it once per numeric
// flavour, with RM_FLAVOR_NS / RM_FAST defined and the matching
// `#pragma clang fp contract(..)` in effect:
//   rmdev_strict  every multiply and add separately rounded, sqrt then divide, closest
//                 hit ordered by |p - o|^2 -- the reference's operations in its order;
//   rmdev_fast    FMA contraction, rsqrt-based normalisation, closest hit ordered by t,
//                 viewer direction taken from the ray.  Exact zeros survive all of these
//                 (0 * x = 0, fma of exact products is exact), which is what keeps the
//                 reference's on-edge decisions on symmetry axes intact.
namespace RM_FLAVOR_NS {
using namespace rmdev;


struct V3 { double x, y, z; };

__device__ __forceinline__ V3 mk(double x, double y, double z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(V3 a, V3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ V3 neg(V3 a) { return mk(-a.x, -a.y, -a.z); }
__device__ __forceinline__ V3 scaled(V3 a, double s) { return mk(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ V3 pick(bool c, V3 a, V3 b) { return mk(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z); }
// geometry.rs:180-182: (x*x' + y*y') + z*z'
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
#ifndef RM_CHECKED
#define RM_CHECKED 0
#endif
// RM_CHECKED (rm_render_kernel.hpp: the strict plain-walk kernels' tile body): a lane's "an operand lay outside the range the
// range-free sequences below are proven for" travels with the calls; the tile is rendered again by the exact code if any is set.
#if RM_CHECKED
#define RM_SUS_PARAM , bool &sus
#define RM_SUS_ARG , sus
#else
#define RM_SUS_PARAM
#define RM_SUS_ARG
#endif
#if RM_CHECKED
// The compiler's own expansion of a binary64 square root (v_rsq_f64, g = x y, h = y / 2, one coupled refinement of both, two
// residual corrections of g) without what it puts around it for x < 2^-767 -- a compare, two selects, two v_ldexp_f64 that
// scale by 2^256 and back.  The same operations on the same values: for x >= 2^-767 bit for bit the compiler's root.
// `h`: ~ 0.5 / sqrt(x) as the iteration leaves it.
__device__ __forceinline__ double sqrt_unscaled(double x, double &h) {
    const double y = __builtin_amdgcn_rsq(x);
    const double g0 = x * y, h0 = y * 0.5;
    const double r0 = __builtin_fma(-h0, g0, 0.5);
    const double g1 = __builtin_fma(g0, r0, g0), h1 = __builtin_fma(h0, r0, h0);
    const double d0 = __builtin_fma(-g1, g1, x);
    const double g2 = __builtin_fma(d0, h1, g1);
    const double d1 = __builtin_fma(-g2, g2, x);
    h = h1;
    return __builtin_fma(d1, h1, g2);
}
// ... with the compiler's select for 0, -0 and +inf (the root of a tangent ray's discriminant is exactly 0).  The argument is
// r^2 - d^2 of a sphere test: not below r^2 2^-54 unless it is zero, and the upload keeps r^2 within [2^-600, 2^600]
// (rm_image.cpp scene_exact_only) -- no lane needs a guard.
__device__ __forceinline__ double sqrt_discriminant(double x) {
    double h;
    const double r = sqrt_unscaled(x, h);
    return (x == 0. || x == __builtin_inf()) ? x : r;
}
#define RM_SQRT_DISCRIMINANT(x) sqrt_discriminant(x)
// The range the checked normalisation is proven for, with margin: the root needs x >= 2^-767; the division's scaling sets in
// for divisors beyond about 2^+-768, far outside the norms 2^-300 .. 2^300 of this range.
#define RM_CHECKED_X_MIN 0x1p-600
#define RM_CHECKED_X_MAX 0x1p+600
struct CheckedNorm { double norm, inv; bool outside; };
// sqrt, then 1 / norm of the ROUNDED norm (geometry.rs:104-109): the compiler's own expansion of the division (v_rcp_f64, two
// Newton steps, the quotient's residual correction) without what it puts around it for operands near the ends of the
// exponent range -- two v_div_scale_f64, which leave a divisor within [2^-300, 2^300] and the dividend 1 as they are,
// v_div_fmas_f64, which is then a plain fma, and v_div_fixup_f64, which passes such a quotient through.  The same operations
// on the same values: bit for bit the compiler's quotient.  Everything outside the range (NaN, the zero vector) is `outside`.
// (Seeding the reciprocal with h + h from the root's iteration instead of v_rcp_f64 -- one Newton step less, no second
// transcendental -- was built first and is NOT bit-identical: it rounds 1 / norm the other way for every norm whose
// significand is all ones, and that is the norm of every nearly unit vector whose squared length falls an ulp or two short
// of 1 -- the refracted directions: DESIGN.md section 4.)
__device__ __forceinline__ CheckedNorm checked_norm(double x) {
    CheckedNorm c;
    double h;
    c.norm = sqrt_unscaled(x, h);
    const double y0 = __builtin_amdgcn_rcp(c.norm);
    const double y1 = __builtin_fma(y0, __builtin_fma(-c.norm, y0, 1.), y0);
    const double y2 = __builtin_fma(y1, __builtin_fma(-c.norm, y1, 1.), y1);
    c.inv = __builtin_fma(__builtin_fma(-c.norm, y2, 1.), y2, y2);
    c.outside = !((x >= RM_CHECKED_X_MIN) & (x <= RM_CHECKED_X_MAX));              // (NaN and the zero vector: outside)
    return c;
}
#else
#define RM_SQRT_DISCRIMINANT(x) __builtin_sqrt(x)
#endif
// geometry.rs:104-109: multiply by the reciprocal of the norm
// (RM_CHECKED: `on` -- the lanes whose vector is a ray's; the others' flags do not count)
#if RM_CHECKED
__device__ __forceinline__ V3 normalized(V3 a, bool on, bool &sus) {
    const CheckedNorm c = checked_norm(dot(a, a));
    sus = sus | (on & c.outside);
    return scaled(a, (c.norm > 0.) ? c.inv : 1.);
}
#define RM_NORMALIZED(a, on) normalized(a, on, sus)
#else
__device__ __forceinline__ V3 normalized(V3 a) {
#if RM_FAST
    // 1/sqrt(x) from the hardware estimate (v_rsq_f64, ~26 bits) and two Newton steps,
    // instead of a correctly rounded sqrt followed by a correctly rounded division
    // (~15 instead of ~30 instructions; |rel. error| ~1e-16; squared norms are assumed
    // to lie in [1e-280, 1e280]).
    const double x = dot(a, a);
    double y = __builtin_amdgcn_rsq(x);
    const double h = 0.5 * x;
    y = y * (1.5 - h * y * y);
    y = y * (1.5 - h * y * y);
    return scaled(a, (x > 0.) ? y : 1.);          // a zero vector stays itself (x * 1 is exact)
#else
    const double norm = __builtin_sqrt(dot(a, a));
    const double inv = 1. / norm;
    return scaled(a, (norm > 0.) ? inv : 1.);     // `if norm > 0` of the reference: else the vector itself (x * 1 is exact)
#endif
}
#define RM_NORMALIZED(a, on) normalized(a)
#endif

// Scene view: S points at the blob (LDS copy), H carries counts and offsets in SGPRs.
struct SceneView {
    const double *S;                  // per-lane gathers: LDS copy, or the blob itself
    const double *__restrict__ G;     // wave-uniform walks: the blob in global memory (scalar loads)
    const double *cull_bounds;        // the bundle cull's arrays: every primitive's bounding sphere (4 words) ...
    const double *cull_planar;        // ... and the planar primitives' lifted vertices (16 words): in the blob, or packed into the wave's LDS block (cull_stage)
    uint32_t *bstack;                 // this wave's hierarchy stack in LDS (64 entries)
    double cull_cos;                  // ray bundles at least this narrow (cosine of the half-angle) cull primitives
    rm_dev_header H;
#ifdef RM_EXP_STAMPS
    uint32_t *cnt;                    // diagnostic build: [0] cull steps [1] candidates kept [2] wide bundles [3] narrow bundles
#endif
};
// (RM_EXP_WALKSTATS, with the stamps: the four counters hold the hierarchy walks' figures instead -- [0] walks [1] nodes visited
// [2] primitives tested in leaves [3] lanes whose ray meets a child box, summed over the nodes)
// (RM_EXP_PHASES, with the stamps: the counters hold 100 MHz ticks instead -- [0] in closest_hit [1] in any_hit / any_hit2
// [2] from the wave's start to its first ray step [3] in shade_direct, the shadow walks included)
#if defined(RM_EXP_STAMPS) && !defined(RM_EXP_WALKSTATS) && !defined(RM_EXP_PHASES) && !defined(RM_EXP_STARTUP)
#define RM_COUNT(sc, i, v) do { (sc).cnt[i] += (v); } while (0)
#else
#define RM_COUNT(sc, i, v) do {} while (0)
#endif
#if defined(RM_EXP_STAMPS) && defined(RM_EXP_WALKSTATS)
#define RM_WCOUNT(sc, i, v) do { (sc).cnt[i] += (v); } while (0)
#else
#define RM_WCOUNT(sc, i, v) do {} while (0)
#endif
#if defined(RM_EXP_STAMPS) && defined(RM_EXP_PHASES)
#define RM_PHASE_T() __builtin_amdgcn_s_memrealtime()
#define RM_PHASE_ADD(sc, i, t0) do { (sc).cnt[i] += (uint32_t)(__builtin_amdgcn_s_memrealtime() - (t0)); } while (0)
#else
#define RM_PHASE_T() 0ull
#define RM_PHASE_ADD(sc, i, t0) do { (void)(t0); } while (0)
#endif

__device__ __forceinline__ uint32_t prim_key(const SceneView &sc, uint32_t pid) {
    const uint32_t *keys = reinterpret_cast<const uint32_t *>(sc.S + sc.H.off_keys);
    return keys[pid];
}

// shapes.rs:130 / obj.rs:198: `!hit || dist_hit < dist_closest`, first in list
// order wins an exact tie.  Primitives are visited grouped by kind (or in any order at
// all: hierarchy, culling), so an exact tie consults the list-order keys unless grouping
// preserved the list order AND the walk visits in ascending pid order.
// Written with bitwise bool ops: the result feeds selects, not branches.
template <bool ORDERED_WALK>
__device__ __forceinline__ bool closer(const SceneView &sc, bool valid, bool hit, double d, double best, uint32_t pid,
                                       uint32_t best_pid) {
    bool take = valid & (!hit | (d < best));
    if (!(ORDERED_WALK && sc.H.list_ordered)) {                       // wave-uniform
        const bool tie = valid & hit & (d == best);
        if (__any(tie)) take = take | (tie & (prim_key(sc, tie ? pid : 0u) < prim_key(sc, tie ? best_pid : 0u)));
    }
    return take;
}

struct Hit {
    double t;       // ray parameter of the closest hit (point = orig + dir * t)
    uint32_t pid;   // device primitive id
};

// ---- wave-level helpers (all 64 lanes execute) -----------------------------------------
__device__ __forceinline__ double lane_f64(double v, uint32_t lane) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, (int)lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), (int)lane);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_f32(float x) {
    // lanes whose source is out of range keep their own value (bound_ctrl off, old = x)
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, x), __builtin_bit_cast(int, x),
                                                                 CTRL, ROW_MASK, 0xf, false));
}
// min / max over the 64 lanes (idempotent: overlapping partial results are harmless);
// row_shr 1, 2, 4, 8 leave each row's result in its lane 15, row_bcast 15 / 31 carry it on
__device__ __forceinline__ float wave_min_f32(float x) {
    x = __builtin_fminf(x, dpp_f32<0x111, 0xf>(x));
    x = __builtin_fminf(x, dpp_f32<0x112, 0xf>(x));
    x = __builtin_fminf(x, dpp_f32<0x114, 0xf>(x));
    x = __builtin_fminf(x, dpp_f32<0x118, 0xf>(x));
    x = __builtin_fminf(x, dpp_f32<0x142, 0xa>(x));
    x = __builtin_fminf(x, dpp_f32<0x143, 0xc>(x));
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
}
__device__ __forceinline__ float wave_max_f32(float x) { return -wave_min_f32(-x); }

// How a per-lane condition guards a block.  Kernels WITH the bundle cull keep all 64 lanes
// executing down to the walks (a cull step needs every lane: lane k tests primitive k), so
// a block is entered on a wave vote and the lanes it does not concern are switched off by
// predicates inside.  Kernels WITHOUT it (scenes of a few primitives) branch per lane, as a
// recursion would: inside the block the predicate is known to be true, the compiler folds
// it away and updates values in place under the execution mask instead of through selects
// (measured on the demo scene: 83 us against 94 us for the all-predicated form).
template <bool DIV>
__device__ __forceinline__ bool where(bool p) { return DIV ? p : (bool)__any(p); }

// ---- primitive records as the loops read them ------------------------------------
// The loops below are wave-uniform: the records are fetched with scalar loads into
// SGPRs and feed the FP64 ops as scalar operands.  A scalar load costs a full round
// trip to the scalar cache per dependent use, so records are fetched in BATCHES -- four
// spheres, a polygon header together with its first four vertices, two triangles --
// and one wait covers the whole batch.
struct SphereRec { double cx, cy, cz, r2; };
struct Vert2 { double x, y; };
struct PolyRec { double nx, ny, nz, px, py, pz; uint32_t first, nv; Vert2 q[4]; };
struct TriRec { double nx, ny, nz, cx, cy, cz, ax, ay, bx, by, ex, ey; };

__device__ __forceinline__ SphereRec load_sphere(const double *__restrict__ S, const rm_dev_header &H, uint32_t i) {
    const double *sp = S + H.off_spheres + RM_SPHERE_WORDS * i;
    return SphereRec{sp[0], sp[1], sp[2], sp[3]};
}

// Where device sphere i stands, given its record.  The default is the record's own centre; a kernel whose samples move their
// spheres (rm_motion.hip) hands closest_hit, any_hit, any_hit2, surface_at and shade_direct another rule.  `operator()` serves
// the walks (a record fetched by a wave-uniform index), `centre` the normal (the lane's own hit): one rule forms both, so the
// normal sees the centre the hit test saw.  Nothing else in those five reads a sphere's position but the hierarchy's boxes, the
// bundle cull and the occluder masks, which hold for the stored centres: such a kernel runs without the three.
//
// Where a planar primitive stands, in the same way: a walk asks the rule for a `Planar` (planar()), points it at the polygon or
// the triangle it is about to test (polygon(g), triangle(k): device indices; they return the Planar as it then stands, which
// the walk hands to the hit test as it is) and the hit tests read every coordinate of the record through it -- x, y, z of the
// plane point or the centre, x and y of a vertex, the pool's vertices too.  StoredPlanar is the identity: the record as the
// scene image says, and what every kernel but the moving shapes' (rm_motion_shapes.hip) walks with.
struct StoredPlanar {
    __device__ __forceinline__ StoredPlanar polygon(uint32_t) const { return StoredPlanar(); }
    __device__ __forceinline__ StoredPlanar triangle(uint32_t) const { return StoredPlanar(); }
    __device__ __forceinline__ double x(double v) const { return v; }
    __device__ __forceinline__ double y(double v) const { return v; }
    __device__ __forceinline__ double z(double v) const { return v; }
};
struct StoredSpheres {
    static constexpr bool moves = false;
    static constexpr bool swept = false;                                 // (a rule that moves may enter a swept hierarchy: rm_swept.hip)
    using Planar = StoredPlanar;
    __device__ __forceinline__ SphereRec operator()(const SphereRec &s, uint32_t) const { return s; }
    __device__ __forceinline__ V3 centre(const double *sp, uint32_t) const { return mk(sp[0], sp[1], sp[2]); }
    __device__ __forceinline__ Planar planar() const { return Planar(); }
};
__device__ __forceinline__ PolyRec load_polygon(const double *__restrict__ S, const rm_dev_header &H, uint32_t i) {
    const double *pg = S + H.off_polygons + RM_POLYGON_WORDS * i;
    const uint32_t *u = reinterpret_cast<const uint32_t *>(pg + 6);
    return PolyRec{pg[0], pg[1], pg[2], pg[3], pg[4], pg[5], u[0], u[1],
                   {{pg[8], pg[9]}, {pg[10], pg[11]}, {pg[12], pg[13]}, {pg[14], pg[15]}}};
}
__device__ __forceinline__ Vert2 load_vertex(const double *__restrict__ S, const rm_dev_header &H, uint32_t v) {
    const double *pv = S + H.off_pverts + RM_PVERT_WORDS * v;
    return Vert2{pv[0], pv[1]};
}
__device__ __forceinline__ TriRec load_triangle(const double *__restrict__ S, const rm_dev_header &H, uint32_t i) {
    const double *t = S + H.off_triangles + RM_TRIANGLE_WORDS * i;
    return TriRec{t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], t[9], t[10], t[11]};
}

// sphere.rs:27-61 up to the discriminant: tca and d2 for one sphere.  `line` and its square
// depend on the ray's ORIGIN only: two rays from one point share them (any_hit2).
struct SphereFrom { V3 line; double ll; };
__device__ __forceinline__ SphereFrom sphere_from(const SphereRec &s, V3 o) {
    SphereFrom f;
    f.line = mk(s.cx - o.x, s.cy - o.y, s.cz - o.z);
    f.ll = dot(f.line, f.line);
    return f;
}
__device__ __forceinline__ void sphere_setup(const SphereFrom &f, V3 d, double &tca, double &d2) {
    tca = dot(f.line, d);
    d2 = f.ll - tca * tca;
}
__device__ __forceinline__ void sphere_setup(const SphereRec &s, V3 o, V3 d, double &tca, double &d2) {
    sphere_setup(sphere_from(s, o), d, tca, d2);
}

// polygon.rs:60-98: plane hit + 2-D inside test (polygon.rs:54-56: only the z of
// (v_i - p) x (v_{i+1} - p), i.e. x and y of the vertices).  `q` holds the first four
// vertices of the polygon (they travel in its record; the rest come from the vertex pool).
// `on`: the lanes this test concerns.
// `num` = (plane point - origin) . normal depends on the ray's origin only (any_hit2).
__device__ __forceinline__ double plane_num(double px, double py, double pz, double nx, double ny, double nz, V3 o) {
    return dot(mk(px - o.x, py - o.y, pz - o.z), mk(nx, ny, nz));
}
// `at`: where the polygon stands (StoredPlanar: as the record says); a caller that forms `num` itself forms it from at's point.
template <class AT = StoredPlanar>
__device__ __forceinline__ bool polygon_hit_num(const double *__restrict__ S, const rm_dev_header &H, const PolyRec &g,
                                                const Vert2 (&q)[4], double num, V3 o, V3 d, bool on, double &dist, V3 &p,
                                                const AT at = AT()) {
    const V3 n = mk(g.nx, g.ny, g.nz);
    const double dotprod = dot(d, n);
    // :66 parallel, :71-76 `dist = num / dotprod; if dist < 0 -> None`.  The quotient is
    // negative exactly when the signs differ (|dotprod| <= 1, so no underflow to -0 while
    // |num| > 1e-300): such lanes are rejected before the division and the edge tests,
    // and a wave whose lanes are all rejected skips them altogether.
    bool alive = on & !(dotprod == 0.) & !(((num < -1e-300) & (dotprod > 0.)) | ((num > 1e-300) & (dotprod < 0.)));
    if (!__any(alive)) return false;
    dist = num / dotprod;
    alive = alive & !(dist < 0.);
    p = o + scaled(d, dist);
    const double x0 = at.x(q[0].x) - p.x, y0 = at.y(q[0].y) - p.y;
    const double x1 = at.x(q[1].x) - p.x, y1 = at.y(q[1].y) - p.y;
    const double x2 = at.x(q[2].x) - p.x, y2 = at.y(q[2].y) - p.y;
    alive = alive & (x0 * y1 - y0 * x1 > 0.);
    if (!__any(alive)) return false;                                  // the whole wave is outside edge 0
    alive = alive & (x1 * y2 - y1 * x2 > 0.);
    if (g.nv == 3u) {
        alive = alive & (x2 * y0 - y2 * x0 > 0.);
    } else {
        double ax = at.x(q[3].x) - p.x, ay = at.y(q[3].y) - p.y;
        alive = alive & (x2 * ay - y2 * ax > 0.);
        for (uint32_t e = 4; e < g.nv; e++) {                         // pentagons and up
            const Vert2 v = load_vertex(S, H, g.first + e);
            const double bx = at.x(v.x) - p.x, by = at.y(v.y) - p.y;
            alive = alive & (ax * by - ay * bx > 0.);
            ax = bx; ay = by;
        }
        alive = alive & (ax * y0 - ay * x0 > 0.);
    }
    return alive;
}

template <class AT = StoredPlanar>
__device__ __forceinline__ bool polygon_hit(const double *__restrict__ S, const rm_dev_header &H, const PolyRec &g,
                                            const Vert2 (&q)[4], V3 o, V3 d, bool on, double &dist, V3 &p, const AT at = AT()) {
    return polygon_hit_num(S, H, g, q, plane_num(at.x(g.px), at.y(g.py), at.z(g.pz), g.nx, g.ny, g.nz, o), o, d, on, dist, p, at);
}

// triangle.rs:49-83; `at` as polygon_hit_num's
template <class AT = StoredPlanar>
__device__ __forceinline__ bool triangle_hit_num(const TriRec &t, double num, V3 o, V3 d, bool on, double &dist, V3 &p,
                                                 const AT at = AT()) {
    const V3 n = mk(t.nx, t.ny, t.nz);
    const double dotprod = dot(d, n);
    // :57 parallel, :62-67 going away -- same early sign test as polygon_hit
    bool alive = on & !(__builtin_fabs(dotprod) < 1e-6) &
                 !(((num < -1e-300) & (dotprod > 0.)) | ((num > 1e-300) & (dotprod < 0.)));
    if (!__any(alive)) return false;
    dist = num / dotprod;
    alive = alive & !(dist < 0.);
    p = o + scaled(d, dist);
    const double ax = at.x(t.ax) - p.x, ay = at.y(t.ay) - p.y;
    const double bx = at.x(t.bx) - p.x, by = at.y(t.by) - p.y;
    const double cx = at.x(t.ex) - p.x, cy = at.y(t.ey) - p.y;
    alive = alive & (ax * by - ay * bx > 0.);
    if (!__any(alive)) return false;
    alive = alive & (bx * cy - by * cx > 0.);
    alive = alive & (cx * ay - cy * ax > 0.);
    return alive;
}
template <class AT = StoredPlanar>
__device__ __forceinline__ bool triangle_hit(const TriRec &t, V3 o, V3 d, bool on, double &dist, V3 &p, const AT at = AT()) {
    return triangle_hit_num(t, plane_num(at.x(t.cx), at.y(t.cy), at.z(t.cz), t.nx, t.ny, t.nz, o), o, d, on, dist, p, at);
}

// ---- ray bundles: which primitives can the rays of this wave reach at all? ---------------
// The 64 rays of a wave are usually a narrow bundle: the primary rays of a 16x4 tile leave
// one point within a fraction of a degree of each other; the shadow rays of a tile all pass
// (within the 1e-3 surface offset) through the light.  Such a bundle is enclosed in a cone
// (apex ball A +- rho, unit axis u, half-angle theta), and before a walk the LANES TEST
// THE PRIMITIVES, one primitive per lane, 64 per step: bounding sphere against cone, about
// twenty instructions for 64 primitives, one ballot.  Only the primitives of the resulting
// mask are then tested ray by ray, with exactly the tests of the plain walk -- the cull only
// decides WHICH primitives are tested, and its margins (1e-7 relative, far beyond the
// rounding of any of the tests) make sure every primitive some ray could hit is among them.
// The reference computes a bounding box per shape and never uses it (shapes.rs:34-86).
// Wide bundles (incoherent secondary rays) fall back to the plain walk / the hierarchy.
struct Bundle {
    double ax, ay, az;      // apex
    double ux, uy, uz;      // axis (unit, a ray direction)
    double cos2, sin_t;     // of the half-angle, rounded towards a wider cone
    double chord;           // |w - u| <= chord for every direction w of the bundle (2 sin(theta/2), rounded up)
    double rho;             // every ray line passes within rho of the apex
    bool two_sided;         // the rays run TOWARDS the apex and beyond (shadow rays through the light)
    bool narrow;            // usable
};

// Cone over the directions `d` of the lanes `part` around the direction of one of them.
__device__ __forceinline__ void bundle_cone(Bundle &b, V3 d, bool part, uint32_t ref, double cull_cos) {
    b.ux = lane_f64(d.x, ref); b.uy = lane_f64(d.y, ref); b.uz = lane_f64(d.z, ref);
    const double c = __builtin_fma(d.z, b.uz, __builtin_fma(d.y, b.uy, d.x * b.ux));
    // single precision is enough for the angle (1 - cos resolves 6e-8: 3.5e-4 rad) as long
    // as it errs towards the wider cone
    // (a ray that is not a number "hits" in the reference's tests, sphere.rs:37 -- no cone holds it)
    const float cf = wave_min_f32(part ? ((c == c) ? (float)c - 2.4e-7f : -2.f) : 1.f);
    const double cm = (double)cf;
    b.narrow = cm >= cull_cos;
    b.cos2 = cm * cm;
    const double s2 = __builtin_fmax((1. - cm) * (1. + cm), 0.);
    b.sin_t = (double)__builtin_sqrtf((float)s2) * (1. + 1e-6) + 1e-7;
    b.chord = (double)__builtin_sqrtf((float)__builtin_fmax(2. * (1. - cm), 0.)) * (1. + 1e-6) + 1e-7;
}

// The lane whose ray serves as the cone's axis: one in the middle of the 16x4 tile when it takes
// part (lane 27: column 11, row 1 -- the cone around it is half as wide as around a corner
// ray), else the first that does.
__device__ __forceinline__ uint32_t axis_lane(bool part) {
    const unsigned long long m = __ballot(part);
    return ((m >> 27) & 1ull) ? 27u : (uint32_t)__builtin_ctzll(m | (1ull << 63));
}

// Rays with origins of their own (primary rays: all at the camera; secondary rays).
__device__ __forceinline__ Bundle bundle_of_rays(V3 o, V3 d, bool part, double cull_cos) {
    Bundle b;
    const uint32_t ref = axis_lane(part);
    b.ax = lane_f64(o.x, ref); b.ay = lane_f64(o.y, ref); b.az = lane_f64(o.z, ref);
    const double ex = o.x - b.ax, ey = o.y - b.ay, ez = o.z - b.az;
    const double e2 = __builtin_fma(ez, ez, __builtin_fma(ey, ey, ex * ex));
    const float r2 = wave_max_f32(part ? ((e2 == e2) ? (float)e2 * (1.f + 2.4e-7f) : __builtin_inff()) : 0.f);
    b.rho = (double)__builtin_sqrtf(r2) * (1. + 1e-6);
    b.two_sided = false;
    bundle_cone(b, d, part, ref, cull_cos);
    return b;
}

// Rays that all pass within `rho` of the point `apex`, running towards it (shadow rays).
__device__ __forceinline__ Bundle bundle_through(V3 apex, double rho, V3 d, bool part, double cull_cos) {
    Bundle b;
    const uint32_t ref = axis_lane(part);
    b.ax = apex.x; b.ay = apex.y; b.az = apex.z;
    b.rho = rho;
    b.two_sided = true;
    bundle_cone(b, d, part, ref, cull_cos);
    return b;
}

// One step of the cull: lane k tests primitive base + k against the bundle.
//
// (1) Bounding sphere (4 words per pid at off_bounds: centre, radius -- inflated on the host).
// A sphere (C, R) meets the solid double cone iff q cos(theta) - |h| sin(theta) <= R, with
// h = (C - A).u and q the distance of C from the axis; squared, no root.  One-sided bundles
// also drop what lies wholly behind the apex.  NaN anywhere keeps the primitive.
//
// (2) Planar primitives (triangles, polygons of up to four vertices; 16 words per primitive
// at off_planar: the vertices LIFTED onto the plane the hit test uses, and their count) are
// large and mostly seen at a slant -- the walls of a box: the sphere around one is hit by
// bundles that pass far from it.  A ray from the apex A hits the primitive only if its
// direction lies inside the pyramid spanned by A and the edges; if for ONE edge every
// direction of the cone lies on the outer side of the plane through A and that edge, no ray
// of the bundle hits it.  With n = (v_i - A) x (v_j - A), oriented by the centroid, that is
// n.w / |n| < 0 for all w, which n.u / |n| + chord < 0 guarantees.  Rays that start up to rho
// off the apex can still reach across the plane, but only within rho / margin of A: the
// primitive must be farther than that.  Two-sided bundles (lines through the apex) need an
// edge for each of the two directions.  About 90 instructions for 64 primitives; compiled
// into the kernels for scenes with several planar primitives only (EDGES: its registers cost
// the sphere-only steps of other scenes 25 %).
#define RM_CULL_TAIL 3u

// Bounding sphere (centre, radius at bp[0..1]) against the bundle: true = no ray of the bundle
// reaches it.  vx.. = centre - apex and vv = its square are handed back for the edge test.
struct SphereCull { double vx, vy, vz, vv, r; bool out; };
__device__ __forceinline__ SphereCull cull_sphere(const double2 *bp, const Bundle &b) {
    SphereCull c;
    const double2 c01 = bp[0], c23 = bp[1];
    c.vx = c01.x - b.ax; c.vy = c01.y - b.ay; c.vz = c23.x - b.az;
    c.r = c23.y;
    const double rr = c23.y + b.rho;
    const double h = __builtin_fma(c.vz, b.uz, __builtin_fma(c.vy, b.uy, c.vx * b.ux));
    c.vv = __builtin_fma(c.vz, c.vz, __builtin_fma(c.vy, c.vy, c.vx * c.vx));
    const double q2 = __builtin_fmax(__builtin_fma(-h, h, c.vv), 0.);
    const double t = __builtin_fma(__builtin_fabs(h), b.sin_t, rr);
    c.out = (q2 * b.cos2 > t * t * (1. + 1e-9)) | (!b.two_sided & (h < -rr)) | (c23.y < 0.);   // radius -1: never hit (upload)
    return c;
}

// The primitives of a cull step (64 consecutive pids -- neighbours in space where the upload
// stores a kind in the leaf order of its hierarchy) have a bounding sphere of their own
// (off_groups), and a first step tests those, lane g the g-th: only the steps whose group some
// ray of the bundle can reach are taken at all.  Scenes of three steps and more (measured: one
// group around the whole Cornell box, tested before its one step, costs 3 % -- 69.0 against
// 67.1 us: the tiles that see nothing still look at the box's bounding sphere; the four groups
// of the 256-sphere scene save one step in five, 1,410 -> 1,400 us).
__device__ __forceinline__ unsigned long long cull_groups(const SceneView &sc, const Bundle &b, uint32_t n_groups) {
    const uint32_t g = threadIdx.x & 63u;
    const bool in = g < n_groups;
    const double2 *bp = reinterpret_cast<const double2 *>(sc.G + sc.H.off_groups) + 2u * (in ? g : 0u);
    return __ballot(in & !cull_sphere(bp, b).out);
}

// The edge test of one planar primitive against the bundle (see (2) above): true = some edge plane
// through the apex has every direction of the bundle on its outer side.  `pp`: the primitive's
// 16-word record at off_planar; sph: what cull_sphere left of its bounding sphere.  `nv == 4` may
// differ from lane to lane (lane per primitive) or be the same for all (lane per bundle).
// (in two halves -- the first three edges, the fourth where some lane's primitive has one -- so that two primitives' tests can
// run side by side in one stretch of code: the classification's chains, rm_classify.inc)
struct EdgeCull { V3 e0, e3; double vx, vy, vz, dist, far; uint32_t nv; bool plus, minus; };
__device__ __forceinline__ void cull_edge(EdgeCull &c, const Bundle &b, V3 p, V3 q) {
    const V3 nrm = mk(p.y * q.z - p.z * q.y, p.z * q.x - p.x * q.z, p.x * q.y - p.y * q.x);
    const double n2 = __builtin_fma(nrm.z, nrm.z, __builtin_fma(nrm.y, nrm.y, nrm.x * nrm.x));
    const double inv = __builtin_amdgcn_rsq(n2);                            // ~26 bits: the margins are 1e-7
    const double side = __builtin_fma(nrm.z, c.vz, __builtin_fma(nrm.y, c.vy, nrm.x * c.vx));   // the centroid's side
    double sn = __builtin_fma(nrm.z, b.uz, __builtin_fma(nrm.y, b.uy, nrm.x * b.ux)) * inv;
    sn = (side < 0.) ? -sn : sn;                              // > 0: the axis points to the inner side
    const bool usable = (n2 > 0.) & (__builtin_fabs(side) * inv > 1e-9 * c.dist);   // the centroid is clearly on one side
    const double m_plus = -sn - b.chord - 1e-7, m_minus = sn - b.chord - 1e-7;
    c.plus = c.plus | (usable & (m_plus > 0.) & !(m_plus * c.far < b.rho));
    c.minus = c.minus | (usable & (m_minus > 0.) & !(m_minus * c.far < b.rho));
}
__device__ __forceinline__ EdgeCull cull_edges_begin(const double2 *pp, const Bundle &b, const SphereCull &sph, bool planar) {
    EdgeCull c;
    c.vx = sph.vx; c.vy = sph.vy; c.vz = sph.vz;
    const double2 w0 = pp[0], w1 = pp[1], w2 = pp[2], w3 = pp[3], w4 = pp[4], w5 = pp[5], w6 = pp[6];
    c.nv = planar ? (uint32_t)w6.x : 0u;                      // 0: no edge test for this one
    // vertices relative to the apex; a triangle repeats its first vertex as the fourth
    c.e0 = mk(w0.x - b.ax, w0.y - b.ay, w1.x - b.az);
    const V3 e1 = mk(w1.y - b.ax, w2.x - b.ay, w2.y - b.az), e2 = mk(w3.x - b.ax, w3.y - b.ay, w4.x - b.az);
    c.e3 = mk(w4.y - b.ax, w5.x - b.ay, w5.y - b.az);
    // how far the primitive is from the apex at least (its bounding sphere), for the rho term
    c.dist = (double)__builtin_sqrtf((float)sph.vv);          // |C - A| to 6e-8
    c.far = __builtin_fmax(c.dist * (1. - 1e-6) - sph.r, 0.);
    c.plus = false; c.minus = false;
    cull_edge(c, b, c.e0, e1);
    cull_edge(c, b, e1, e2);
    cull_edge(c, b, e2, c.e3);
    return c;
}
__device__ __forceinline__ void cull_edges_fourth(EdgeCull &c, const Bundle &b) {
    const bool was_p = c.plus, was_m = c.minus;
    cull_edge(c, b, c.e3, c.e0);
    c.plus = (c.nv == 4u) ? c.plus : was_p;
    c.minus = (c.nv == 4u) ? c.minus : was_m;
}
__device__ __forceinline__ bool cull_edges_end(const EdgeCull &c, const Bundle &b, bool planar) {
    return planar & (c.nv >= 3u) & (b.two_sided ? (c.plus & c.minus) : c.plus);
}
__device__ __forceinline__ bool cull_edges(const double2 *pp, const Bundle &b, const SphereCull &sph, bool planar) {
    EdgeCull c = cull_edges_begin(pp, b, sph, planar);
    if (__any(c.nv == 4u)) cull_edges_fourth(c, b);
    return cull_edges_end(c, b, planar);
}

// The two arrays packed into an LDS block: 4 n words of bounds, then 16 words per planar primitive.  (One wave to a workgroup.)
__device__ __forceinline__ void cull_stage(const double *__restrict__ blob, const rm_dev_header &H, double *lds) {
    const uint32_t lane = threadIdx.x & 63u, n = H.n_spheres + H.n_polygons + H.n_triangles, npl = H.n_polygons + H.n_triangles;
    const double2 *src_b = reinterpret_cast<const double2 *>(blob + H.off_bounds), *src_p = reinterpret_cast<const double2 *>(blob + H.off_planar);
    double2 *bounds = reinterpret_cast<double2 *>(lds), *planar = reinterpret_cast<double2 *>(lds + 4u * n);
    for (uint32_t i = lane; i < 2u * n; i += 64u) bounds[i] = src_b[i];
    for (uint32_t i = lane; i < 8u * npl; i += 64u) planar[i] = src_p[i];
}

template <bool EDGES>
__device__ __forceinline__ unsigned long long cull_step(const SceneView &sc, const Bundle &b, uint32_t base, uint32_t n) {
    const uint32_t pid = base + (threadIdx.x & 63u);
    const bool in = pid < n;
    // (per-lane loads from the blob.  The two arrays in the wave's LDS block instead (KernelArgs::cull_lds_words, RM_CULL_LDS=1):
    // no difference in round 2 -- 68.2 / 68.2 us on the Cornell box, 1936 / 1930 us on 256 spheres -- and slower in round 4, with
    // the Cornell launch at 33 us: 33.8 against 33.0)
    const double2 *bp = reinterpret_cast<const double2 *>(sc.cull_bounds) + 2u * (in ? pid : 0u);
    const SphereCull sph = cull_sphere(bp, b);
    bool out = sph.out;
    const uint32_t ns = sc.H.n_spheres;
    const bool planar = in & (pid >= ns) & !out;
    if (EDGES && __any(planar)) {                                     // this step holds planar primitives the spheres kept
        const double2 *pp = reinterpret_cast<const double2 *>(sc.cull_planar) + 8u * (planar ? pid - ns : 0u);
        out = out | cull_edges(pp, b, sph, planar);
    }
    return __ballot(in & !out);
}

// ---- wave-cooperative hierarchy walk --------------------------------------------------
// For scenes with many spheres / triangles the upload builds a bounding-volume hierarchy
// per kind (rm_bvh.hpp).  The WAVE walks it together: a node is fetched with scalar
// loads, every lane tests its own ray against the two child boxes, and a child is visited
// when ANY lane needs it (one vote per child).  The stack is therefore one per wave (LDS,
// uniform index) instead of one per lane, the node and leaf fetches stay scalar, and a
// leaf runs the very same primitive tests as the flat walk -- the hierarchy only decides
// which primitives are tested, so results are identical.  It serves the bundles too wide
// to cull (incoherent secondary rays) and the scenes too large to cull lane by lane.
struct RayBox {
    double ix, iy, iz;      // 1 / d, clamped to +-1e150 where |d| < 1e-150
    double ax, ay, az;      // -o / d
};

// A ray component of exactly 0 is routine here (the image's centre column and row), and
// with 1/0 = inf the slab expressions turn into inf - inf = NaN, which fmin/fmax then
// silently drop -- in the wrong direction for one of the two faces.  A huge finite
// reciprocal keeps the arithmetic ordinary: inside the slab the two face distances are
// -huge and +huge, outside they have the same sign and the box is missed.
__device__ __forceinline__ double slab_rcp(double d) {
    return (__builtin_fabs(d) < 1e-150) ? __builtin_copysign(1e150, d) : 1. / d;
}

__device__ __forceinline__ RayBox ray_box(V3 o, V3 d) {
    RayBox r;
    r.ix = slab_rcp(d.x); r.iy = slab_rcp(d.y); r.iz = slab_rcp(d.z);
    r.ax = -o.x * r.ix; r.ay = -o.y * r.iy; r.az = -o.z * r.iz;
    return r;
}

// Entry distance of the ray into the box lo..hi (slab test); returns false when the ray
// misses it or enters beyond `limit`.  Boxes are inflated on the host by 1e-7 relative,
// far more than the rounding of these expressions, so the test is conservative.
__device__ __forceinline__ bool box_hit(const double *b, const RayBox &r, double limit, double &t_in) {
    // (fused, in the strict flavour too: this test only decides which primitives are tested, and its margin is the boxes' 1e-7 --
    // six instructions for twelve at every node of every walk)
    const double x1 = __builtin_fma(b[0], r.ix, r.ax), x2 = __builtin_fma(b[3], r.ix, r.ax);
    const double y1 = __builtin_fma(b[1], r.iy, r.ay), y2 = __builtin_fma(b[4], r.iy, r.ay);
    const double z1 = __builtin_fma(b[2], r.iz, r.az), z2 = __builtin_fma(b[5], r.iz, r.az);
    const double lo = __builtin_fmax(__builtin_fmax(__builtin_fmin(x1, x2), __builtin_fmin(y1, y2)),
                                     __builtin_fmax(__builtin_fmin(z1, z2), 0.));
    const double hi = __builtin_fmin(__builtin_fmin(__builtin_fmax(x1, x2), __builtin_fmax(y1, y2)),
                                     __builtin_fmax(z1, z2));
    t_in = lo;
    return !(lo > hi) & !(lo > limit);
}

// Walks the hierarchy at blob offset `off`.  `limit()` gives the lane's current pruning
// distance (+inf for "any"), `done()` says the lane needs nothing (more), `leaf(first,
// count)` tests the primitives [first, first+count) of the kind for all lanes.
// The builder keeps the depth under 60 (rm_bvh.hpp) and the upload checks it: the 64-entry
// stack cannot overflow; the guard below is the last line of defence (a wave that would
// overflow stops descending rather than write beyond its LDS block).
template <class Limit, class Done, class Leaf>
__device__ __forceinline__ void bvh_walk(const SceneView &sc, uint32_t off, const RayBox &rb, Limit limit, Done done,
                                         Leaf leaf) {
    const double *__restrict__ G = sc.G;
    uint32_t sp = 0;
    uint32_t cur = 0;                                   // inner node index; the root is node 0
    RM_WCOUNT(sc, 0, 1u);
    for (;;) {
        RM_WCOUNT(sc, 1, 1u);
        const double *nd = G + off + RM_BVH_NODE_WORDS * cur;
        const double boxes[12] = {nd[0], nd[1], nd[2], nd[3], nd[4], nd[5], nd[6], nd[7], nd[8], nd[9], nd[10], nd[11]};
        const uint32_t *refs = reinterpret_cast<const uint32_t *>(nd + 12);
        const uint32_t l_idx = refs[0], l_cnt = refs[1], r_idx = refs[2], r_cnt = refs[3];
        const bool live = !done();
        if (!__any(live)) return;
        const double lim = limit();
        double tl, tr;
        const bool hl = live & box_hit(boxes, rb, lim, tl);
        const bool hr = live & box_hit(boxes + 6, rb, lim, tr);
        const bool any_l = __any(hl), any_r = __any(hr);
        RM_WCOUNT(sc, 3, (uint32_t)__popcll(__ballot(hl)) + (uint32_t)__popcll(__ballot(hr)));
        // visit the child most lanes enter first, park the other
        uint32_t first_idx = 0, first_cnt = 0, second_idx = 0, second_cnt = 0;
        bool have_first = false, have_second = false;
        if (any_l & any_r) {
            const bool left_first = __popcll(__ballot(hl & (!hr | (tl <= tr)))) >= __popcll(__ballot(hr & (!hl | (tr < tl))));
            first_idx = left_first ? l_idx : r_idx;   first_cnt = left_first ? l_cnt : r_cnt;
            second_idx = left_first ? r_idx : l_idx;  second_cnt = left_first ? r_cnt : l_cnt;
            have_first = have_second = true;
        } else if (any_l) { first_idx = l_idx; first_cnt = l_cnt; have_first = true; }
        else if (any_r)   { first_idx = r_idx; first_cnt = r_cnt; have_first = true; }

        // near child first (so that closest-hit pruning tightens early); the far child is
        // parked on the wave's stack, leaves included (entry: bit 31 = leaf, bits 30:29 =
        // count - 1, bits 28:0 = first primitive or node index)
        if (have_second) {
            if (sp >= 64u) return;                        // cannot happen (depth <= 60 checked at upload)
            sc.bstack[sp++] = second_cnt ? (0x80000000u | ((second_cnt - 1u) << 29) | second_idx) : second_idx;
        }
        bool descended = false;
        if (have_first) {
            if (first_cnt) { RM_WCOUNT(sc, 2, first_cnt); leaf(first_idx, first_cnt); }
            else { cur = first_idx; descended = true; }
        }
        while (!descended) {
            if (sp == 0) return;
            const uint32_t e = __builtin_amdgcn_readfirstlane(sc.bstack[--sp]);
            if (e & 0x80000000u) { RM_WCOUNT(sc, 2, ((e >> 29) & 3u) + 1u); leaf(e & 0x1FFFFFFFu, ((e >> 29) & 3u) + 1u); }
            else { cur = e; descended = true; }
        }
    }
}

// ---- closest hit ---------------------------------------------------------
struct ClosestState {
    bool hit;
    double best, best_t;
    uint32_t best_pid;
};

__device__ __forceinline__ void closest_update(ClosestState &c, bool take, double dist, double t, uint32_t pid) {
    c.best = take ? dist : c.best;
    c.best_t = take ? t : c.best_t;
    c.best_pid = take ? pid : c.best_pid;
    c.hit = c.hit | take;
}

template <bool ORDERED_WALK>
__device__ __forceinline__ void closest_sphere(const SceneView &sc, ClosestState &c, const SphereRec &s, uint32_t pid,
                                               V3 o, V3 d, bool on) {
    double tca, d2;
    sphere_setup(s, o, d, tca, d2);
    const bool in = on & !(d2 > s.r2);                               // sphere.rs:37
    if (!__any(in)) return;                                          // the whole wave misses: no sqrt
    const double thc = RM_SQRT_DISCRIMINANT(s.r2 - d2);
    const double t0 = tca - thc;
    const double t1 = tca + thc;
    const double t = (t0 < 0.) ? t1 : t0;                            // :46-48
    const bool valid = in & !(t < 0.);                               // :50-52
#if RM_FAST
    const double dist = t;           // |o + d t - o|^2 = t^2 is monotonic in t >= 0: order by t
#else
    const V3 p = o + scaled(d, t);
    const V3 dp = p - o;
    const double dist = dot(dp, dp);                                 // shapes.rs:128
#endif
    closest_update(c, closer<ORDERED_WALK>(sc, valid, c.hit, dist, c.best, pid, c.best_pid), dist, t, pid);
}

template <bool ORDERED_WALK, class AT = StoredPlanar>
__device__ __forceinline__ void closest_polygon(const SceneView &sc, ClosestState &c, uint32_t g, V3 o, V3 d, bool on, const AT at = AT()) {
    const PolyRec pg = load_polygon(sc.G, sc.H, g);
    double dist;
    V3 p;
    const bool valid = polygon_hit(sc.G, sc.H, pg, pg.q, o, d, on, dist, p, at);
    if (!__any(valid)) return;
#if RM_FAST
    const double dh = dist;
#else
    const V3 dp = p - o;
    const double dh = dot(dp, dp);
#endif
    const uint32_t pid = sc.H.n_spheres + g;
    closest_update(c, closer<ORDERED_WALK>(sc, valid, c.hit, dh, c.best, pid, c.best_pid), dh, dist, pid);
}

// obj.rs:193-210: closest triangle, strict `<`
template <bool ORDERED_WALK, class AT = StoredPlanar>
__device__ __forceinline__ void closest_triangle(const SceneView &sc, ClosestState &c, const TriRec &t, uint32_t k, V3 o,
                                                 V3 d, bool on, const AT at = AT()) {
    double dist;
    V3 p;
    const bool valid = triangle_hit(t, o, d, on, dist, p, at);
    if (!__any(valid)) return;
#if RM_FAST
    const double dh = dist;
#else
    const V3 dp = p - o;
    const double dh = dot(dp, dp);
#endif
    const uint32_t pid = sc.H.n_spheres + sc.H.n_polygons + k;
    closest_update(c, closer<ORDERED_WALK>(sc, valid, c.hit, dh, c.best, pid, c.best_pid), dh, dist, pid);
}

// `on`: the lanes that hold a ray.  Returns, per lane, whether its ray hit anything.
// (Host-precomputed origin-only terms for the primary rays of the plain-walk kernels -- the
// vector to each sphere's centre and its square, the plane numerators: 48 of ~1,200 vector
// instructions per tile -- were measured in both rounds and cost more than they save: two
// code paths per primitive, 114 -> 126 VGPRs, 80.5 -> 83.0 us.)
// `have_mask` (wave-uniform): the tile was classified and these are its primary rays -- only the
// primitives of `mask` (bit = pid, scenes of up to 64 primitives) can be hit by any of them
// (rm_classify.hip: the same conservative tests as the bundle cull, once per tile instead of once per wave).
// `spheres`: where each sphere stands (StoredSpheres: as the scene image says; another rule walks flat, without cull or mask).
template <bool BVH, bool CULL, bool EDGES, class SPHERES = StoredSpheres>
__device__ __forceinline__ bool closest_hit(const SceneView &sc, V3 o, V3 d, bool on, Hit &out, bool have_mask, unsigned long long mask,
                                            const SPHERES &spheres = SPHERES()) {
    static_assert(!SPHERES::moves || (SPHERES::swept && !CULL) || (!BVH && !CULL),
                  "moved shapes walk flat, or a hierarchy swept over their offsets: boxes and bundles hold for the stored records");
    const double *__restrict__ S = sc.G;
    const rm_dev_header &H = sc.H;
    ClosestState c{false, 0., 0., 0u};

    if (have_mask) {                                                 // wave-uniform
        const uint32_t ns = H.n_spheres, np = H.n_polygons;
        unsigned long long m = mask;
        while (m) {
            const uint32_t pid = (uint32_t)__builtin_ctzll(m);
            m &= m - 1ull;
            // (ascending pid order, like the plain walk: list order decides ties where it survived)
            if (pid < ns) closest_sphere<true>(sc, c, load_sphere(S, H, pid), pid, o, d, on);
            else if (pid < ns + np) closest_polygon<true>(sc, c, pid - ns, o, d, on);
            else closest_triangle<true>(sc, c, load_triangle(S, H, pid - ns - np), pid - ns - np, o, d, on);
        }
        out.t = c.best_t;
        out.pid = c.best_pid;
        return c.hit;
    }

    if (CULL) {
        const Bundle b = bundle_of_rays(o, d, on, sc.cull_cos);
        RM_COUNT(sc, b.narrow ? 3 : 2, 1u);
        if (b.narrow) {                                              // wave-uniform
            const uint32_t ns = H.n_spheres, np = H.n_polygons, n = ns + np + H.n_triangles;
            unsigned long long groups = H.off_groups ? cull_groups(sc, b, (n + 63u) >> 6) : ~0ull;
            if (H.off_groups) RM_COUNT(sc, 0, 1u);
            for (uint32_t base = 0; base < n; base += 64u, groups >>= 1) {
                if (!(groups & 1ull)) continue;
                // (a last step of a few primitives -- 257 = 4 x 64 + 1 -- is not worth a cull step:
                // they are tested as they are)
                unsigned long long m = n - base <= RM_CULL_TAIL ? ((1ull << (n - base)) - 1ull) : cull_step<EDGES>(sc, b, base, n);
                RM_COUNT(sc, 0, 1u); RM_COUNT(sc, 1, (uint32_t)__popcll(m));
                while (m) {
                    const uint32_t pid = base + (uint32_t)__builtin_ctzll(m);
                    m &= m - 1ull;
                    // (ascending pid order, like the plain walk: list order decides ties where it survived)
                    if (pid < ns) closest_sphere<true>(sc, c, load_sphere(S, H, pid), pid, o, d, on);
                    else if (pid < ns + np) closest_polygon<true>(sc, c, pid - ns, o, d, on);
                    else closest_triangle<true>(sc, c, load_triangle(S, H, pid - ns - np), pid - ns - np, o, d, on);
                }
            }
            out.t = c.best_t;
            out.pid = c.best_pid;
            return c.hit;
        }
    }

    RayBox rb{};
    if (BVH) rb = ray_box(o, d);
    // a box entered beyond the lane's best hit cannot improve it.  best_t is the reference's t = tca -+ thc, the box's entry a
    // ray parameter: the two agree only as far as d.d = 1.  The margin covers the rays a kernel forms itself (normalised:
    // |d.d - 1| < 1e-15) and, in the strict flavour, hits ordered by |p - o|^2 rather than t; it does NOT cover a caller's
    // ray, admitted with |d.d - 1| < 1e-4 -- the kernels that take those walk without the hierarchy where a wave holds one
    // (rm_radiance_step.inc, complete_walk_view).
    auto prune_at = [&]() { return c.hit ? c.best_t * (1. + 1e-7) + 1e-12 : __builtin_inf(); };
    auto off_lane = [&]() { return !on; };

    uint32_t i = 0;
    if (BVH && H.off_bvh_spheres) {
        bvh_walk(sc, H.off_bvh_spheres, rb, prune_at, off_lane, [&](uint32_t first, uint32_t cnt) {
            const SphereRec s0 = load_sphere(S, H, first), s1 = load_sphere(S, H, first + 1u);
            const SphereRec s2 = load_sphere(S, H, first + 2u), s3 = load_sphere(S, H, first + 3u);
            if constexpr (SPHERES::moves) {
                // a swept hierarchy: the rule stands in the leaves as in the flat loops, and is asked for the primitives the leaf
                // holds alone -- the records behind the last leaf are padding, the pid map behind it is not there at all
                closest_sphere<false>(sc, c, spheres(s0, first), first, o, d, on);
                if (cnt > 1u) closest_sphere<false>(sc, c, spheres(s1, first + 1u), first + 1u, o, d, on);
                if (cnt > 2u) closest_sphere<false>(sc, c, spheres(s2, first + 2u), first + 2u, o, d, on);
                if (cnt > 3u) closest_sphere<false>(sc, c, spheres(s3, first + 3u), first + 3u, o, d, on);
                return;
            }
            closest_sphere<false>(sc, c, s0, first, o, d, on);
            if (cnt > 1u) closest_sphere<false>(sc, c, s1, first + 1u, o, d, on);
            if (cnt > 2u) closest_sphere<false>(sc, c, s2, first + 2u, o, d, on);
            if (cnt > 3u) closest_sphere<false>(sc, c, s3, first + 3u, o, d, on);
        });
        i = H.n_spheres;
    }
    for (; i + 4u <= H.n_spheres; i += 4u) {
        const SphereRec s0 = spheres(load_sphere(S, H, i), i), s1 = spheres(load_sphere(S, H, i + 1u), i + 1u);
        const SphereRec s2 = spheres(load_sphere(S, H, i + 2u), i + 2u), s3 = spheres(load_sphere(S, H, i + 3u), i + 3u);
        closest_sphere<true>(sc, c, s0, i, o, d, on);
        closest_sphere<true>(sc, c, s1, i + 1u, o, d, on);
        closest_sphere<true>(sc, c, s2, i + 2u, o, d, on);
        closest_sphere<true>(sc, c, s3, i + 3u, o, d, on);
    }
    for (; i < H.n_spheres; i++) closest_sphere<true>(sc, c, spheres(load_sphere(S, H, i), i), i, o, d, on);

    typename SPHERES::Planar at = spheres.planar();
    for (uint32_t g = 0; g < H.n_polygons; g++) closest_polygon<true>(sc, c, g, o, d, on, at.polygon(g));

    uint32_t k = 0;
    if (BVH && H.off_bvh_triangles) {
        bvh_walk(sc, H.off_bvh_triangles, rb, prune_at, off_lane, [&](uint32_t first, uint32_t cnt) {
            const TriRec t0 = load_triangle(S, H, first), t1 = load_triangle(S, H, first + 1u);
            if constexpr (SPHERES::moves) {                              // (as the spheres' leaves above)
                closest_triangle<false>(sc, c, t0, first, o, d, on, at.triangle(first));
                if (cnt > 1u) closest_triangle<false>(sc, c, t1, first + 1u, o, d, on, at.triangle(first + 1u));
                return;
            }
            closest_triangle<false>(sc, c, t0, first, o, d, on);
            if (cnt > 1u) closest_triangle<false>(sc, c, t1, first + 1u, o, d, on);
        });
        k = H.n_triangles;
    }
    for (; k + 2u <= H.n_triangles; k += 2u) {
        const TriRec t0 = load_triangle(S, H, k), t1 = load_triangle(S, H, k + 1u);
        closest_triangle<true>(sc, c, t0, k, o, d, on, at.triangle(k));
        closest_triangle<true>(sc, c, t1, k + 1u, o, d, on, at.triangle(k + 1u));
    }
    for (; k < H.n_triangles; k++) closest_triangle<true>(sc, c, load_triangle(S, H, k), k, o, d, on, at.triangle(k));

    out.t = c.best_t;
    out.pid = c.best_pid;
    return c.hit;
}

// ---- any hit (shadow rays) -------------------------------------------------
// shapes.rs:92-108.  The answer does not depend on visiting order.  A lane that
// has found an occluder keeps walking with its result latched; the wave leaves
// a loop early once every lane is occluded or switched off (one vote per batch).
__device__ __forceinline__ bool shadow_sphere_from(const SphereRec &s, const SphereFrom &f, V3 d, bool occ) {
    double tca, d2;
    sphere_setup(f, d, tca, d2);
    const bool in = !(d2 > s.r2);
    // sphere.rs:43-52: hit unless both roots are negative.  thc >= 0, so tca >= 0
    // already gives t1 = tca + thc >= 0 without the square root.
    const bool front = !(tca < 0.);
    bool hit = in & front;
    const bool need = in & !front & !occ;          // origin inside the sphere, or the sphere behind it
    if (__any(need)) {
        const double thc = RM_SQRT_DISCRIMINANT(s.r2 - d2);
        const double t0 = tca - thc;
        const double t1 = tca + thc;
        const double t = (t0 < 0.) ? t1 : t0;
        hit = hit | (need & !(t < 0.));
    }
    return hit;
}
__device__ __forceinline__ bool shadow_sphere(const SphereRec &s, V3 o, V3 d, bool occ) {
    return shadow_sphere_from(s, sphere_from(s, o), d, occ);
}

// Two shadow rays from ONE origin (the two lights of a hit, when both lie on the same side of
// the surface: the origin is the hit point 1e-3 of the normal off it, renderer.rs:168-172) in
// one walk of the plain list: what depends on the origin alone -- the vector to a sphere's
// centre and its square, the numerator of a plane hit -- is computed once, bit for bit what
// each ray's own walk computes; the records are fetched once.  (Few-primitive kernels only:
// the bundles of the two lights cull different primitives.)
template <class SPHERES = StoredSpheres>
__device__ __forceinline__ void any_hit2(const SceneView &sc, V3 o, V3 d0, V3 d1, bool decided0, bool decided1, bool &out0,
                                         bool &out1, const SPHERES &spheres = SPHERES()) {
    const double *__restrict__ S = sc.G;
    const rm_dev_header &H = sc.H;
    bool occ0 = decided0, occ1 = decided1;
    out0 = occ0; out1 = occ1;
    if (__all(occ0 & occ1)) return;
    auto sphere = [&](const SphereRec &s) {
        const SphereFrom f = sphere_from(s, o);
        occ0 = occ0 | shadow_sphere_from(s, f, d0, occ0);
        occ1 = occ1 | shadow_sphere_from(s, f, d1, occ1);
    };
    uint32_t i = 0;
    for (; i + 4u <= H.n_spheres; i += 4u) {
        const SphereRec s0 = spheres(load_sphere(S, H, i), i), s1 = spheres(load_sphere(S, H, i + 1u), i + 1u);
        const SphereRec s2 = spheres(load_sphere(S, H, i + 2u), i + 2u), s3 = spheres(load_sphere(S, H, i + 3u), i + 3u);
        sphere(s0); sphere(s1); sphere(s2); sphere(s3);
        if (__all(occ0 & occ1)) { out0 = occ0; out1 = occ1; return; }
    }
    for (; i < H.n_spheres; i++) sphere(spheres(load_sphere(S, H, i), i));
    typename SPHERES::Planar at = spheres.planar();
    for (uint32_t g = 0; g < H.n_polygons; g++) {
        if (__all(occ0 & occ1)) break;
        const PolyRec pg = load_polygon(S, H, g);
        at.polygon(g);
        const double num = plane_num(at.x(pg.px), at.y(pg.py), at.z(pg.pz), pg.nx, pg.ny, pg.nz, o);
        double dist;
        V3 p;
        occ0 = occ0 | polygon_hit_num(S, H, pg, pg.q, num, o, d0, !occ0, dist, p, at);
        occ1 = occ1 | polygon_hit_num(S, H, pg, pg.q, num, o, d1, !occ1, dist, p, at);
    }
    for (uint32_t k = 0; k < H.n_triangles; k++) {
        if (__all(occ0 & occ1)) break;
        const TriRec t = load_triangle(S, H, k);
        at.triangle(k);
        const double num = plane_num(at.x(t.cx), at.y(t.cy), at.z(t.cz), t.nx, t.ny, t.nz, o);
        double dist;
        V3 p;
        occ0 = occ0 | triangle_hit_num(t, num, o, d0, !occ0, dist, p, at);
        occ1 = occ1 | triangle_hit_num(t, num, o, d1, !occ1, dist, p, at);
    }
    out0 = occ0; out1 = occ1;
}

// The same walk over the primitives of `m0 | m1` only (wave-uniform, bit = pid, scenes of up to 64 pids): those
// that ray 0 / ray 1 of SOME lane can hit at all (shadow_masks2).  A primitive outside a ray's mask is not
// tested for it: no lane's answer can change, since the lane's own mask is part of the union.
__device__ __forceinline__ void any_hit2_masked(const SceneView &sc, V3 o, V3 d0, V3 d1, bool decided0, bool decided1, bool &out0,
                                                bool &out1, unsigned long long m0, unsigned long long m1) {
    const double *__restrict__ S = sc.G;
    const rm_dev_header &H = sc.H;
    const uint32_t ns = H.n_spheres, np = H.n_polygons;
    bool occ0 = decided0, occ1 = decided1;
    unsigned long long m = m0 | m1;
    while (m && !__all(occ0 & occ1)) {
        const uint32_t pid = (uint32_t)__builtin_ctzll(m);
        m &= m - 1ull;
        const bool t0 = (m0 >> pid) & 1ull, t1 = (m1 >> pid) & 1ull;
        if (pid < ns) {
            const SphereRec s = load_sphere(S, H, pid);
            const SphereFrom f = sphere_from(s, o);
            if (t0) occ0 = occ0 | shadow_sphere_from(s, f, d0, occ0);
            if (t1) occ1 = occ1 | shadow_sphere_from(s, f, d1, occ1);
        } else if (pid < ns + np) {
            const PolyRec pg = load_polygon(S, H, pid - ns);
            const double num = plane_num(pg.px, pg.py, pg.pz, pg.nx, pg.ny, pg.nz, o);
            double dist;
            V3 p;
            if (t0) occ0 = occ0 | polygon_hit_num(S, H, pg, pg.q, num, o, d0, !occ0, dist, p);
            if (t1) occ1 = occ1 | polygon_hit_num(S, H, pg, pg.q, num, o, d1, !occ1, dist, p);
        } else {
            const TriRec t = load_triangle(S, H, pid - ns - np);
            const double num = plane_num(t.cx, t.cy, t.cz, t.nx, t.ny, t.nz, o);
            double dist;
            V3 p;
            if (t0) occ0 = occ0 | triangle_hit_num(t, num, o, d0, !occ0, dist, p);
            if (t1) occ1 = occ1 | triangle_hit_num(t, num, o, d1, !occ1, dist, p);
        }
    }
    out0 = occ0; out1 = occ1;
}

// Occluder masks (rm_build_shadow_masks, at upload; H.off_occ != 0): occ[q][l] holds every primitive a shadow ray
// cast from a hit on q towards light l can hit.  The union of the rows of the primitives the wave's lanes shade
// (`got`, `pid`), for lights l and l + 1, is all their walk needs.  (A scalar loop, one step per distinct
// primitive: a vote, a lane read, two scalar loads.)
__device__ __forceinline__ void shadow_masks2(const SceneView &sc, bool got, uint32_t pid, uint32_t l, unsigned long long &m0,
                                              unsigned long long &m1) {
    const unsigned long long *occ = reinterpret_cast<const unsigned long long *>(sc.G + sc.H.off_occ) + l;
    unsigned long long left = __ballot(got);
    m0 = 0ull; m1 = 0ull;
    while (left) {
        const uint32_t q = (uint32_t)__builtin_amdgcn_readlane((int)pid, (int)__builtin_ctzll(left));
        m0 |= occ[q * sc.H.n_lights];
        m1 |= occ[q * sc.H.n_lights + 1u];
        left &= ~__ballot(got & (pid == q));
    }
}

// `decided`: lanes whose answer is not needed (no hit to shade, or a light that adds
// exactly zero); they come back as occluded.  `through` / `rho`: every shadow ray passes
// within rho of that point -- the light (renderer.rs:166-172: the direction is taken from
// the hit point, the origin is 1e-3 of the normal off it).
template <bool BVH, bool CULL, bool EDGES, class SPHERES = StoredSpheres>
__device__ __forceinline__ bool any_hit(const SceneView &sc, V3 o, V3 d, bool decided, V3 through, double rho,
                                        const SPHERES &spheres = SPHERES()) {
    static_assert(!SPHERES::moves || (SPHERES::swept && !CULL) || (!BVH && !CULL),
                  "moved shapes walk flat, or a hierarchy swept over their offsets: boxes and bundles hold for the stored records");
    const double *__restrict__ S = sc.G;
    const rm_dev_header &H = sc.H;
    bool occ = decided;
    if (__all(occ)) return occ;

    if (CULL) {
        const Bundle b = bundle_through(through, rho, d, !occ, sc.cull_cos);
        RM_COUNT(sc, b.narrow ? 3 : 2, 1u);
        if (b.narrow) {
            const uint32_t ns = H.n_spheres, np = H.n_polygons, n = ns + np + H.n_triangles;
            unsigned long long groups = H.off_groups ? cull_groups(sc, b, (n + 63u) >> 6) : ~0ull;
            if (H.off_groups) RM_COUNT(sc, 0, 1u);
            for (uint32_t base = 0; base < n; base += 64u, groups >>= 1) {
                if (!(groups & 1ull)) continue;
                // (a last step of a few primitives -- 257 = 4 x 64 + 1 -- is not worth a cull step:
                // they are tested as they are)
                unsigned long long m = n - base <= RM_CULL_TAIL ? ((1ull << (n - base)) - 1ull) : cull_step<EDGES>(sc, b, base, n);
                RM_COUNT(sc, 0, 1u); RM_COUNT(sc, 1, (uint32_t)__popcll(m));
                while (m) {
                    const uint32_t pid = base + (uint32_t)__builtin_ctzll(m);
                    m &= m - 1ull;
                    double dist;
                    V3 p;
                    if (pid < ns) occ = occ | shadow_sphere(load_sphere(S, H, pid), o, d, occ);
                    else if (pid < ns + np) {
                        const PolyRec pg = load_polygon(S, H, pid - ns);
                        occ = occ | polygon_hit(S, H, pg, pg.q, o, d, !occ, dist, p);
                    } else occ = occ | triangle_hit(load_triangle(S, H, pid - ns - np), o, d, !occ, dist, p);
                    if (__all(occ)) return occ;
                }
            }
            return occ;
        }
    }

    RayBox rb{};
    if (BVH) rb = ray_box(o, d);
    auto no_limit = [&]() { return __builtin_inf(); };
    auto occluded = [&]() { return occ; };

    uint32_t i = 0;
    if (BVH && H.off_bvh_spheres) {
        bvh_walk(sc, H.off_bvh_spheres, rb, no_limit, occluded, [&](uint32_t first, uint32_t cnt) {
            const SphereRec s0 = load_sphere(S, H, first), s1 = load_sphere(S, H, first + 1u);
            const SphereRec s2 = load_sphere(S, H, first + 2u), s3 = load_sphere(S, H, first + 3u);
            if constexpr (SPHERES::moves) {                              // (a swept hierarchy: closest_hit's leaves)
                occ = occ | shadow_sphere(spheres(s0, first), o, d, occ);
                if (cnt > 1u) occ = occ | shadow_sphere(spheres(s1, first + 1u), o, d, occ);
                if (cnt > 2u) occ = occ | shadow_sphere(spheres(s2, first + 2u), o, d, occ);
                if (cnt > 3u) occ = occ | shadow_sphere(spheres(s3, first + 3u), o, d, occ);
                return;
            }
            occ = occ | shadow_sphere(s0, o, d, occ);
            if (cnt > 1u) occ = occ | shadow_sphere(s1, o, d, occ);
            if (cnt > 2u) occ = occ | shadow_sphere(s2, o, d, occ);
            if (cnt > 3u) occ = occ | shadow_sphere(s3, o, d, occ);
        });
        if (__all(occ)) return occ;
        i = H.n_spheres;
    }
    for (; i + 4u <= H.n_spheres; i += 4u) {
        const SphereRec s0 = spheres(load_sphere(S, H, i), i), s1 = spheres(load_sphere(S, H, i + 1u), i + 1u);
        const SphereRec s2 = spheres(load_sphere(S, H, i + 2u), i + 2u), s3 = spheres(load_sphere(S, H, i + 3u), i + 3u);
        occ = occ | shadow_sphere(s0, o, d, occ);
        occ = occ | shadow_sphere(s1, o, d, occ);
        occ = occ | shadow_sphere(s2, o, d, occ);
        occ = occ | shadow_sphere(s3, o, d, occ);
        if (__all(occ)) return occ;
    }
    for (; i < H.n_spheres; i++) occ = occ | shadow_sphere(spheres(load_sphere(S, H, i), i), o, d, occ);
    if (__all(occ)) return occ;

    typename SPHERES::Planar at = spheres.planar();
    for (uint32_t g = 0; g < H.n_polygons; g++) {
        const PolyRec pg = load_polygon(S, H, g);
        double dist;
        V3 p;
        occ = occ | polygon_hit(S, H, pg, pg.q, o, d, !occ, dist, p, at.polygon(g));
        if (__all(occ)) return occ;
    }

    uint32_t k = 0;
    if (BVH && H.off_bvh_triangles) {
        bvh_walk(sc, H.off_bvh_triangles, rb, no_limit, occluded, [&](uint32_t first, uint32_t cnt) {
            const TriRec t0 = load_triangle(S, H, first), t1 = load_triangle(S, H, first + 1u);
            double dist;
            V3 p;
            if constexpr (SPHERES::moves) {
                occ = occ | triangle_hit(t0, o, d, !occ, dist, p, at.triangle(first));
                if (cnt > 1u) occ = occ | triangle_hit(t1, o, d, !occ, dist, p, at.triangle(first + 1u));
                return;
            }
            occ = occ | triangle_hit(t0, o, d, !occ, dist, p);
            if (cnt > 1u) occ = occ | triangle_hit(t1, o, d, !occ, dist, p);
        });
        return occ;
    }
    for (; k + 2u <= H.n_triangles; k += 2u) {
        const TriRec t0 = load_triangle(S, H, k), t1 = load_triangle(S, H, k + 1u);
        double dist;
        V3 p;
        occ = occ | triangle_hit(t0, o, d, !occ, dist, p, at.triangle(k));
        occ = occ | triangle_hit(t1, o, d, !occ, dist, p, at.triangle(k + 1u));
        if (__all(occ)) return occ;
    }
    for (; k < H.n_triangles; k++) {
        double dist;
        V3 p;
        occ = occ | triangle_hit(load_triangle(S, H, k), o, d, !occ, dist, p, at.triangle(k));
    }
    return occ;
}

// ---- surface record ----------------------------------------------------------
struct Surface {
    V3 point, normal;
    const double *mat;   // RM_MATERIAL_WORDS words in the scene blob
};

// `got`: lanes with a hit.  The other lanes read record 0 of everything (in bounds: the
// blob ends in 64 words of padding) and their surface is never used.
template <bool DIV, class SPHERES = StoredSpheres>
__device__ __forceinline__ Surface surface_at(const SceneView &sc, V3 o, V3 d, const Hit &h, bool got RM_SUS_PARAM,
                                              const SPHERES &spheres = SPHERES()) {
    Surface s;
    s.point = o + scaled(d, h.t);
    const uint32_t ns = sc.H.n_spheres, np = sc.H.n_polygons;
    const uint32_t pid = got ? h.pid : 0u;
    const bool is_s = got & (pid < ns);
    const bool is_p = got & !is_s & (pid < ns + np);
    const bool is_t = got & !is_s & !is_p;
    s.normal = mk(0., 0., 0.);
    if (where<DIV>(is_s)) {
        const double *sp = sc.S + sc.H.off_spheres + RM_SPHERE_WORDS * (is_s ? pid : 0u);
        const V3 centre = spheres.centre(sp, is_s ? pid : 0u);
        s.normal = RM_NORMALIZED(mk(s.point.x - centre.x, s.point.y - centre.y, s.point.z - centre.z), is_s);   // sphere.rs:58
    }
    if (where<DIV>(is_p | is_t)) {
        const uint32_t word = is_p ? sc.H.off_polygons + RM_POLYGON_WORDS * (pid - ns)          // polygon.rs:95
                            : is_t ? sc.H.off_triangles + RM_TRIANGLE_WORDS * (pid - ns - np)   // triangle.rs:80
                                   : 0u;
        const double *rec = sc.S + word;
        s.normal = pick(is_s, s.normal, mk(rec[0], rec[1], rec[2]));
    }
    s.mat = sc.S + sc.H.off_materials + RM_MATERIAL_WORDS * pid;
    return s;
}

// optics.rs:4-6
__device__ __forceinline__ V3 reflect(V3 incident, V3 normal) {
    return incident - scaled(normal, 2. * dot(incident, normal));
}

// ---- specular power: f64::powf (renderer.rs:186-188) ---------------------------------
// POW_GENERIC: the device libm pow (<= 1 ulp), any exponent.  Its ~40 polynomial
// constants cannot be f64 literals on gfx950, so the compiler parks them in VGPRs for
// the whole kernel (+38 VGPRs, one wave per SIMD less).
// POW_INTEGER: exponent is a non-negative integer (checked for every material at
// scene upload): binary powering, bit-for-bit the same special cases as pow for such
// exponents (x^0 = 1 also for NaN; 0^n = 0; sign of negative bases), <= ~10 roundings
// instead of 1, no constants.  Called under a per-lane branch: votes see the lit lanes only.
template <int POW>
__device__ __forceinline__ double specular_pow(double x, double y) {
    if (POW == POW_GENERIC) return pow(x, y);
    uint32_t n = (uint32_t)y;
    double r = 1., b = x;
    const uint32_t n0 = __builtin_amdgcn_readfirstlane(n);
    if (__all(n == n0)) {
        // the usual case -- every lane shades a material with the same exponent: the bit
        // walk runs on the scalar unit and the vector unit only multiplies (x^100: 8 f64
        // multiplies instead of 7 rounds of multiply + select + shift + vote)
        for (uint32_t m = n0; m != 0u; m >>= 1) {
            if (m & 1u) r = r * b;
            if (m > 1u) b = b * b;
        }
        return r;
    }
    while (__any(n != 0u)) {
        if (n & 1u) r = r * b;
        b = b * b;
        n >>= 1;
    }
    return r;
}

// ---- direct lighting: renderer.rs:153-193 ---------------------------------------
// `origin` is the origin of the ray that produced the hit (renderer.rs:275), so
// for secondary rays the "viewer" is the previous hit point.
// Colour arithmetic below the shadow test feeds no hit / miss / side decision -- only the
// pixel value, continuously -- so it may use fused multiply-adds in both flavours.
__device__ __forceinline__ double dot_fused(V3 a, V3 b) {
    return __builtin_fma(a.z, b.z, __builtin_fma(a.y, b.y, a.x * b.x));
}

// One light's terms at a hit, up to the shadow test.
struct LightAt {
    V3 dir;             // :166 normalize(light - point)
    V3 from;            // :168-172 origin of the shadow ray
    V3 pos;
    double ldn, sf;     // light_dir . normal; max(reflect(-light_dir, normal) . dir_to_viewer, 0)
    bool dark;          // adds exactly zero whether or not it is shadowed
};

// Where light l stands, given its record `lt` of the scene image.  The default is the record's own position; a kernel whose
// samples move their lights (rm_soft.hip) hands shade_direct another rule.  In shade_direct nothing else reads a light's position (the occluder masks are keyed on
// the stored ones: such a kernel runs with them off).
struct StoredLights {
    __device__ __forceinline__ V3 operator()(const double *lt, uint32_t) const { return mk(lt[0], lt[1], lt[2]); }
};

template <class LIGHTS = StoredLights>
__device__ __forceinline__ LightAt light_at(const SceneView &sc, uint32_t l, const Surface &s, V3 dir_to_viewer, double exponent, bool got RM_SUS_PARAM,
                                            const LIGHTS &lights = LIGHTS()) {
    (void)got;
    LightAt a;
    const double *lt = sc.G + sc.H.off_lights + RM_LIGHT_WORDS * l;
    a.pos = lights(lt, l);
    a.dir = RM_NORMALIZED(a.pos - s.point, got);                      // :166 (a ray direction: exact)
    a.ldn = dot(a.dir, s.normal);
    // :168-172 point -/+ normal * 1e-3: one expression, p - n k == p + n (-k) bit for bit
    a.from = s.point + scaled(s.normal, (a.ldn < 0.) ? -1e-3 : 1e-3);
    // :144-150 reflect(-light_dir, normal) . dir_to_viewer
    const double k2 = -2. * dot_fused(a.dir, s.normal);
    const V3 reflected = mk(__builtin_fma(-k2, s.normal.x, -a.dir.x), __builtin_fma(-k2, s.normal.y, -a.dir.y),
                            __builtin_fma(-k2, s.normal.z, -a.dir.z));
    a.sf = __builtin_fmax(dot_fused(reflected, dir_to_viewer), 0.);
    // A light that faces neither the surface (diffusion 0) nor the mirror direction
    // (0^exponent = 0) adds exactly zero whether or not it is shadowed: such lanes
    // enter the shadow walk as already decided, and the wave skips it when all are.
    a.dark = !(a.ldn > 0.) & !(a.sf > 0.) & (exponent > 0.);
    return a;
}

// `pid`: the primitive each lane's hit lies on.
// `lights`: where each light stands (StoredLights: as the scene image says).
// `spheres`: where each sphere stands in the shadow walks (StoredSpheres: as the scene image says).
template <int POW, bool BVH, bool CULL, bool EDGES, class LIGHTS = StoredLights, class SPHERES = StoredSpheres>
__device__ __forceinline__ V3 shade_direct(const SceneView &sc, V3 neg_dir, const Surface &s, bool got, uint32_t pid RM_SUS_PARAM,
                                           const LIGHTS &lights = LIGHTS(), const SPHERES &spheres = SPHERES()) {
    const double *m = s.mat;
    const double exponent = m[5];
    // (colour and specular weight are fetched where a light is found unshadowed: held in
    // registers they would be live across both shadow walks)
    // renderer.rs:149 dir_to_viewer = normalize(origin - point).  point = origin + dir * t
    // with |dir| = 1, so this is -dir up to rounding, and it only enters the specular
    // colour term: the ray's own direction is used and a normalisation is saved per hit.
    const V3 dir_to_viewer = neg_dir;
    V3 li = mk(0., 0., 0.);
    auto add_light = [&](uint32_t l, const LightAt &a, bool lit) {
        if (lit) {                                                    // per-lane branch: the sums are updated in place
            const double *lt = sc.G + sc.H.off_lights + RM_LIGHT_WORDS * l;
            const V3 lcol = mk(lt[3], lt[4], lt[5]);
            const double intensity = lt[6];
            const V3 diffuse_color = mk(m[1], m[2], m[3]);
            const double specular_k = m[4];
            const double diffusion = __builtin_fmax(a.ldn, 0.);       // :139
            const double di = diffusion * intensity;
            const double spec = specular_pow<POW>(a.sf * specular_k, exponent);   // :186-188
            // :181-183 + :189
            li = mk(__builtin_fma(lcol.x, spec, __builtin_fma(lcol.x * diffuse_color.x, di, li.x)),
                    __builtin_fma(lcol.y, spec, __builtin_fma(lcol.y * diffuse_color.y, di, li.y)),
                    __builtin_fma(lcol.z, spec, __builtin_fma(lcol.z * diffuse_color.z, di, li.z)));
        }
    };
    // plain-walk kernels: the occluder masks of the walks, where the scene has them
    // (keyed on the stored centres: a rule that moves the spheres walks without them, whatever the header says)
    const bool masks = !BVH && !CULL && !SPHERES::moves && sc.H.off_occ != 0u;
    for (uint32_t l = 0; l < sc.H.n_lights;) {
        const LightAt a = light_at(sc, l, s, dir_to_viewer, exponent, got RM_SUS_ARG, lights);
        const bool dec_a = !got | a.dark;
        if (!BVH && !CULL && l + 1u < sc.H.n_lights) {
            // plain-walk kernels: lights two at a time -- where both lie on the same side of the
            // surface their shadow rays leave one point and share one walk (any_hit2); where some
            // lane has them on opposite sides (rare) the second light is taken up again alone
            const LightAt b = light_at(sc, l + 1u, s, dir_to_viewer, exponent, got RM_SUS_ARG, lights);
            const bool dec_b = !got | b.dark;
            if (__all(dec_a | dec_b | ((a.ldn < 0.) == (b.ldn < 0.)))) {
                bool occ_a, occ_b;
                const unsigned long long t_sh = RM_PHASE_T();
                const V3 from = pick(dec_a, b.from, a.from);
                unsigned long long m_a = 0ull, m_b = 0ull;
                if (masks) shadow_masks2(sc, got, pid, l, m_a, m_b);
                // (where both masks hold every primitive -- hits on the floor: its shadow rays can meet anything --
                // the plain walk, which fetches its records in batches)
                const uint32_t n = sc.H.n_spheres + sc.H.n_polygons + sc.H.n_triangles;
                if (masks && (m_a & m_b) != ((n >= 64u) ? ~0ull : (1ull << n) - 1ull))
                    any_hit2_masked(sc, from, a.dir, b.dir, dec_a, dec_b, occ_a, occ_b, m_a, m_b);
                else
                    any_hit2(sc, from, a.dir, b.dir, dec_a, dec_b, occ_a, occ_b, spheres);
                RM_PHASE_ADD(sc, 1, t_sh);
                add_light(l, a, !occ_a);                              // :174
                add_light(l + 1u, b, !occ_b);
                l += 2u;
                continue;
            }
        }
        const unsigned long long t_sh = RM_PHASE_T();
        const bool lit = !any_hit<BVH, CULL, EDGES>(sc, a.from, a.dir, dec_a, a.pos, sc.H.shadow_rho, spheres);   // :174
        RM_PHASE_ADD(sc, 1, t_sh);
        add_light(l, a, lit);
        l += 1u;
    }
    return scaled(li, m[0]);                                          // :192
}

// ---- secondary rays: optics.rs:8-89 ------------------------------------------------
// Both are computed for all lanes; the result says, per lane, whether the child exists.
// Sign flips are exact in IEEE arithmetic ((-a) b == -(a b), a - b == a + (-b)), so the
// reference's `normal = -normal` / `c = -c` branches become sign selects on scalars:
// reflect(i, -n) == reflect(i, n) bit for bit, and c enters only squared.
// LAZY (per-lane kernels): the reflected ray exists under total reflection only -- no lane of
// most waves has one -- and is computed under that branch.
// `dn`: d . normal, the dot that decides the side of the surface the child starts on (where the child was computed; else 0).
template <bool LAZY>
__device__ __forceinline__ bool reflect_child(V3 incident, const Surface &s, double ri, double inv_ri, V3 &o, V3 &d, double &dn) {
    const double c = dot(s.normal, incident);                         // optics.rs:16 (no sign flip)
    const double r = (c < 0.) ? ri : inv_ri;
    const double cos_theta_2 = 1. - r * r * (1. - c * c);
    const bool has = !(cos_theta_2 > 0.);                             // :33-35
    dn = 0.;
    if (!LAZY || has) {
        d = reflect(incident, s.normal);
        dn = dot(d, s.normal);
        o = s.point + scaled(s.normal, (dn < 0.) ? -1e-4 : 1e-4);     // :41-45, un-flipped normal
    }
    return has;
}
template <bool LAZY>
__device__ __forceinline__ bool reflect_child(V3 incident, const Surface &s, double ri, double inv_ri, V3 &o, V3 &d) {
    double dn;
    return reflect_child<LAZY>(incident, s, ri, inv_ri, o, d, dn);
}

// `dn`: d . normal (the un-flipped normal), the dot that decides the side of the surface the child starts on.
__device__ __forceinline__ bool refract_child(V3 incident, const Surface &s, double ri, double inv_ri, bool glass, V3 &o, V3 &d, double &dn RM_SUS_PARAM) {
    (void)glass;
    const double c0 = -dot(s.normal, incident);                       // optics.rs:57
    const bool flip = c0 < 0.;                                        // :60-68: then c = -c, normal = -normal
    const double r = flip ? ri : inv_ri;
    const double c = flip ? -c0 : c0;
    const double cos_theta_2 = 1. - r * r * (1. - c * c);
    const double k = r * c - __builtin_sqrt(cos_theta_2);
    // (under total reflection k is NaN and there is no such ray: its lanes' flags do not count)
    d = RM_NORMALIZED(scaled(incident, r) + scaled(s.normal, flip ? -k : k), glass & !(cos_theta_2 < 0.));   // :78-79 (flipped normal * k)
    dn = dot(d, s.normal);                                            // d . flipped normal = -(d . normal) when flipped
    const bool along = flip ? (dn < 0.) : (dn > 0.);                  // :82 `dir.dot(normal) > 0` with the flipped normal
    o = s.point + scaled(s.normal, (along != flip) ? 1e-4 : -1e-4);   // :82-86: point +- flipped normal * 1e-4
    return !(cos_theta_2 < 0.);                                       // :74
}
// The same in two halves, for render_tile's per-lane kernels (the others, the query and the shading units keep the whole above,
// and compile as before).  The FATE -- does the ray exist, and through which side of the surface does it leave -- is known after a
// dozen instructions; the RAY costs a root, a normalisation, two dots and the offset origin.  One behind the other they are
// refract_child's operations in refract_child's order; the per-lane kernels form the ray only where it is walked or its
// computed dot is needed (DESIGN.md section 4, "early child fates").
// `has`: the ray exists (:74); `flip`: the incident ray runs along the normal (:60-68: then c = -c, normal = -normal) -- the
// refracted ray leaves into the side the un-flipped normal points to, else into the other one.
struct RefractFate { double r, c, cos_theta_2; bool flip, has; };
// From this cos_theta_2 on, with r no larger than this, the sign of the computed d . normal is the predicted one (DESIGN.md
// section 4: before the normalisation the dot is -+sqrt(cos_theta_2) to within 3.6e-5 for a normal that is unit to 1e-6, what a
// flagged primitive's is; tests/test_refract_fate.py).
#define RM_FATE_COS2_MIN 0x1p-16
#define RM_FATE_R_MAX 16.
__device__ __forceinline__ RefractFate refract_fate(V3 incident, const Surface &s, double ri, double inv_ri) {
    RefractFate f;
    const double c0 = -dot(s.normal, incident);                       // optics.rs:57
    f.flip = c0 < 0.;                                                 // :60-68
    f.r = f.flip ? ri : inv_ri;
    f.c = f.flip ? -c0 : c0;
    f.cos_theta_2 = 1. - f.r * f.r * (1. - f.c * f.c);
    f.has = !(f.cos_theta_2 < 0.);                                    // :74
    return f;
}
__device__ __forceinline__ void refract_ray(V3 incident, const Surface &s, const RefractFate &f, bool glass, V3 &o, V3 &d, double &dn RM_SUS_PARAM) {
    (void)glass;
    // (RM_CHECKED: the root without its scaling, as the discriminants' -- a cos_theta_2 that is not zero is 2^-53 at least)
#ifdef RM_AB_FATE_SCALED_ROOT   // (A/B build: the early fates with the compiler's own root)
    const double k = f.r * f.c - __builtin_sqrt(f.cos_theta_2);
#else
    const double k = f.r * f.c - RM_SQRT_DISCRIMINANT(f.cos_theta_2);
#endif
    // (under total reflection k is NaN and there is no such ray: its lanes' flags do not count)
    d = RM_NORMALIZED(scaled(incident, f.r) + scaled(s.normal, f.flip ? -k : k), glass & f.has);   // :78-79 (flipped normal * k)
    dn = dot(d, s.normal);                                            // d . flipped normal = -(d . normal) when flipped
    const bool along = f.flip ? (dn < 0.) : (dn > 0.);                // :82 `dir.dot(normal) > 0` with the flipped normal
    o = s.point + scaled(s.normal, (along != f.flip) ? 1e-4 : -1e-4); // :82-86: point +- flipped normal * 1e-4
}
__device__ __forceinline__ bool refract_child(V3 incident, const Surface &s, double ri, double inv_ri, bool glass, V3 &o, V3 &d RM_SUS_PARAM) {
    double dn;
    return refract_child(incident, s, ri, inv_ri, glass, o, d, dn RM_SUS_ARG);
}

}  // namespace RM_FLAVOR_NS
