// rm_image.cpp -- builds the device image of a scene description (rm_image.hpp; the layout: rm_internal.h).  Host
// arithmetic only, no HIP header in sight: the CPU tests and the sanitizer program reach all of it.  What the kernels'
// culls and shortcuts rest on is decided here: the bounds' margins, the "never hit" radius of -1, the edge records for
// convex lists only, the occluder masks, the empty half-spaces in the glass word and the checked numerics' verdict.
// Built with -ffp-contract=off: an image is the same words whichever compiler builds this file.
#include "rm_image.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "rm_bvh.hpp"
#include "rm_plan.hpp"

namespace {

// RM_ERR_SCENE_LIMIT is left for what the blob's 32-bit word offsets cannot address.
constexpr uint64_t RM_SCENE_MAX_WORDS = 0xFFFFFFF0ull;
// A hierarchy is built over a kind once it has this many primitives (below, the flat walk
// is as fast: the demo scene has 4 spheres).
constexpr size_t RM_BVH_MIN_SPHERES = 16, RM_BVH_MIN_TRIANGLES = 12;
// The occluder masks and the empty half-spaces are built for scenes of up to this many pids (a bit per pid).
constexpr uint32_t RM_SHADOW_MASK_MAX_PRIMS = 64u;
// empty_sides[pid]: bit 0 -- nothing of the scene lies on the side of the polygon's / triangle's plane its normal points to,
// bit 1 -- nothing on the other side (spheres, and anything in doubt: 0)
constexpr unsigned RM_EMPTY_SIDE_POS = 1u, RM_EMPTY_SIDE_NEG = 2u;
// ... which the render reads only while the camera's L1 norm is at most this (a hit point then rounds far below the 1e-4 by
// which a child ray starts off its surface)
constexpr double RM_EMPTY_SIDES_CAMERA_MAX = 1e9;

inline uint64_t pack_u32x2(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }

inline rm_vec3 v3(double x, double y, double z) { return rm_vec3{x, y, z}; }
inline rm_vec3 operator-(rm_vec3 a, rm_vec3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline rm_vec3 scaled(rm_vec3 a, double s) { return v3(a.x * s, a.y * s, a.z * s); }
inline double dot(rm_vec3 a, rm_vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline rm_vec3 cross(rm_vec3 a, rm_vec3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

// ---- the shadow rays' occluder masks (rm_internal.h: occ; rm_trace.inc any_hit2) ----------------------
// A shadow ray of a hit on primitive P towards light L (renderer.rs:163-174) starts 1e-3 of the normal off
// the hit point p -- within shadow_rho of it -- and runs along normalize(L - p); the reference's test
// (shapes.rs:92) reports a hit at ANY distance, beyond the light too.  With p in P's bounding sphere (c, r)
// every such ray stays within shadow_rho of
//   (H) the hull of that sphere and L -- the part up to the light -- and
//   (N) the cone beyond L: apex L, axis L - c, half-angle asin(r / |L - c|).
// Both lie in the double cone with apex L around a = (c - L) / |c - L|, (H) below (x - L).a <= |c - L| + r.
// A primitive Q whose hit points all lie farther than shadow_rho from (H) and from (N) cannot occlude any
// such ray, and its bit stays clear.  Q's bounding sphere against the double cone and that cap decides
// first; triangles and quads whose sphere is not out -- a large floor's meets most cones -- are tested
// again by their lifted vertices (the hull of their hit points): Q is out when some plane has all of them
// beyond (H) and some plane has all of them beyond (N).  The planes tried: normal a, the coordinate axes,
// Q's own plane, and the planes through L and each of Q's edges, both ways round.
// Margins: 1e-7 of the coordinates' magnitude on top of the bounds' own inflation, 1e-9 on the cone's
// sine -- far beyond the rounding of the kernel's tests and of the hit point itself (while the camera
// stays within 1e6 scene sizes: camera_limit, the render drops the table beyond).  P's own bit is always set; a light
// inside or on P's sphere, or anything that is not a finite number, sets every bit.  Primitives that can
// never be hit (radius -1, planar_bounds) are in no mask.

// planes of normal n through L: all of Q's vertices w (relative to L) beyond (H) -- the hull of the sphere
// (cl = c - L, r) and the origin -- and beyond (N), the cone (apex 0, axis -a, sine sin_t), by `marg`
struct PlaneSep { bool h = false, n = false; };
inline void try_plane(PlaneSep &sep, rm_vec3 n, const rm_vec3 *w, uint32_t nv, rm_vec3 cl, double r, rm_vec3 a, double sin_t,
                      double marg) {
    const double len = std::sqrt(dot(n, n));
    if (!(len > 1e-150) || !std::isfinite(len)) return;
    n = scaled(n, 1. / len);
    for (int sign = 0; sign < 2; sign++, n = scaled(n, -1.)) {
        double lo = HUGE_VAL;
        for (uint32_t i = 0; i < nv; i++) lo = std::fmin(lo, dot(w[i], n));
        if (!std::isfinite(lo)) continue;
        sep.h = sep.h || lo > std::fmax(0., dot(cl, n) + r) + marg;
        sep.n = sep.n || (dot(a, n) >= sin_t + 1e-9 && lo > marg);
    }
}

void rm_build_shadow_masks(const double *blob, const rm_dev_header &H, unsigned long long *occ) {
    const uint32_t n = H.n_spheres + H.n_polygons + H.n_triangles, nl = H.n_lights;
    const unsigned long long all = n >= 64u ? ~0ull : ((1ull << n) - 1ull);
    const double rho = H.shadow_rho;
    auto finite3 = [](rm_vec3 v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); };
    auto mag = [](rm_vec3 v) { return std::fabs(v.x) + std::fabs(v.y) + std::fabs(v.z); };
    for (uint32_t l = 0; l < nl; l++) {
        const double *lw = blob + H.off_lights + RM_LIGHT_WORDS * l;
        const rm_vec3 L = v3(lw[0], lw[1], lw[2]);
        for (uint32_t P = 0; P < n; P++) {
            unsigned long long &m = occ[(size_t)P * nl + l];
            m = all;
            const double *bp = blob + H.off_bounds + 4u * P;
            const rm_vec3 c = v3(bp[0], bp[1], bp[2]);
            if (!(bp[3] >= 0.) || !std::isfinite(bp[3]) || !finite3(c) || !finite3(L) || !(rho >= 0.) || !std::isfinite(rho)) continue;
            const double tol = 1e-7 * (1. + mag(L) + mag(c) + bp[3]);
            const double r = bp[3] + tol;
            const rm_vec3 cl = c - L;
            const double D = std::sqrt(dot(cl, cl));
            if (!(D > r * (1. + 1e-6) + rho + tol)) continue;         // the light inside or on P's sphere
            const rm_vec3 a = scaled(cl, 1. / D);
            const double sin_t = std::fmin(1., r / D * (1. + 1e-9) + 1e-9);
            const double cos_t = std::sqrt(std::fmax(0., 1. - sin_t * sin_t)) * (1. - 1e-9);
            const double cap = D + r;                                 // (H) ends here along a
            unsigned long long keep = 1ull << P;
            for (uint32_t Q = 0; Q < n; Q++) {
                if (Q == P) continue;
                const double *bq = blob + H.off_bounds + 4u * Q;
                if (bq[3] < 0.) continue;                             // never hit
                const rm_vec3 cq = v3(bq[0], bq[1], bq[2]);
                if (!std::isfinite(bq[3]) || !finite3(cq)) { keep |= 1ull << Q; continue; }
                const double marg = rho + tol + 1e-7 * (mag(cq) + bq[3]);
                const double R = bq[3] + marg;
                const rm_vec3 v = cq - L, x = cross(v, a);
                const double h = dot(v, a), q = std::sqrt(dot(x, x));   // along the axis, off it
                bool out = (q * cos_t - std::fabs(h) * sin_t > R) || (h - R > cap);
                if (!out && Q >= H.n_spheres) {
                    const double *pl = blob + H.off_planar + 16u * (Q - H.n_spheres);
                    const uint32_t nv = pl[12] == 3. ? 3u : pl[12] == 4. ? 4u : 0u;   // 0: no lifted vertices
                    rm_vec3 w[4];
                    bool fin = nv != 0u;
                    for (uint32_t i = 0; i < nv; i++) { w[i] = v3(pl[3 * i], pl[3 * i + 1], pl[3 * i + 2]) - L; fin = fin && finite3(w[i]); }
                    if (fin) {
                        PlaneSep sep;
                        try_plane(sep, a, w, nv, cl, r, a, sin_t, marg);
                        try_plane(sep, v3(1., 0., 0.), w, nv, cl, r, a, sin_t, marg);
                        try_plane(sep, v3(0., 1., 0.), w, nv, cl, r, a, sin_t, marg);
                        try_plane(sep, v3(0., 0., 1.), w, nv, cl, r, a, sin_t, marg);
                        try_plane(sep, cross(w[1] - w[0], w[2] - w[0]), w, nv, cl, r, a, sin_t, marg);
                        for (uint32_t i = 0; i < nv; i++) try_plane(sep, cross(w[i], w[(i + 1u) % nv]), w, nv, cl, r, a, sin_t, marg);
                        out = sep.h && sep.n;
                    }
                }
                if (!out) keep |= 1ull << Q;
            }
            m = keep;
        }
    }
}

// ---- empty half-spaces of the planar primitives (rm_internal.h: the glass word; rm_render_kernel.inc render_tile) --------
// A child ray of a hit on a polygon or triangle P (optics.rs:8-89) starts 1e-4 of P's normal off the hit point, on the side
// its direction d points to (:41-45, :82-86: the side sign(d . normal)), and never comes back to P's plane.  Where every other
// primitive lies strictly on the OTHER side of that plane such a ray can hit nothing: not P -- its test rejects a ray that
// runs away from its plane on the sign of the very same dot product -- and nothing else.  The kernel then adds what the
// ray's own step would have added, weight x background, and does not walk it.
// sides[P] bit 0: the side P's normal points to is empty, bit 1: the other one.  A primitive Q is on the other side when its
// lifted vertices (the hull of its hit points) all are, or its bounding sphere is, by
//   1e-4 + shadow_rho + 1e-7 x (1 + the coordinates' magnitudes)
// -- the scale of the occluder masks' margins, far beyond the rounding of a hit point.  Anything that is not a finite number,
// a normal that is not unit to 1e-6, a coordinate of 1e6 and more (the hit points' rounding must stay far below the 1e-4
// offset) leaves both bits clear.  Primitives that can never be hit (radius -1) are ignored and get no bits themselves.
void rm_build_empty_sides(const double *blob, const rm_dev_header &H, unsigned char *sides) {
    const uint32_t n = H.n_spheres + H.n_polygons + H.n_triangles;
    const double rho = H.shadow_rho, big = 1e6;
    auto finite3 = [](rm_vec3 v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); };
    auto mag = [](rm_vec3 v) { return std::fabs(v.x) + std::fabs(v.y) + std::fabs(v.z); };
    for (uint32_t P = 0; P < n; P++) sides[P] = 0;
    if (!(rho >= 0.) || !std::isfinite(rho)) return;
    for (uint32_t P = H.n_spheres; P < n; P++) {
        const double *rec = P < H.n_spheres + H.n_polygons ? blob + H.off_polygons + RM_POLYGON_WORDS * (P - H.n_spheres)
                                                           : blob + H.off_triangles + RM_TRIANGLE_WORDS * (P - H.n_spheres - H.n_polygons);
        const rm_vec3 nrm = v3(rec[0], rec[1], rec[2]), pp = v3(rec[3], rec[4], rec[5]);
        const double *bp = blob + H.off_bounds + 4u * P;
        const rm_vec3 c = v3(bp[0], bp[1], bp[2]);
        if (!(bp[3] >= 0.) || !std::isfinite(bp[3]) || !finite3(c) || !finite3(nrm) || !finite3(pp)) continue;
        if (!(std::fabs(std::sqrt(dot(nrm, nrm)) - 1.) <= 1e-6)) continue;
        if (!(mag(c) + bp[3] < big) || !(mag(pp) < big)) continue;
        bool pos = true, neg = true;                                  // the side the normal points to / the other one is empty
        for (uint32_t Q = 0; Q < n && (pos || neg); Q++) {
            if (Q == P) continue;
            const double *bq = blob + H.off_bounds + 4u * Q;
            if (bq[3] < 0.) continue;                                 // never hit
            const rm_vec3 cq = v3(bq[0], bq[1], bq[2]);
            if (!std::isfinite(bq[3]) || !finite3(cq) || !(mag(cq) + bq[3] < big)) { pos = neg = false; break; }
            // by its bounding sphere
            const double marg = 1e-4 + rho + 1e-7 * (1. + mag(pp) + mag(cq) + bq[3]);
            const double h = dot(cq - pp, nrm);
            bool below = h + bq[3] < -marg, above = h - bq[3] > marg;
            // ... or by its lifted vertices, all of them
            if (!below && !above && Q >= H.n_spheres) {
                const double *pl = blob + H.off_planar + 16u * (Q - H.n_spheres);
                const uint32_t nv = pl[12] == 3. ? 3u : pl[12] == 4. ? 4u : 0u;   // 0: no lifted vertices
                bool lo = nv != 0u, hi = nv != 0u;
                for (uint32_t i = 0; i < nv; i++) {
                    const rm_vec3 w = v3(pl[3 * i], pl[3 * i + 1], pl[3 * i + 2]);
                    if (!finite3(w) || !(mag(w) < big)) { lo = hi = false; break; }
                    const double mw = 1e-4 + rho + 1e-7 * (1. + mag(pp) + mag(w));
                    const double hw = dot(w - pp, nrm);
                    lo = lo && hw < -mw;
                    hi = hi && hw > mw;
                }
                below = lo; above = hi;
            }
            pos = pos && below;
            neg = neg && above;
        }
        sides[P] = (unsigned char)((pos ? RM_EMPTY_SIDE_POS : 0u) | (neg ? RM_EMPTY_SIDE_NEG : 0u));
    }
}
// Checked numerics (rm_trace.inc RM_CHECKED; the bounds: rm_plan.hpp): a scene is rendered by the exact code alone when any
// coordinate, radius or light word of its description is not finite or beyond RM_CHECKED_COORD_MAX in magnitude --
// within it no intermediate of a sphere test overflows into a NaN whose payload the two square-root sequences might carry
// differently -- or a sphere's radius_square lies outside the range in which the discriminant's root needs no scaling.
// (The camera is the launch's: rm_camera_update can set it to anything, and the plan looks at the one a launch carries.)
bool scene_exact_only(const rm_scene_desc *d) {
    bool ok = true;
    auto v3 = [&](const rm_vec3 &v) { ok = ok && rm_checked_coord_ok(v.x) && rm_checked_coord_ok(v.y) && rm_checked_coord_ok(v.z); };
    for (uint32_t i = 0; i < d->n_spheres; i++) {
        v3(d->spheres[i].center);
        const double r2 = d->spheres[i].radius_square;
        ok = ok && r2 >= RM_CHECKED_R2_MIN && r2 <= RM_CHECKED_R2_MAX && rm_checked_coord_ok(r2);
    }
    for (uint32_t i = 0; i < d->n_polygons; i++) { v3(d->polygons[i].plane_normal); v3(d->polygons[i].plane_point); }
    for (uint32_t i = 0; i < d->n_polygon_vertices; i++) v3(d->polygon_vertices[i]);
    for (uint32_t i = 0; i < d->n_triangles; i++) {
        const rm_triangle &t = d->triangles[i];
        v3(t.normal); v3(t.center);
        for (const rm_vec3 &v : t.vertices) v3(v);
    }
    for (uint32_t i = 0; i < d->n_lights; i++) {
        v3(d->lights[i].position); v3(d->lights[i].color);
        ok = ok && rm_checked_coord_ok(d->lights[i].intensity);
    }
    return !ok;
}

// The primitives of one kind in the order the image stores them.
struct kind_list {
    std::vector<uint32_t> src;         // indices into the description's array of the kind
    std::vector<uint32_t> key;         // ordinal in flattened Scene.shapes order
};

// One image in the making: the steps below run in the order rm_build_image calls them.
struct image_builder {
    const rm_scene_desc *const d;
    rm_image &img;
    rm_dev_header &H;
    std::vector<double> &blob;
    std::string &error;
    kind_list spheres, polygons, triangles;
    std::vector<uint32_t> ordinal_shape;   // ordinal -> (index into Scene.shapes, triangle index inside the Obj)
    std::vector<uint32_t> keys;            // the three kinds' keys back to back: keys[pid]
    rm_bvh bvh_s, bvh_t;
    uint32_t n_prims = 0, n_pverts = 0, n_groups = 0;
    double max_normal = 1.;                // sphere normals are unit (sphere.rs:58)

    image_builder(const rm_scene_desc *desc, rm_image &image, std::string &err) : d(desc), img(image), H(image.H), blob(image.blob), error(err) {}

    rm_status fail(rm_status st, const char *msg) { error = msg; return st; }

    // ---- regroup Scene.shapes by kind, remembering list order for ties ----
    rm_status regroup() {
        uint32_t ordinal = 0;
        for (uint32_t i = 0; i < d->n_shapes; i++) {
            const rm_shape_ref &r = d->shapes[i];
            switch (r.kind) {
            case RM_SHAPE_SPHERE:
            case RM_SHAPE_POLYGON: {
                const bool sphere = r.kind == RM_SHAPE_SPHERE;
                if (r.first >= (sphere ? d->n_spheres : d->n_polygons) || r.count != 1)
                    return fail(RM_ERR_INVALID_ARG, sphere ? "rm_scene_upload: bad sphere ref" : "rm_scene_upload: bad polygon ref");
                kind_list &list = sphere ? spheres : polygons;
                list.src.push_back(r.first); list.key.push_back(ordinal++);
                ordinal_shape.insert(ordinal_shape.end(), {i, 0u});
                break;
            }
            case RM_SHAPE_MESH:
                if ((uint64_t)r.first + r.count > d->n_triangles) return fail(RM_ERR_INVALID_ARG, "rm_scene_upload: bad mesh ref");
                for (uint32_t t = 0; t < r.count; t++) {
                    triangles.src.push_back(r.first + t); triangles.key.push_back(ordinal++);
                    ordinal_shape.insert(ordinal_shape.end(), {i, t});
                }
                break;
            default:
                return fail(RM_ERR_INVALID_ARG, "rm_scene_upload: unknown shape kind");
            }
        }
        return RM_OK;
    }

    // A hierarchy over the primitives of one kind (rm_bvh.hpp): they are re-ordered into leaf order; their list-order
    // keys travel with them
    template <class BoxOf>
    static rm_bvh build_hierarchy(kind_list &list, uint32_t leaf_size, BoxOf box_of) {
        std::vector<rm_aabb> boxes(list.src.size());
        for (size_t i = 0; i < boxes.size(); i++) box_of(list.src[i], boxes[i]);
        rm_bvh bvh = rm_build_bvh(boxes, leaf_size);
        kind_list leaf_order{std::vector<uint32_t>(boxes.size()), std::vector<uint32_t>(boxes.size())};
        for (size_t k = 0; k < boxes.size(); k++) { leaf_order.src[k] = list.src[bvh.order[k]]; leaf_order.key[k] = list.key[bvh.order[k]]; }
        list = std::move(leaf_order);
        return bvh;
    }

    // ---- hierarchies over the spheres and the mesh triangles ----
    void build_hierarchies() {
        if (spheres.src.size() >= RM_BVH_MIN_SPHERES)
            bvh_s = build_hierarchy(spheres, 4, [&](uint32_t src, rm_aabb &box) {
                const rm_sphere &sp = d->spheres[src];
                const double r = std::sqrt(sp.radius_square) * (1. + 1e-12);
                const double c[3] = {sp.center.x, sp.center.y, sp.center.z};
                for (int a = 0; a < 3; a++) { box.lo[a] = c[a] - r; box.hi[a] = c[a] + r; }
            });
        if (triangles.src.size() >= RM_BVH_MIN_TRIANGLES)
            bvh_t = build_hierarchy(triangles, 2, [&](uint32_t src, rm_aabb &box) {
                box.reset();
                for (const rm_vec3 &v : d->triangles[src].vertices) {
                    const double c[3] = {v.x, v.y, v.z};
                    for (int a = 0; a < 3; a++) { box.lo[a] = std::min(box.lo[a], c[a]); box.hi[a] = std::max(box.hi[a], c[a]); }
                }
            });
    }

    // ---- the keys in pid order, the counts, and the queries' way back from a device primitive to the reference's
    // (shape, element): through the same keys ----
    void number_pids() {
        keys.insert(keys.end(), spheres.key.begin(), spheres.key.end());
        keys.insert(keys.end(), polygons.key.begin(), polygons.key.end());
        keys.insert(keys.end(), triangles.key.begin(), triangles.key.end());
        bool ordered = true;
        for (size_t i = 1; i < keys.size(); i++) ordered = ordered && keys[i - 1] < keys[i];
        img.pid_map.assign(2u * keys.size(), 0u);
        for (size_t q = 0; q < keys.size(); q++) {
            img.pid_map[2u * q] = ordinal_shape[2u * keys[q]];
            img.pid_map[2u * q + 1u] = ordinal_shape[2u * keys[q] + 1u];
        }
        H.n_spheres = (uint32_t)spheres.src.size();
        H.n_polygons = (uint32_t)polygons.src.size();
        H.n_triangles = (uint32_t)triangles.src.size();
        H.n_lights = d->n_lights;
        n_prims = H.n_spheres + H.n_polygons + H.n_triangles;
        H.list_ordered = ordered ? 1u : 0u;
    }

    // ---- the offsets of every section, and the zero-filled blob ----
    rm_status lay_out() {
        for (uint32_t src : polygons.src) {
            const rm_polygon &p = d->polygons[src];
            if (p.n_vertices < 3 || (uint64_t)p.first_vertex + p.n_vertices > d->n_polygon_vertices)
                return fail(RM_ERR_INVALID_ARG, "rm_scene_upload: bad polygon vertex range");
            n_pverts += p.n_vertices;
        }
        // 32-bit word offsets: refuse scenes they cannot address
        const uint64_t need_words = (uint64_t)H.n_spheres * RM_SPHERE_WORDS + (uint64_t)H.n_polygons * RM_POLYGON_WORDS +
                                    ((uint64_t)n_pverts + 1u) * RM_PVERT_WORDS + (uint64_t)H.n_triangles * RM_TRIANGLE_WORDS +
                                    (uint64_t)n_prims * (RM_MATERIAL_WORDS + 1u + 4u + 16u + 1u) + (uint64_t)H.n_lights * RM_LIGHT_WORDS +
                                    bvh_s.nodes.size() + bvh_t.nodes.size() + 256u;
        if (need_words > RM_SCENE_MAX_WORDS)
            return fail(RM_ERR_SCENE_LIMIT, "rm_scene_upload: scene exceeds the 32 GiB the device layout can address");
        uint32_t off = 0;
        auto take = [&](uint32_t words) { uint32_t o = off; off += (words + 1u) & ~1u; return o; };
        H.off_spheres = take(H.n_spheres * RM_SPHERE_WORDS);
        H.off_polygons = take(H.n_polygons * RM_POLYGON_WORDS);
        H.off_pverts = take((n_pverts + 1u) * RM_PVERT_WORDS);   // +1: the loops fetch four vertices at a time
        H.off_triangles = take(H.n_triangles * RM_TRIANGLE_WORDS);
        H.off_materials = take(n_prims * RM_MATERIAL_WORDS);
        H.off_lights = take(H.n_lights * RM_LIGHT_WORDS);
        H.off_keys = take((n_prims + 1u) / 2u);
        H.off_bounds = take(n_prims * 4u);
        H.off_planar = take((H.n_polygons + H.n_triangles) * 16u);
        n_groups = (n_prims + 63u) / 64u;
        H.off_groups = (n_groups >= 3u && n_groups <= 64u) ? take(n_groups * 4u) : 0u;
        // The wave's hierarchy stack holds 64 entries, one parked sibling per level: the builder
        // keeps every tree under RM_BVH_MAX_DEPTH levels (rm_bvh.hpp); a tree that is deeper all
        // the same is not walked (its primitives keep their leaf order and are walked flat).
        if (bvh_s.depth > RM_BVH_MAX_DEPTH) bvh_s.nodes.clear();
        if (bvh_t.depth > RM_BVH_MAX_DEPTH) bvh_t.nodes.clear();
        H.off_bvh_spheres = bvh_s.nodes.empty() ? 0u : take((uint32_t)bvh_s.nodes.size());
        H.off_bvh_triangles = bvh_t.nodes.empty() ? 0u : take((uint32_t)bvh_t.nodes.size());
        take(64u);                                               // batch loads may read past the last record
        H.total_words = off;
        blob.assign(H.total_words ? H.total_words : 2, 0.);
        return RM_OK;
    }

    void put_material(uint32_t pid, const rm_reflectance &r) {
        double *m = &blob[H.off_materials + RM_MATERIAL_WORDS * pid];
        m[0] = r.diffusion;
        m[1] = r.diffuse_color.x; m[2] = r.diffuse_color.y; m[3] = r.diffuse_color.z;
        m[4] = r.specular; m[5] = r.specular_exponent;
        m[6] = r.reflection; m[7] = r.refractive_index;
        m[8] = r.is_glass_like ? 1. : 0.;
        m[9] = 1. / r.refractive_index;   // reflect_child / refract_child read it: one IEEE division here, the bits of the device's per ray
        // specular_pow<POW_INTEGER> applies when pow(x, y) is a plain integer power for every material
        const double y = r.specular_exponent;
        img.integer_exponents = img.integer_exponents && (y >= 0. && y <= 1048576. && y == std::floor(y));
    }

    // Bounding sphere of everything of primitive `pid` a ray can hit, for the bundle cull
    // (rm_trace.inc): inflated by 1e-7 relative + 1e-9 of the coordinates' magnitude -- far
    // beyond the rounding of any hit test, so a primitive some ray hits is never culled.
    // Anything that is not a finite number makes the primitive a candidate for every bundle.
    void put_bounds(uint32_t pid, double cx, double cy, double cz, double r) {
        double *w = &blob[H.off_bounds + 4u * pid];
        const double mag = std::fabs(cx) + std::fabs(cy) + std::fabs(cz);
        double rr = r * (1. + 1e-7) + 1e-9 * (1. + mag);
        if (!(rr >= 0.) || !std::isfinite(rr) || !std::isfinite(mag)) { cx = cy = cz = 0.; rr = std::numeric_limits<double>::infinity(); }
        w[0] = cx; w[1] = cy; w[2] = cz; w[3] = rr;
    }

    // A planar primitive is hit where the ray meets the plane (point, normal) AND the x, y of
    // that point pass the 2-D edge tests (polygon.rs:54-56, triangle.rs:69-77), i.e. lie in
    // the convex hull of the vertices' x, y: the hit points are the hull of the vertices
    // LIFTED onto that plane along z -- the vertices themselves when they are coplanar with
    // it, as they are for everything the reference's constructors build.  That holds for ANY vertex
    // list, convex or not: a point that is to the left of every edge is wound round by the closed
    // line at least once, so it lies inside the line's hull (bow ties, darts, clockwise lists:
    // tests/test_gpu_grazing.py test_odd_vertex_lists).
    void planar_bounds(uint32_t pid, const rm_vec3 &n, const rm_vec3 &pp, const rm_vec3 *v, uint32_t nv) {
        max_normal = std::max(max_normal, std::sqrt(n.x * n.x + n.y * n.y + n.z * n.z));
        double *pl = &blob[H.off_planar + 16u * (pid - H.n_spheres)];   // zero-filled: count 0 = no edge test
        // The inside test reads only x and y (polygon.rs:54-56): with every vertex at the SAME x
        // (or the same y) its cross products are differences of the same rounded products, sum to
        // zero exactly and can never all be positive -- the primitive is never hit (the floor and
        // ceiling of the Cornell box, any wall along z).  Radius -1: the cull drops it outright.
        bool same_x = true, same_y = true;
        for (uint32_t i = 1; i < nv; i++) { same_x = same_x && v[i].x == v[0].x; same_y = same_y && v[i].y == v[0].y; }
        // Likewise two CONSECUTIVE vertices with the same x and the same y (a wall along z cut into triangles:
        // the red wall of the Cornell box): the cross product of that edge is x y' - y x' with (x, y) == (x', y')
        // bit for bit -- the same product twice, exactly zero, never > 0 -- for every hit point.
        bool twin_edge = false;
        for (uint32_t i = 0; i < nv; i++) {
            const rm_vec3 &p = v[i], &q = v[(i + 1u) % nv];
            twin_edge = twin_edge || (p.x == q.x && p.y == q.y);
        }
        if (same_x || same_y || twin_edge) {
            double *w = &blob[H.off_bounds + 4u * pid];
            w[0] = w[1] = w[2] = 0.; w[3] = -1.;
            return;
        }
        if (!(std::fabs(n.z) > 1e-12 * (std::fabs(n.x) + std::fabs(n.y) + std::fabs(n.z)))) {
            // plane along z: the x, y of its points are a line; no finite bound holds the lifted hull
            put_bounds(pid, 0., 0., 0., std::numeric_limits<double>::infinity());
            return;
        }
        std::vector<rm_vec3> lifted(nv);
        double cx = 0., cy = 0., cz = 0.;
        for (uint32_t i = 0; i < nv; i++) {
            const double z = pp.z - (n.x * (v[i].x - pp.x) + n.y * (v[i].y - pp.y)) / n.z;
            lifted[i] = rm_vec3{v[i].x, v[i].y, z};
            cx += v[i].x; cy += v[i].y; cz += z;
        }
        cx /= nv; cy /= nv; cz /= nv;
        double r2 = 0.;
        for (const rm_vec3 &q : lifted) r2 = std::max(r2, (q.x - cx) * (q.x - cx) + (q.y - cy) * (q.y - cy) + (q.z - cz) * (q.z - cz));
        put_bounds(pid, cx, cy, cz, std::sqrt(r2));
        // the lifted vertices for the cull's edge test (triangles and quads; a triangle
        // repeats its first vertex so that edge 2-3 closes it)
        bool with_edges = nv == 3u || nv == 4u;
        for (const rm_vec3 &q : lifted) with_edges = with_edges && std::isfinite(q.x) && std::isfinite(q.y) && std::isfinite(q.z);
        // The edge test takes the side of an edge's plane that holds the vertices' mean for the inner one (rm_trace.inc
        // cull_edge): true of a convex list of either winding, not of any list -- a dart's mean lies on the OUTER side
        // of the edges at its reflex vertex, and the bundles that hit it between them would be dropped
        // (tests/test_gpu_grazing.py).  Only lists whose x, y turn one way at every vertex, strictly, get the record;
        // the others keep their bounding sphere alone.
        int turn = 0;
        for (uint32_t i = 0; i < nv && with_edges; i++) {
            const rm_vec3 &p = lifted[i], &q = lifted[(i + 1u) % nv];
            for (uint32_t k = 0; k < nv && with_edges; k++) {
                if (k == i || k == (i + 1u) % nv) continue;
                const double c = (q.x - p.x) * (lifted[k].y - p.y) - (q.y - p.y) * (lifted[k].x - p.x);
                const int sgn = c > 0. ? 1 : c < 0. ? -1 : 0;
                with_edges = sgn != 0 && (turn == 0 || sgn == turn);
                turn = sgn;
            }
        }
        if (with_edges) {
            for (uint32_t i = 0; i < 4u; i++) {
                const rm_vec3 &q = lifted[i < nv ? i : 0u];
                pl[3 * i] = q.x; pl[3 * i + 1] = q.y; pl[3 * i + 2] = q.z;
            }
            pl[12] = (double)nv;
        }
    }

    // ---- the sphere, polygon and triangle records, each with its material, its bounds and (planar ones) its lifted vertices;
    // the light records, the keys and the hierarchies' nodes ----
    void write_records() {
        img.integer_exponents = true;
        uint32_t pid = 0;
        for (uint32_t i = 0; i < H.n_spheres; i++, pid++) {
            const rm_sphere &s = d->spheres[spheres.src[i]];
            double *w = &blob[H.off_spheres + RM_SPHERE_WORDS * i];
            w[0] = s.center.x; w[1] = s.center.y; w[2] = s.center.z; w[3] = s.radius_square;
            put_material(pid, s.reflectance);
            put_bounds(pid, s.center.x, s.center.y, s.center.z, std::sqrt(s.radius_square));
        }
        uint32_t pv = 0;
        for (uint32_t i = 0; i < H.n_polygons; i++, pid++) {
            const rm_polygon &p = d->polygons[polygons.src[i]];
            double *w = &blob[H.off_polygons + RM_POLYGON_WORDS * i];
            w[0] = p.plane_normal.x; w[1] = p.plane_normal.y; w[2] = p.plane_normal.z;
            w[3] = p.plane_point.x; w[4] = p.plane_point.y; w[5] = p.plane_point.z;
            const uint64_t packed = pack_u32x2(pv, p.n_vertices);
            std::memcpy(&w[6], &packed, sizeof packed);
            w[7] = 0.;
            for (uint32_t v = 0; v < p.n_vertices; v++, pv++) {
                const rm_vec3 &q = d->polygon_vertices[p.first_vertex + v];
                blob[H.off_pverts + RM_PVERT_WORDS * pv] = q.x;
                blob[H.off_pverts + RM_PVERT_WORDS * pv + 1] = q.y;
                // the first four also travel in the record: one fetch per polygon, not two dependent ones
                if (v < 4) { w[8 + 2 * v] = q.x; w[9 + 2 * v] = q.y; }
            }
            put_material(pid, p.reflectance);
            planar_bounds(pid, p.plane_normal, p.plane_point, &d->polygon_vertices[p.first_vertex], p.n_vertices);
        }
        for (uint32_t i = 0; i < H.n_triangles; i++, pid++) {
            const rm_triangle &t = d->triangles[triangles.src[i]];
            double *w = &blob[H.off_triangles + RM_TRIANGLE_WORDS * i];
            w[0] = t.normal.x; w[1] = t.normal.y; w[2] = t.normal.z;
            w[3] = t.center.x; w[4] = t.center.y; w[5] = t.center.z;
            for (int v = 0; v < 3; v++) { w[6 + 2 * v] = t.vertices[v].x; w[7 + 2 * v] = t.vertices[v].y; }
            put_material(pid, t.reflectance);
            planar_bounds(pid, t.normal, t.center, t.vertices, 3u);
        }
        // renderer.rs:168-172: a shadow ray starts 1e-3 of the normal off the hit point and runs
        // along normalize(light - point): it passes within 1e-3 |normal| of the light
        H.shadow_rho = 1e-3 * max_normal * (1. + 1e-6) + 1e-12;
        for (uint32_t l = 0; l < H.n_lights; l++) {
            const rm_light &lt = d->lights[l];
            double *w = &blob[H.off_lights + RM_LIGHT_WORDS * l];
            w[0] = lt.position.x; w[1] = lt.position.y; w[2] = lt.position.z;
            w[3] = lt.color.x; w[4] = lt.color.y; w[5] = lt.color.z;
            w[6] = lt.intensity; w[7] = 0.;
        }
        if (!keys.empty()) std::memcpy(&blob[H.off_keys], keys.data(), keys.size() * sizeof(uint32_t));
        if (H.off_bvh_spheres) std::memcpy(&blob[H.off_bvh_spheres], bvh_s.nodes.data(), bvh_s.nodes.size() * sizeof(double));
        if (H.off_bvh_triangles) std::memcpy(&blob[H.off_bvh_triangles], bvh_t.nodes.data(), bvh_t.nodes.size() * sizeof(double));
    }

    // The cull's first step in scenes of 3+ steps: a sphere around the bounding spheres of each 64
    // consecutive pids (box centre of the members; primitives that can never be hit -- radius -1 --
    // do not count, a group of nothing else is never visited).
    void write_groups() {
        for (uint32_t g = 0; H.off_groups && g < n_groups; g++) {
            const uint32_t first = g * 64u, last = std::min(n_prims, first + 64u);
            double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
            bool any = false, unbounded = false;
            for (uint32_t q = first; q < last; q++) {
                const double *w = &blob[H.off_bounds + 4u * q];
                if (w[3] < 0.) continue;
                any = true;
                if (!std::isfinite(w[3])) { unbounded = true; continue; }
                for (int c = 0; c < 3; c++) { lo[c] = std::min(lo[c], w[c] - w[3]); hi[c] = std::max(hi[c], w[c] + w[3]); }
            }
            double *o = &blob[H.off_groups + 4u * g];
            if (!any) { o[0] = o[1] = o[2] = 0.; o[3] = -1.; continue; }
            if (unbounded) { o[0] = o[1] = o[2] = 0.; o[3] = std::numeric_limits<double>::infinity(); continue; }
            const double cx = 0.5 * (lo[0] + hi[0]), cy = 0.5 * (lo[1] + hi[1]), cz = 0.5 * (lo[2] + hi[2]);
            double r = 0.;
            for (uint32_t q = first; q < last; q++) {
                const double *w = &blob[H.off_bounds + 4u * q];
                if (w[3] < 0.) continue;
                const double dx = w[0] - cx, dy = w[1] - cy, dz = w[2] - cz;
                r = std::max(r, std::sqrt(dx * dx + dy * dy + dz * dz) + w[3]);
            }
            const double mag = std::fabs(cx) + std::fabs(cy) + std::fabs(cz);
            double rr = r * (1. + 1e-9) + 1e-12 * (1. + mag);
            if (!std::isfinite(rr) || !std::isfinite(mag)) { o[0] = o[1] = o[2] = 0.; rr = std::numeric_limits<double>::infinity(); }
            else { o[0] = cx; o[1] = cy; o[2] = cz; }
            o[3] = rr;
        }
    }

    // the camera beyond which neither table below is used (the hit points' rounding: 1e-7 of the scene's size
    // is the builders' margin), from the coordinates they are built from
    double camera_limit() const {
        double size = 0.;
        for (uint32_t q = 0; q < n_prims; q++) {
            const double *w = &blob[H.off_bounds + 4u * q];
            if (w[3] >= 0.) size = std::fmax(size, std::fabs(w[0]) + std::fabs(w[1]) + std::fabs(w[2]) + w[3]);
        }
        for (uint32_t l = 0; l < H.n_lights; l++) {
            const double *w = &blob[H.off_lights + RM_LIGHT_WORDS * l];
            size = std::fmax(size, std::fabs(w[0]) + std::fabs(w[1]) + std::fabs(w[2]));
        }
        return std::isfinite(size) ? 1e6 * (1. + size) : 0.;
    }

    // The planar primitives' empty half-spaces (rm_build_empty_sides) for scenes of up to 64 pids: a glass-like one carries them in
    // its glass word, which every reader but the plain-walk kernels' render_tile tests for != 0 only.
    void mark_empty_sides() {
        if (n_prims == 0u || n_prims > RM_SHADOW_MASK_MAX_PRIMS) return;
        img.empty_sides.assign(n_prims, 0);
        rm_build_empty_sides(blob.data(), H, img.empty_sides.data());
        bool any = false;
        for (uint32_t q = 0; q < n_prims; q++) {
            double &glass = blob[H.off_materials + RM_MATERIAL_WORDS * q + 8];
            if (glass != 0. && img.empty_sides[q]) {
                glass = 1. + ((img.empty_sides[q] & RM_EMPTY_SIDE_POS) ? 2. : 0.) + ((img.empty_sides[q] & RM_EMPTY_SIDE_NEG) ? 4. : 0.);
                any = true;
            }
        }
        if (any) img.dead_camera_limit = std::fmin(camera_limit(), RM_EMPTY_SIDES_CAMERA_MAX);
    }

    // The shadow rays' occluder masks (rm_build_shadow_masks) for the plain-walk kernels' scenes, behind the
    // image the staged kernels copy (the walks read them with scalar loads): scenes of up to 64 pids.
    void append_occluder_masks() {
        if (n_prims == 0u || n_prims > RM_SHADOW_MASK_MAX_PRIMS || H.n_lights == 0u) return;
        const uint64_t words = (uint64_t)n_prims * H.n_lights;
        if ((uint64_t)H.total_words + words + 2u > RM_SCENE_MAX_WORDS) return;
        H.off_occ = H.total_words;
        blob.resize((size_t)H.total_words + ((words + 1u) & ~1ull), 0.);
        rm_build_shadow_masks(blob.data(), H, reinterpret_cast<unsigned long long *>(&blob[H.off_occ]));
        img.occ_camera_limit = camera_limit();
    }
};

}  // namespace

bool rm_desc_arrays_present(const rm_scene_desc *d) {
    return !((d->n_shapes && !d->shapes) || (d->n_spheres && !d->spheres) || (d->n_polygons && !d->polygons) ||
             (d->n_polygon_vertices && !d->polygon_vertices) || (d->n_triangles && !d->triangles) || (d->n_lights && !d->lights));
}

rm_status rm_build_image(const rm_scene_desc *d, const rm_image_options &opt, rm_image &img, std::string &error) {
    img = rm_image{};
    image_builder b(d, img, error);
    if (!rm_desc_arrays_present(d)) return b.fail(RM_ERR_INVALID_ARG, "rm_scene_upload: NULL array with non-zero count");
    if (rm_status st = b.regroup()) return st;
    if (opt.use_bvh) b.build_hierarchies();
    b.number_pids();
    if (rm_status st = b.lay_out()) return st;
    b.write_records();
    b.write_groups();
    b.mark_empty_sides();
    if (opt.shadow_masks) b.append_occluder_masks();
    img.exact_only = scene_exact_only(d);
    return RM_OK;
}

// ---- test hooks, not part of the ABI: what the upload of `d` builds.  Host work only: no device is needed. ----

// The image of `d` for a hook: its refusal, or that of a NULL argument, goes to the thread's error text.
static rm_status hook_image(const char *who, const rm_scene_desc *d, const void *out, const rm_image_options &opt, rm_image &img) {
    std::string error = std::string(who) + ": NULL argument";
    const rm_status st = (d && out) ? rm_build_image(d, opt, img, error) : RM_ERR_INVALID_ARG;
    if (st) rm_set_host_error(error);
    return st;
}

// tests/test_shadow_masks.py: the occluder masks, with the knob's default.  dims[0] = pids, dims[1] = lights, dims[2] = 1
// where there is a table; then, when there is and cap >= pids x lights, occ[pid * lights + light] and shape_of[pid] = the
// pid's index into Scene.shapes.
extern "C" rm_status rmi_shadow_masks(const rm_scene_desc *d, uint64_t *occ, uint32_t *shape_of, uint32_t cap, uint32_t *dims) {
    rm_image img;
    if (rm_status st = hook_image("rmi_shadow_masks", d, dims, rm_image_options{}, img)) return st;
    const rm_dev_header &H = img.H;
    const uint32_t n = H.n_spheres + H.n_polygons + H.n_triangles;
    dims[0] = n; dims[1] = H.n_lights; dims[2] = H.off_occ ? 1u : 0u;
    if (H.off_occ && occ && shape_of && (uint64_t)n * H.n_lights <= cap) {
        std::memcpy(occ, &img.blob[H.off_occ], (size_t)n * H.n_lights * sizeof(uint64_t));
        for (uint32_t q = 0; q < n; q++) shape_of[q] = img.pid_map[2u * q];
    }
    return RM_OK;
}

// tests/test_dead_children.py: the empty half-spaces.  dims[0] = pids, dims[1] = 1 where there is a table; then, when there
// is and cap >= pids, sides[pid] (RM_EMPTY_SIDE_POS | RM_EMPTY_SIDE_NEG), glass[pid] = the pid's glass word as the kernels
// read it, and shape_of[pid] = the pid's index into Scene.shapes; *camera_limit = the camera beyond which a render does not
// use them.
extern "C" rm_status rmi_empty_sides(const rm_scene_desc *d, uint8_t *sides, double *glass, uint32_t *shape_of, uint32_t cap, uint32_t *dims, double *camera_limit) {
    rm_image img;
    if (rm_status st = hook_image("rmi_empty_sides", d, dims, rm_image_options{}, img)) return st;
    const rm_dev_header &H = img.H;
    const uint32_t n = H.n_spheres + H.n_polygons + H.n_triangles;
    dims[0] = n; dims[1] = img.empty_sides.empty() ? 0u : 1u;
    if (camera_limit) *camera_limit = img.dead_camera_limit;
    if (dims[1] && sides && glass && shape_of && n <= cap) {
        for (uint32_t q = 0; q < n; q++) {
            sides[q] = img.empty_sides[q];
            glass[q] = img.blob[H.off_materials + RM_MATERIAL_WORDS * q + 8];
            shape_of[q] = img.pid_map[2u * q];
        }
    }
    return RM_OK;
}

// tests/test_checked_numerics.py, tests/test_gpu_checked_numerics.py: what the upload decides and builds for the checked
// numerics.  dims[0] = pids, dims[1] = 1 where the scene is exact only; then, when cap >= 10 x pids, the material words of
// every pid.
extern "C" rm_status rmi_upload_numerics(const rm_scene_desc *d, double *materials, uint32_t cap, uint32_t *dims) {
    rm_image img;
    if (rm_status st = hook_image("rmi_upload_numerics", d, dims, rm_image_options{}, img)) return st;
    const uint32_t n = img.H.n_spheres + img.H.n_polygons + img.H.n_triangles;
    dims[0] = n; dims[1] = img.exact_only ? 1u : 0u;
    if (materials && (uint64_t)n * RM_MATERIAL_WORDS <= cap)
        std::memcpy(materials, &img.blob[img.H.off_materials], (size_t)n * RM_MATERIAL_WORDS * sizeof(double));
    return RM_OK;
}

// tests/test_scene_image.py: the whole image.  sizes[0] = the blob's words (the occluder masks behind total_words included),
// sizes[1] = the pid map's; header[19] = rm_dev_header's integer fields in their order; reals[3] = shadow_rho,
// occ_camera_limit, dead_camera_limit; verdicts[2] = exact_only, integer_exponents; then, when blob_cap and map_cap hold
// them, the blob's words bit for bit and the pid map.
extern "C" rm_status rmi_scene_image(const rm_scene_desc *d, uint32_t use_bvh, uint32_t shadow_masks, uint64_t *sizes, uint32_t *header,
                                     double *reals, uint32_t *verdicts, uint64_t *blob, uint64_t blob_cap, uint32_t *pid_map, uint64_t map_cap) {
    rm_image img;
    const bool outs = sizes && header && reals && verdicts;
    if (rm_status st = hook_image("rmi_scene_image", d, outs ? sizes : nullptr, rm_image_options{use_bvh != 0, shadow_masks != 0}, img)) return st;
    const rm_dev_header &H = img.H;
    const uint32_t fields[19] = {H.n_spheres, H.n_polygons, H.n_triangles, H.n_lights, H.off_spheres, H.off_polygons, H.off_pverts,
                                 H.off_triangles, H.off_materials, H.off_lights, H.off_keys, H.total_words, H.list_ordered,
                                 H.off_bvh_spheres, H.off_bvh_triangles, H.off_bounds, H.off_planar, H.off_groups, H.off_occ};
    std::memcpy(header, fields, sizeof fields);
    reals[0] = H.shadow_rho; reals[1] = img.occ_camera_limit; reals[2] = img.dead_camera_limit;
    verdicts[0] = img.exact_only ? 1u : 0u; verdicts[1] = img.integer_exponents ? 1u : 0u;
    sizes[0] = img.blob.size(); sizes[1] = img.pid_map.size();
    if (blob && pid_map && img.blob.size() <= blob_cap && img.pid_map.size() <= map_cap) {
        std::memcpy(blob, img.blob.data(), img.blob.size() * sizeof(double));
        if (!img.pid_map.empty()) std::memcpy(pid_map, img.pid_map.data(), img.pid_map.size() * sizeof(uint32_t));
    }
    return RM_OK;
}
