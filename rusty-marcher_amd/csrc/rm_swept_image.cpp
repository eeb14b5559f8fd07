// rm_swept_image.cpp -- the swept hierarchy of a scene image: see rm_swept_image.hpp.  Host arithmetic only; links without HIP.
//
// The refit keeps the image's topology -- child refs, leaf order, pid map, list-order keys -- and rewrites the twelve box words
// of every node.  A leaf child's box is the union, over the leaf's primitives, of the primitive's box with its shape at
// record + lo and at record + hi; an inner child's box is the union of the uninflated boxes below it; either is inflated once
// (rm_bvh_detail::inflate).  That is the builder's procedure (rm_bvh.hpp: a subtree's box is the union of its primitives'
// boxes, inflated where it is written), so with extents of zero the nodes come out as the image holds them, bit for bit: a
// zero's sign does not survive the inflation, whose margin is at least 1e-9.
//
// Why the two corners suffice: the kernels move a primitive by one addition a component, rounded once (OffsetShapes,
// rm_radiance_step.inc), and fl(c + off) is monotone in off.  A sphere's box is fl(c + off) -+ r, a triangle's the minimum and
// maximum of fl(v + off) over its vertices: each bound is monotone in off.c for its own component c and independent of the other
// two, so for lo <= off <= hi it lies between its values at the two corners.
//
// The primitive boxes are build_hierarchies' (rm_image.cpp) at the moved position.  A triangle's takes the z of its vertices,
// which the triangle record does not hold (the inside test reads x and y alone): the refit reads the description the image
// was built from, which the context keeps for its upload's comparison anyway.
#include "rm_swept_image.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>

#include "rm_bvh.hpp"

namespace {

struct refit {
    const rm_scene_desc *d;
    const rm_image &img;
    const double *lo, *hi;
    double *blob;

    // build_hierarchies' sphere box with the centre moved by `off`
    static void sphere_box(const rm_sphere &sp, const double *off, rm_aabb &box) {
        const double r = std::sqrt(sp.radius_square) * (1. + 1e-12);
        const double c[3] = {sp.center.x + off[0], sp.center.y + off[1], sp.center.z + off[2]};
        for (int a = 0; a < 3; a++) { box.lo[a] = c[a] - r; box.hi[a] = c[a] + r; }
    }
    // ... and its triangle box with every vertex moved by `off`
    static void triangle_box(const rm_triangle &t, const double *off, rm_aabb &box) {
        box.reset();
        for (const rm_vec3 &v : t.vertices) {
            const double c[3] = {v.x + off[0], v.y + off[1], v.z + off[2]};
            for (int a = 0; a < 3; a++) { box.lo[a] = std::min(box.lo[a], c[a]); box.hi[a] = std::max(box.hi[a], c[a]); }
        }
    }

    // The uninflated box of primitives [first, first + count) of a kind (device order) over their shapes' extents
    void leaf_box(bool spheres, uint32_t first, uint32_t count, rm_aabb &box) const {
        const rm_dev_header &H = img.H;
        box.reset();
        for (uint32_t j = first; j < first + count; j++) {
            const uint32_t pid = spheres ? j : H.n_spheres + H.n_polygons + j;
            const uint32_t shape = img.pid_map[2u * pid], element = img.pid_map[2u * pid + 1u];
            const rm_shape_ref &ref = d->shapes[shape];
            for (const double *off : {lo + 3u * shape, hi + 3u * shape}) {
                rm_aabb b;
                if (spheres) sphere_box(d->spheres[ref.first], off, b);
                else triangle_box(d->triangles[ref.first + element], off, b);
                box.grow(b);
            }
        }
    }

    // Rewrites the boxes of node `node` of the hierarchy at blob offset `off` and of every node below it; `box`: the union of
    // the uninflated boxes below the node
    void node_box(bool spheres, uint32_t off, uint32_t node, rm_aabb &box) const {
        double *n = blob + off + (size_t)RM_BVH_NODE_WORDS * node;
        rm_aabb child[2];
        for (int side = 0; side < 2; side++) {
            uint64_t ref;
            std::memcpy(&ref, &n[12 + side], 8);
            const uint32_t idx = (uint32_t)ref, cnt = (uint32_t)(ref >> 32);
            if (cnt) leaf_box(spheres, idx, cnt, child[side]);
            else node_box(spheres, off, idx, child[side]);
        }
        box = child[0];
        box.grow(child[1]);
        for (int side = 0; side < 2; side++) {
            rm_bvh_detail::inflate(child[side]);
            for (int a = 0; a < 3; a++) { n[6 * side + a] = child[side].lo[a]; n[6 * side + 3 + a] = child[side].hi[a]; }
        }
    }
};

rm_status refuse(std::string &error, const std::string &msg) {
    error = msg;
    return RM_ERR_INVALID_ARG;
}

}  // namespace

rm_status rm_swept_refit(const char *who, const rm_scene_desc *d, const rm_image &img, const double *lo, const double *hi, uint32_t n_shapes,
                         std::vector<double> &blob, std::string &error) {
    if (n_shapes != d->n_shapes) {
        char buf[192];
        std::snprintf(buf, sizeof buf, "%s: n_shapes %u, the resident scene has %u", who, n_shapes, d->n_shapes);
        return refuse(error, buf);
    }
    if (n_shapes > 0u && (!lo || !hi)) return refuse(error, std::string(who) + ": NULL extents");
    for (uint32_t k = 0; k < n_shapes; k++)
        for (uint32_t c = 0; c < 3u; c++) {
            const double l = lo[3u * k + c], h = hi[3u * k + c];
            if (!std::isfinite(l) || !std::isfinite(h) || !(l <= h)) {
                char buf[224];
                std::snprintf(buf, sizeof buf, "%s: the extents of shape %u are not finite with lo <= hi (component %u: lo = %g, hi = %g)", who, k, c, l, h);
                return refuse(error, buf);
            }
        }
    // (the map's shape words index lo and hi: an image of another description is the caller's bug, not a reason to read beyond them)
    for (size_t q = 0; q < img.pid_map.size(); q += 2u)
        if (img.pid_map[q] >= n_shapes) return refuse(error, std::string(who) + ": the image is not the description's");
    std::vector<double> out = img.blob;
    const refit r{d, img, lo, hi, out.data()};
    rm_aabb root;
    if (img.H.off_bvh_spheres) r.node_box(true, img.H.off_bvh_spheres, 0u, root);
    if (img.H.off_bvh_triangles) r.node_box(false, img.H.off_bvh_triangles, 0u, root);
    blob.swap(out);
    return RM_OK;
}

extern "C" {

rm_status rm_swept_extents(const double *table, uint32_t rows, uint32_t n_shapes, double *lo, double *hi) {
    const char *who = "rm_swept_extents";
    if (rows == 0u) { rm_set_host_error(std::string(who) + ": a table of no rows has no extents"); return RM_ERR_INVALID_ARG; }
    if (n_shapes == 0u) return RM_OK;
    if (!table || !lo || !hi) { rm_set_host_error(std::string(who) + ": NULL argument"); return RM_ERR_INVALID_ARG; }
    const size_t words = 3u * (size_t)n_shapes;
    for (size_t w = 0; w < words; w++) lo[w] = hi[w] = table[w];
    for (uint32_t r = 1; r < rows; r++)
        for (size_t w = 0; w < words; w++) {
            const double v = table[(size_t)r * words + w];
            lo[w] = std::min(lo[w], v);
            hi[w] = std::max(hi[w], v);
        }
    return RM_OK;
}

// The extents of rm_motion_sequence's rows, whatever rows: row s holds fl(v.c * t) with 0 <= t = fl(shutter * phi_17(s)) <= shutter,
// and rounding is monotone, so every entry lies between 0 and fl(v.c * shutter)
rm_status rm_swept_motion_extents(const rm_vec3 *velocities, uint32_t n_shapes, double shutter, double *lo, double *hi) {
    const char *who = "rm_swept_motion_extents";
    if (n_shapes == 0u) return RM_OK;
    if (!velocities || !lo || !hi) { rm_set_host_error(std::string(who) + ": NULL argument"); return RM_ERR_INVALID_ARG; }
    for (uint32_t k = 0; k < n_shapes; k++) {
        const double e[3] = {velocities[k].x * shutter, velocities[k].y * shutter, velocities[k].z * shutter};
        for (int c = 0; c < 3; c++) { lo[3u * k + c] = std::min(0., e[c]); hi[3u * k + c] = std::max(0., e[c]); }
    }
    return RM_OK;
}

// Test hook, not part of the ABI (tests/test_swept_abi.py): the swept blob of `d`'s image, built as the upload builds it with
// the hierarchies on or off.  *words = the blob's words; then, when cap holds them, the blob bit for bit.  Host work only.
rm_status rmi_swept_image(const rm_scene_desc *d, uint32_t use_bvh, const double *lo, const double *hi, uint32_t n_shapes, uint64_t *words,
                          uint64_t *blob, uint64_t cap) {
    std::string error = "rmi_swept_image: NULL argument";
    rm_image img;
    std::vector<double> out;
    rm_status st = (d && words) ? rm_build_image(d, rm_image_options{use_bvh != 0, true}, img, error) : RM_ERR_INVALID_ARG;
    if (!st) st = rm_swept_refit("rmi_swept_image", d, img, lo, hi, n_shapes, out, error);
    if (st) { rm_set_host_error(error); return st; }
    *words = out.size();
    if (blob && out.size() <= cap) std::memcpy(blob, out.data(), out.size() * sizeof(double));
    return RM_OK;
}

}  // extern "C"
