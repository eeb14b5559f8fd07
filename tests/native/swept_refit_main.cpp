// AddressSanitizer / UBSan exercise of the swept hierarchies' refit (csrc/rm_swept_image.cpp: rm_swept_refit, rm_swept_extents,
// rm_swept_motion_extents and the hook rmi_swept_image) over images built by csrc/rm_image.cpp from scenes of the host builder
// (csrc/rm_scene.cpp).  Scenes whose device order ends in a partial leaf, both hierarchies at once, no hierarchy at all, and
// every refusal.  CPU only; links no HIP.
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rusty_marcher_amd.h"
#include "rm_internal.h"
#include "rm_swept_image.hpp"

// (rm_device.hip's in the library: the one thing rm_scene.cpp needs of it)
extern "C" const char *rm_last_error(const rm_ctx *) { return rm_get_host_error(); }

extern "C" rm_status rmi_swept_image(const rm_scene_desc *d, uint32_t use_bvh, const double *lo, const double *hi, uint32_t n_shapes,
                                     uint64_t *words, uint64_t *blob, uint64_t cap);

static rm_scene *scene_of(uint32_t n_spheres, uint32_t n_triangles) {
    rm_scene *s = nullptr;
    assert(rm_scene_new(&s) == RM_OK);
    rm_reflectance r;
    rm_reflectance_default(&r);
    for (uint32_t k = 0; k < n_spheres; k++)
        assert(rm_scene_add_sphere(s, rm_vec3{-6. + 3. * (k % 5), -4. + 2. * (k / 5), -12. - 0.5 * (k % 3)}, 0.75 + 0.125 * (k % 2), &r) == RM_OK);
    if (n_triangles) {
        std::vector<double> tri;
        for (uint32_t k = 0; k < n_triangles; k++) {
            const double x = -5. + 2.5 * (k % 4), y = -3.5 + 2.5 * (k / 4), z = -10. - 0.5 * (k % 3);
            const double t[9] = {x, y, z, x + 2., y + 0.25, z - 0.25, x + 0.5, y + 2., z + 0.25};
            tri.insert(tri.end(), t, t + 9);
        }
        assert(rm_scene_add_mesh(s, tri.data(), n_triangles, rm_vec3{0., 0., 0.}) == RM_OK);
    }
    assert(rm_scene_add_light(s, rm_vec3{2., 6., 2.}, rm_vec3{1., 1., 1.}, 1.) == RM_OK);
    return s;
}

// The blob of (lo, hi) by the hook; refused: empty
static std::vector<uint64_t> swept(const rm_scene_desc &d, bool bvh, const std::vector<double> &lo, const std::vector<double> &hi, rm_status want = RM_OK) {
    uint64_t words = 0;
    const uint32_t n = (uint32_t)(lo.size() / 3);
    const rm_status st = rmi_swept_image(&d, bvh ? 1u : 0u, lo.data(), hi.data(), n, &words, nullptr, 0);
    assert(st == want);
    if (st) return {};
    std::vector<uint64_t> blob(words);
    assert(rmi_swept_image(&d, bvh ? 1u : 0u, lo.data(), hi.data(), n, &words, blob.data(), blob.size()) == RM_OK && words == blob.size());
    return blob;
}

int main() {
    int cases = 0;
    const uint32_t shapes[][2] = {{17u, 0u}, {0u, 13u}, {17u, 13u}, {21u, 25u}, {3u, 2u}, {16u, 12u}, {0u, 0u}};
    for (const auto &c : shapes) {
        rm_scene *s = scene_of(c[0], c[1]);
        rm_scene_desc d;
        assert(rm_scene_get_desc(s, &d) == RM_OK);
        const uint32_t n = d.n_shapes;
        assert(n == c[0] + (c[1] ? 1u : 0u));
        rm_image img;
        std::string error;
        assert(rm_build_image(&d, rm_image_options{}, img, error) == RM_OK);
        const bool any = img.H.off_bvh_spheres || img.H.off_bvh_triangles;
        assert(any == (c[0] >= 16u || c[1] >= 12u));

        // extents of zero: the image's own words; extents that are not: the same size, other boxes where there is a hierarchy
        const std::vector<double> zero(3u * n, 0.);
        std::vector<double> lo(3u * n), hi(3u * n);
        for (uint32_t w = 0; w < 3u * n; w++) { lo[w] = w % 4u == 0u ? 0. : -0.25 * (w % 7u); hi[w] = w % 5u == 0u ? 0. : 0.5 * (w % 3u) + 100. * (w % 11u == 0u); }
        const std::vector<uint64_t> same = swept(d, true, zero, zero), moved = swept(d, true, lo, hi);
        assert(same.size() == img.blob.size() && std::memcmp(same.data(), img.blob.data(), same.size() * 8u) == 0);
        assert(moved.size() == same.size() && (std::memcmp(moved.data(), same.data(), same.size() * 8u) != 0) == (any && n > 0u));
        const std::vector<uint64_t> flat = swept(d, false, lo, hi), flat0 = swept(d, false, zero, zero);
        assert(flat == flat0);

        // the unit's own entry, into a vector that holds something: replaced on success, left alone on a refusal
        std::vector<double> out(5u, 7.);
        assert(rm_swept_refit("main", &d, img, lo.data(), hi.data(), n, out, error) == RM_OK && out.size() == img.blob.size());
        if (n > 0u) {
            std::vector<double> bad = hi;
            bad[3u * (n - 1u) + 2u] = std::nan("");
            out.assign(5u, 7.);
            assert(rm_swept_refit("main", &d, img, lo.data(), bad.data(), n, out, error) == RM_ERR_INVALID_ARG && out.size() == 5u && out[4] == 7.);
            assert(error.find("shape " + std::to_string(n - 1u)) != std::string::npos);
            bad = lo;
            bad[0] = 1.;
            (void)swept(d, true, bad, zero, RM_ERR_INVALID_ARG);
            assert(std::string(rm_get_host_error()).find("shape 0") != std::string::npos);
            assert(rm_swept_refit("main", &d, img, nullptr, nullptr, n, out, error) == RM_ERR_INVALID_ARG);
        }
        assert(rm_swept_refit("main", &d, img, lo.data(), hi.data(), n + 1u, out, error) == RM_ERR_INVALID_ARG);
        assert(error.find("n_shapes") != std::string::npos);

        // the extents helpers: a table of three rows, and the velocities' own
        std::vector<double> table(3u * 3u * n);
        for (size_t w = 0; w < table.size(); w++) table[w] = std::sin(1. + (double)w);
        std::vector<double> tlo(3u * n + 1u, 9.), thi(3u * n + 1u, 9.);
        assert(rm_swept_extents(table.data(), 3u, n, tlo.data(), thi.data()) == RM_OK && tlo.back() == 9. && thi.back() == 9.);
        for (uint32_t w = 0; w < 3u * n; w++)
            for (uint32_t r = 0; r < 3u; r++) assert(tlo[w] <= table[r * 3u * n + w] && table[r * 3u * n + w] <= thi[w]);
        assert(rm_swept_extents(table.data(), 0u, n, tlo.data(), thi.data()) == RM_ERR_INVALID_ARG);
        std::vector<rm_vec3> v(n);
        for (uint32_t k = 0; k < n; k++) v[k] = rm_vec3{1. * k, -2. * k, k % 2u ? 0.5 : 0.};
        assert(rm_swept_motion_extents(v.data(), n, 0.75, tlo.data(), thi.data()) == RM_OK && tlo.back() == 9.);
        for (uint32_t w = 0; w < 3u * n; w++) assert(tlo[w] <= 0. && 0. <= thi[w]);
        (void)swept(d, true, std::vector<double>(tlo.begin(), tlo.end() - 1), std::vector<double>(thi.begin(), thi.end() - 1));

        rm_scene_free(s);
        cases++;
    }
    assert(rmi_swept_image(nullptr, 1u, nullptr, nullptr, 0u, nullptr, nullptr, 0) == RM_ERR_INVALID_ARG);
    std::printf("swept refit ok: %d scenes\n", cases);
    return 0;
}
