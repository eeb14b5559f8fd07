// AddressSanitizer / UBSan exercise of what the diffuse bounce added to the sampled frames' host arithmetic (csrc/rm_sampling.cpp):
// rm_bounce_sequence and its refusals, the check of the strength, the strength in a frame's identity and the bounce column of the
// staging rule.  Links rm_sampling.cpp alone; the host error text it reports through lives here.  CPU only.
#include <cassert>
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "rusty_marcher_amd.h"
#include "rm_internal.h"
#include "rm_sampling.hpp"

// (rm_scene.cpp's in the library: the one thing rm_sampling.cpp needs of it)
static std::string g_error;
void rm_set_host_error(const std::string &msg) { g_error = msg; }
const char *rm_get_host_error() { return g_error.c_str(); }

// phi_b(s) by the header's words: the digits of s in base b mirrored at the point, one division
static double phi(uint32_t s, uint32_t b) {
    uint64_t r = 0, q = 1;
    for (; s > 0u; s /= b) {
        r = r * b + s % b;
        q *= b;
    }
    return (double)r / (double)q;
}

int main() {
    // the sequence: exactly the rows asked for, not a double more, wherever the slice begins
    for (const auto &slice : {std::pair<uint32_t, uint32_t>{0u, 200u}, {1000u, 7u}, {65535u, 1u}, {65472u, 64u}}) {
        std::vector<double> rows(2u * slice.second + 1u, -7.);
        assert(rm_bounce_sequence(slice.first, slice.second, rows.data()) == RM_OK);
        assert(rows.back() == -7.);
        for (uint32_t k = 0; k < slice.second; k++) {
            assert(rows[2u * k] == phi(slice.first + k, 19u) && rows[2u * k + 1u] == phi(slice.first + k, 23u));
            assert(rows[2u * k] >= 0. && rows[2u * k] < 1. && rows[2u * k + 1u] >= 0. && rows[2u * k + 1u] < 1.);
        }
    }
    double one[2] = {-7., -7.};
    assert(rm_bounce_sequence(0u, 1u, one) == RM_OK && one[0] == 0. && one[1] == 0.);
    // refusals write nothing
    one[0] = one[1] = -7.;
    assert(rm_bounce_sequence(65536u, 1u, one) == RM_ERR_INVALID_ARG && g_error.find("first + count") != std::string::npos);
    assert(rm_bounce_sequence(0u, 65537u, one) == RM_ERR_INVALID_ARG);
    assert(rm_bounce_sequence(0xffffffffu, 2u, one) == RM_ERR_INVALID_ARG);
    assert(rm_bounce_sequence(0u, 1u, nullptr) == RM_ERR_INVALID_ARG && g_error.find("NULL table") != std::string::npos);
    assert(rm_bounce_sequence(12u, 0u, nullptr) == RM_OK && rm_bounce_sequence(65536u, 0u, one) == RM_OK);
    assert(one[0] == -7. && one[1] == -7.);

    // the strength
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (double ok : {0., -0., 1e-300, 0.5, 1., 1e300}) assert(rm_check_strength("t", ok) == RM_OK);
    for (double bad : {-1e-300, -1., inf, -inf, nan}) {
        assert(rm_check_strength("t", bad) == RM_ERR_INVALID_ARG);
        assert(g_error.find("strength") != std::string::npos);
    }

    // the identity: a bounce frame is its own, and the strength is part of it -- a strength of 0 is not "no bounce"
    rm_params p{};
    p.fov = 1.5; p.half_fov = .93; p.height = 32.; p.width = 32.; p.ratio = 1.; p.frame_width = 32u; p.frame_height = 32u; p.max_depth = 3u;
    const rm_lens lens{0., 1., 8u, 0u};
    const rm_vec3 camera{0., 0., 0.};
    const rm_camera_basis basis{{1., 0., 0.}, {0., 1., 0.}, {0., 0., -1.}};
    auto with = [&](const rm_sampling_rules &r) { return rm_frame_identity_of(p, lens, camera, basis, false, 7u, r); };
    rm_sampling_rules none, zero, one_, half;
    zero.bounce = true; zero.strength = 0.;
    one_.bounce = true; one_.strength = 1.;
    half.bounce = true; half.strength = .5;
    assert(rm_same_frame(with(none), with(none)) && rm_same_frame(with(one_), with(one_)));
    assert(!rm_same_frame(with(none), with(zero)) && !rm_same_frame(with(zero), with(one_)) && !rm_same_frame(with(one_), with(half)));
    const double radii[2] = {1., 2.};
    rm_sampling_rules soft_bounce = one_, soft;
    soft.soft = soft_bounce.soft = true; soft.radii = soft_bounce.radii = radii; soft.n_lights = soft_bounce.n_lights = 2u;
    assert(!rm_same_frame(with(soft), with(soft_bounce)) && !rm_same_frame(with(one_), with(soft_bounce)));

    // the staging rule: two bounce columns for a bounce tick and none otherwise; the progressive bounce kernel reads a light row
    // for every light of the scene (zeros without radii), the converging one only with radii
    for (uint32_t lights : {0u, 2u})
        for (bool with_radii : {false, true}) {
            rm_sampling_rules r = with_radii ? soft_bounce : one_;
            if (with_radii) r.n_lights = lights;
            const rm_staging a = rm_staging_of(RM_TICK_PROGRESSIVE, r, lights, 3u, 4u);
            const rm_staging c = rm_staging_of(RM_TICK_CONVERGING, r, lights, 3u, 4u);
            assert(a.bounce_columns == 2u && c.bounce_columns == 2u && a.shape_columns == 0u && c.shape_columns == 0u);
            assert(a.light_columns == lights && a.light_zeros == !with_radii);
            assert(c.light_columns == (with_radii ? lights : 0u) && !c.light_zeros);
            std::vector<double> rows(3u * 2u + 1u, -7.);
            assert(rm_fill_bounce_rows(4u, 3u, rows.data()) == RM_OK && rows.back() == -7.);
            for (uint32_t k = 0; k < 3u; k++) assert(rows[2u * k] == phi(4u + k, 19u) && rows[2u * k + 1u] == phi(4u + k, 23u));
        }
    for (rm_tick_kind kind : {RM_TICK_PROGRESSIVE, RM_TICK_CONVERGING, RM_TICK_CONVERGING_MOVING})
        assert(rm_staging_of(kind, none, 2u, 3u, 4u).bounce_columns == 0u && rm_staging_of(kind, soft, 2u, 3u, 4u).bounce_columns == 0u);
    std::printf("bounce sampling ok\n");
    return 0;
}
