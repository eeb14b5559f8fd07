// rm_sampling.cpp -- the host arithmetic of the sampled frames (rm_sampling.hpp): sequences, number checks, frame identity,
// staging rule.  No device, no context, no HIP header.
#include "rm_sampling.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

static rm_status refuse(const std::string &msg) {
    rm_set_host_error(msg);
    return RM_ERR_INVALID_ARG;
}

// phi_b(s): the digits of s in base b mirrored at the point, as the integer pair (r, q) -- r / q is the value
static void digit_reversed(uint32_t s, uint32_t b, uint64_t *r, uint64_t *q) {
    uint64_t rr = 0, qq = 1;
    while (s > 0u) {
        rr = rr * b + s % b;
        qq *= b;
        s /= b;
    }
    *r = rr;
    *q = qq;
}

static double radical_inverse(uint32_t s, uint32_t b) {
    uint64_t r, q;
    digit_reversed(s, b, &r, &q);
    return (double)r / (double)q;
}

// The rows a sequence has: [0, RM_PROGRESSIVE_MAX_SAMPLES)
static rm_status check_rows(const char *who, uint32_t first, uint32_t count) {
    if ((uint64_t)first + count <= RM_PROGRESSIVE_MAX_SAMPLES) return RM_OK;
    char buf[128];
    std::snprintf(buf, sizeof buf, "%s: first + count = %u + %u is more than %u", who, first, count, RM_PROGRESSIVE_MAX_SAMPLES);
    return refuse(buf);
}

rm_status rm_check_radii(const char *who, const double *radii, uint32_t n_lights) {
    if (n_lights > 0u && !radii) return refuse(std::string(who) + ": NULL radii");
    for (uint32_t l = 0; l < n_lights; l++)
        if (!std::isfinite(radii[l]) || !(radii[l] >= 0.)) {
            char buf[160];
            std::snprintf(buf, sizeof buf, "%s: radii[%u] = %g is not a finite number >= 0", who, l, radii[l]);
            return refuse(buf);
        }
    return RM_OK;
}

rm_status rm_check_velocities(const char *who, const rm_vec3 *velocities, uint32_t n_shapes, double shutter) {
    if (n_shapes > 0u && !velocities) return refuse(std::string(who) + ": NULL velocities");
    for (uint32_t k = 0; k < n_shapes; k++) {
        const rm_vec3 &v = velocities[k];
        if (!std::isfinite(v.x) || !std::isfinite(v.y) || !std::isfinite(v.z)) {
            char buf[192];
            std::snprintf(buf, sizeof buf, "%s: velocities[%u] = (%g, %g, %g) is not finite", who, k, v.x, v.y, v.z);
            return refuse(buf);
        }
    }
    if (!std::isfinite(shutter) || !(shutter >= 0.)) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "%s: shutter = %g is not a finite number >= 0", who, shutter);
        return refuse(buf);
    }
    return RM_OK;
}

rm_status rm_check_strength(const char *who, double strength) {
    if (std::isfinite(strength) && strength >= 0.) return RM_OK;
    char buf[160];
    std::snprintf(buf, sizeof buf, "%s: strength = %g is not a finite number >= 0", who, strength);
    return refuse(buf);
}

rm_frame_identity rm_frame_identity_of(const rm_params &p, const rm_lens &lens, const rm_vec3 &camera, const rm_camera_basis &basis, bool oriented,
                                       uint64_t upload_copies, const rm_sampling_rules &rules) {
    rm_frame_identity id;
    rm_progressive_key &key = id.key;
    std::memset(&key, 0, sizeof key);
    key.fov = p.fov; key.half_fov = p.half_fov; key.height = p.height; key.width = p.width; key.ratio = p.ratio;
    key.frame_width = p.frame_width; key.frame_height = p.frame_height; key.max_depth = p.max_depth;
    key.oriented = oriented ? 1u : 0u;
    key.background = p.background;
    key.aperture = lens.aperture; key.focus = lens.focus;
    key.camera = camera;
    key.basis = basis;
    key.copies = upload_copies;
    if (rules.soft) {
        key.soft = 1u; key.n_lights = rules.n_lights;
        id.radii.assign(rules.radii, rules.radii + rules.n_lights);             // (n_lights == 0: empty, radii may be NULL)
    }
    if (rules.motion) {
        key.motion = 1u; key.n_shapes = rules.n_shapes; key.shutter = rules.shutter;
        id.velocities.assign(rules.velocities, rules.velocities + rules.n_shapes);
    }
    if (rules.camera) {
        key.camera_moves = 1u;
        key.camera_motion = *rules.camera;
        key.shutter = rules.shutter;                                           // (with or without velocities)
    }
    if (rules.bounce) {
        key.bounce = 1u;
        key.strength = rules.strength;
    }
    return id;
}

template <class T>
static bool same_bytes(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

bool rm_same_radii(const rm_frame_identity &a, const rm_frame_identity &b) { return same_bytes(a.radii, b.radii); }

bool rm_same_frame(const rm_frame_identity &a, const rm_frame_identity &b) {
    return std::memcmp(&a.key, &b.key, sizeof a.key) == 0 && rm_same_radii(a, b) && same_bytes(a.velocities, b.velocities);
}

rm_staging rm_staging_of(rm_tick_kind kind, const rm_sampling_rules &rules, uint32_t scene_lights, uint32_t scene_spheres, uint32_t scene_shapes) {
    rm_staging s;
    // kernels that read a row for every light of the scene (the progressive bounce kernel is the area lights'; the converging
    // one has a form with stored lights, as the converging kernel has)
    const bool every_light = rules.motion || rules.camera != nullptr || (rules.bounce && kind == RM_TICK_PROGRESSIVE);
    s.light_columns = every_light ? scene_lights : rules.soft ? rules.n_lights : 0u;
    s.light_zeros = every_light && !rules.soft;
    s.shape_columns = rules.motion && (kind != RM_TICK_CONVERGING || scene_spheres > 0u) ? scene_shapes : 0u;
    s.bounce_columns = rules.bounce ? 2u : 0u;
    return s;
}

rm_status rm_fill_light_rows(const rm_sampling_rules &rules, const rm_staging &staged, uint32_t first, uint32_t count, double *out) {
    if (!staged.light_zeros) return rm_light_sequence(first, count, rules.radii, rules.n_lights, out);
    std::fill(out, out + (size_t)count * staged.light_columns * 3u, 0.);
    return RM_OK;
}

rm_status rm_fill_shape_rows(const rm_sampling_rules &rules, uint32_t first, uint32_t count, double *out) {
    return rm_motion_sequence(first, count, rules.velocities, rules.n_shapes, rules.shutter, out);
}

double rm_shutter_time(uint32_t s, double shutter) { return shutter * radical_inverse(s, 17u); }   // (row 0: 0, the scene as uploaded)

extern "C" {

rm_status rm_lens_sequence(uint32_t first, uint32_t count, double *table) {
    if (rm_status rst = check_rows("rm_lens_sequence", first, count)) return rst;
    if (count == 0u) return RM_OK;
    if (!table) return refuse("rm_lens_sequence: NULL table");
    for (uint32_t k = 0; k < count; k++) {
        const uint32_t s = first + k;
        const double a = 2. * radical_inverse(s, 5u) - 1.;
        const double b = 2. * radical_inverse(s, 7u) - 1.;
        double *r = table + 4u * (size_t)k;
        r[0] = radical_inverse(s, 2u);
        r[1] = radical_inverse(s, 3u);
        r[2] = a * std::sqrt(1. - b * b / 2.);
        r[3] = b * std::sqrt(1. - a * a / 2.);
    }
    return RM_OK;
}

rm_status rm_light_sequence(uint32_t first, uint32_t count, const double *radii, uint32_t n_lights, double *offsets) {
    const char *who = "rm_light_sequence";
    if (rm_status rst = check_rows(who, first, count)) return rst;
    if (count == 0u || n_lights == 0u) return RM_OK;
    if (rm_status rst = rm_check_radii(who, radii, n_lights)) return rst;
    if (!offsets) return refuse(std::string(who) + ": NULL offsets");
    for (uint32_t k = 0; k < count; k++) {
        const uint32_t s = first + k;
        const double p11 = radical_inverse(s, 11u), p13 = radical_inverse(s, 13u);
        for (uint32_t l = 0; l < n_lights; l++) {
            double x = p11 + (double)l * 0.6180339887498949;
            x = x - std::floor(x);
            double y = p13 + (double)l * 0.6180339887498949;
            y = y - std::floor(y);
            const double a = 2. * x - 1., b = 2. * y - 1.;
            const double u = a * std::sqrt(1. - b * b / 2.), v = b * std::sqrt(1. - a * a / 2.);   // the disc of rm_lens_table
            const double r2 = u * u + v * v;
            const double h = 2. * std::sqrt(std::fmax(1. - r2, 0.));                                 // ... lifted to the sphere
            double *o = offsets + ((size_t)k * n_lights + l) * 3u;
            o[0] = radii[l] * (u * h);
            o[1] = radii[l] * (v * h);
            o[2] = radii[l] * (1. - 2. * r2);
        }
    }
    return RM_OK;
}

rm_status rm_bounce_sequence(uint32_t first, uint32_t count, double *table) {
    if (rm_status rst = check_rows("rm_bounce_sequence", first, count)) return rst;
    if (count == 0u) return RM_OK;
    if (!table) return refuse("rm_bounce_sequence: NULL table");
    for (uint32_t k = 0; k < count; k++) {
        table[2u * (size_t)k] = radical_inverse(first + k, 19u);
        table[2u * (size_t)k + 1u] = radical_inverse(first + k, 23u);
    }
    return RM_OK;
}

rm_status rm_motion_sequence(uint32_t first, uint32_t count, const rm_vec3 *velocities, uint32_t n_shapes, double shutter, double *offsets) {
    const char *who = "rm_motion_sequence";
    if (rm_status rst = check_rows(who, first, count)) return rst;
    if (count == 0u || n_shapes == 0u) return RM_OK;
    if (rm_status vst = rm_check_velocities(who, velocities, n_shapes, shutter)) return vst;
    if (!offsets) return refuse(std::string(who) + ": NULL offsets");
    for (uint32_t k = 0; k < count; k++) {
        const double t = rm_shutter_time(first + k, shutter);
        for (uint32_t j = 0; j < n_shapes; j++) {
            double *o = offsets + ((size_t)k * n_shapes + j) * 3u;
            o[0] = velocities[j].x * t;
            o[1] = velocities[j].y * t;
            o[2] = velocities[j].z * t;
        }
    }
    return RM_OK;
}

}  // extern "C"
