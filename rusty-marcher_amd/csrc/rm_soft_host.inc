// rm_soft_host.inc -- host side of the area lights (include/rusty_marcher_amd.h, "area lights"); included at the end of
// rm_device.hip, behind rm_accum_host.inc whose checks (check_accum_device), sequence arithmetic (radical_inverse) and tick
// (rm_render_progressive_impl, which stages the offsets and calls launch_soft below) it shares.  The kernel is rm_soft.hip's.
//
// rm_accumulate_soft_device touches no render state and keeps none of its own: one launch on the caller's stream, nothing
// waited for.  rm_render_progressive_soft is rm_render_progressive with the radii in the frame's key.

// n_lights of a soft call: the resident scene's, as rm_lights_visible requires
static rm_status check_soft_lights(rm_ctx *ctx, const char *who, uint32_t n_lights) {
    if (n_lights != ctx->image.H.n_lights) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "%s: n_lights %u, the resident scene has %u", who, n_lights, ctx->image.H.n_lights);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    return RM_OK;
}

// A radius is a finite number >= 0 (a NaN fails the comparison); ctx may be NULL (rm_light_sequence has none)
static rm_status check_radii(rm_ctx *ctx, const char *who, const double *radii, uint32_t n_lights) {
    if (n_lights > 0u && !radii) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL radii");
    for (uint32_t l = 0; l < n_lights; l++)
        if (!std::isfinite(radii[l]) || !(radii[l] >= 0.)) {
            char buf[160];
            std::snprintf(buf, sizeof buf, "%s: radii[%u] = %g is not a finite number >= 0", who, l, radii[l]);
            return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
        }
    return RM_OK;
}

static rm_status check_soft_radii(rm_ctx *ctx, const char *who, const double *radii, uint32_t n_lights) {
    if (rm_status lst = check_soft_lights(ctx, who, n_lights)) return lst;
    return check_radii(ctx, who, radii, n_lights);
}

// The launch on `stream`; everything was checked, rows > 0.  offsets: NULL where the scene has no lights.
static rm_status launch_soft(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *table, const void *offsets, uint32_t n_before,
                             void *sum, void *mean, void *rgb8, hipStream_t stream) {
    SoftArgs a{};
    a.A.L = lens_args(ctx, p, lens, table, nullptr);
    a.A.n_before = n_before;
    a.A.sum = static_cast<double *>(sum);
    a.A.mean = static_cast<double *>(mean);
    a.A.rgb8 = static_cast<uint8_t *>(rgb8);
    a.offsets = static_cast<const double *>(offsets);
    return launch_shading(ctx, shade_family{"area lights", rm_soft_kernel}, a.A.L.max_depth, lens_extent(ctx, a.A.L), a, stream);
}

static rm_status rm_accumulate_soft_device_impl(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *device_table,
                                                const void *device_offsets, uint32_t n_lights, uint32_t n_before, void *device_sum,
                                                void *device_mean, void *device_rgb8, void *hip_stream) {
    const char *who = "rm_accumulate_soft_device";
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
    if (rm_status cst = check_accum_device(ctx, who, p, lens, device_table, n_before, device_sum, device_mean)) return cst;
    if (rm_status lst = check_soft_lights(ctx, who, n_lights)) return lst;
    if (n_lights > 0u && !device_offsets) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL offsets");
    if (refine_rows(p) == 0u) return RM_OK;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    return launch_soft(ctx, p, lens, device_table, n_lights > 0u ? device_offsets : nullptr, n_before, device_sum, device_mean, device_rgb8,
                       (hipStream_t)hip_stream);
}

extern "C" {

rm_status rm_light_sequence(uint32_t first, uint32_t count, const double *radii, uint32_t n_lights, double *offsets) {
    const char *who = "rm_light_sequence";
    if ((uint64_t)first + count > RM_PROGRESSIVE_MAX_SAMPLES) {
        char buf[128];
        std::snprintf(buf, sizeof buf, "%s: first + count = %u + %u is more than %u", who, first, count, RM_PROGRESSIVE_MAX_SAMPLES);
        return ctx_fail(nullptr, RM_ERR_INVALID_ARG, buf);
    }
    if (count == 0u || n_lights == 0u) return RM_OK;
    if (rm_status rst = check_radii(nullptr, who, radii, n_lights)) return rst;
    if (!offsets) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL offsets");
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

rm_status rm_accumulate_soft_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const void *device_table,
                                    const void *device_offsets, uint32_t n_lights, uint32_t n_before, void *device_sum, void *device_mean,
                                    void *device_rgb8, void *hip_stream) {
    return guarded(ctx, "rm_accumulate_soft_device", [&]() {
        return rm_accumulate_soft_device_impl(ctx, params, lens, device_table, device_offsets, n_lights, n_before, device_sum, device_mean,
                                              device_rgb8, hip_stream);
    });
}

rm_status rm_render_progressive_soft(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const double *radii, uint32_t n_lights,
                                     int restart, double *host_rgb, uint8_t *host_rgb8, uint32_t *n_total, rm_timing *timing) {
    return guarded(ctx, "rm_render_progressive_soft", [&]() {
        return rm_render_progressive_impl(ctx, "rm_render_progressive_soft", params, lens, true, radii, n_lights, restart, host_rgb, host_rgb8,
                                          n_total, timing);
    });
}

}  // extern "C"
