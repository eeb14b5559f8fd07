// rm_bounce_host.inc -- host side of the diffuse bounce (include/rusty_marcher_amd.h, "diffuse bounce"); included at the end of
// rm_device.hip, behind rm_soft_host.inc and rm_converge_host.inc whose checks and argument blocks it shares, and behind the two
// ticks (rm_motion_host.inc, rm_converge_motion_host.inc), which declare the two launches here and end in them where their
// rules say `bounce`.  The kernels are rm_bounce.hip's and rm_converge_bounce.hip's; rm_bounce_sequence, the check of the
// strength, the frames' identity and the staging rule are rm_sampling.cpp's.
//
// The device calls touch no render state and keep none of their own: launches on the caller's stream, nothing waited for.  The
// ticks are the progressive and the converging tick with frames of their own (the strength joins the key) and one table more: a
// slice, or a resident prefix, of rm_bounce_sequence.

// What a bounce call checks beside the call it is built over: the table and the strength
static rm_status check_bounce(rm_ctx *ctx, const char *who, const void *device_bounce, double strength) {
    if (!device_bounce) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL bounce table");
    return host_refusal(ctx, rm_check_strength(who, strength));
}

// The launch; offsets: NULL where the scene has no lights.
static rm_status launch_bounce(rm_ctx *ctx, const accum_call &c, const void *offsets, const void *bounce, double strength) {
    BounceArgs a{};
    a.S.A = accum_args(ctx, c);
    a.S.offsets = static_cast<const double *>(offsets);
    a.bounce = static_cast<const double *>(bounce);
    a.strength = strength;
    return launch_shading(ctx, shade_family{"diffuse bounce", rm_bounce_kernel}, a.S.A.L.max_depth, lens_extent(ctx, a.S.A.L), a, c.stream);
}

// The converging frames' three steps with the bounce kernel in the third; offsets: NULL for the lights where the scene image says
static rm_status launch_converge_bounce(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c, const void *table,
                                        uint32_t table_rows, const void *offsets, const void *bounce, double strength, int fresh,
                                        const rm_converge_frame *b, hipStream_t stream) {
    ConvergeBounceArgs m{};
    m.C = converge_args(ctx, p, lens, c, table, table_rows, offsets, fresh, b);
    m.bounce = static_cast<const double *>(bounce);
    m.strength = strength;
    const shade_family stored{"converging with a diffuse bounce", [](bool bvh, int pow_mode, int stack) { return rm_converge_bounce_kernel(bvh, pow_mode, stack, false); }};
    const shade_family moved{"converging with a diffuse bounce", [](bool bvh, int pow_mode, int stack) { return rm_converge_bounce_kernel(bvh, pow_mode, stack, true); }};
    return launch_converge_with(ctx, offsets ? moved : stored, m, m.C, stream);
}

static rm_sampling_rules rules_with_bounce(const double *radii, uint32_t n_lights, double strength) {
    rm_sampling_rules r = rules_with_radii(radii, n_lights);
    r.bounce = true;
    r.strength = strength;
    return r;
}

extern "C" {

rm_status rm_accumulate_bounce_device(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *device_table,
                                      const void *device_offsets, uint32_t n_lights, const void *device_bounce, double strength,
                                      uint32_t n_before, void *device_sum, void *device_mean, void *device_rgb8, void *hip_stream) {
    const char *who = "rm_accumulate_bounce_device";
    return guarded(ctx, who, [&]() -> rm_status {
        if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
        if (rm_status cst = check_accum_device(ctx, who, p, lens, device_table, n_before, device_sum, device_mean)) return cst;
        if (rm_status ost = check_offset_tables(ctx, who, "offsets", device_offsets, n_lights)) return ost;
        if (rm_status bst = check_bounce(ctx, who, device_bounce, strength)) return bst;
        if (refine_rows(p) == 0u) return RM_OK;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        return launch_bounce(ctx, accum_call{p, lens, device_table, n_before, device_sum, device_mean, device_rgb8, (hipStream_t)hip_stream},
                             n_lights > 0u ? device_offsets : nullptr, device_bounce, strength);
    });
}

rm_status rm_accumulate_converging_bounce_device(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c,
                                                 const void *device_table, uint32_t table_rows, const void *device_offsets,
                                                 uint32_t n_lights, const void *device_bounce, double strength, int fresh,
                                                 const rm_converge_frame *b, void *hip_stream) {
    const char *who = "rm_accumulate_converging_bounce_device";
    return guarded(ctx, who, [&]() -> rm_status {
        if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
        // (without a table n_lights is not looked at)
        auto tables = [&]() { return device_offsets ? check_offset_tables(ctx, who, "offsets", device_offsets, n_lights) : RM_OK; };
        if (rm_status cst = check_converge_call(ctx, who, p, lens, c, device_table, table_rows, b, tables)) return cst;
        if (rm_status bst = check_bounce(ctx, who, device_bounce, strength)) return bst;
        if (refine_rows(p) == 0u) return RM_OK;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        return launch_converge_bounce(ctx, p, lens, c, device_table, table_rows, ctx->image.H.n_lights > 0u ? device_offsets : nullptr,
                                      device_bounce, strength, fresh, b, (hipStream_t)hip_stream);
    });
}

rm_status rm_render_progressive_bounce(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const double *radii, uint32_t n_lights,
                                       double strength, int restart, double *host_rgb, uint8_t *host_rgb8, uint32_t *n_total,
                                       rm_timing *timing) {
    return guarded(ctx, "rm_render_progressive_bounce", [&]() {
        return rm_render_progressive_impl(ctx, "rm_render_progressive_bounce", params, lens, rules_with_bounce(radii, n_lights, strength), restart,
                                          host_rgb, host_rgb8, n_total, timing);
    });
}

rm_status rm_render_converging_bounce(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const rm_converge *converge,
                                      const double *radii, uint32_t n_lights, double strength, int restart, double *host_rgb,
                                      uint8_t *host_rgb8, rm_converge_report *report, rm_timing *timing) {
    return guarded(ctx, "rm_render_converging_bounce", [&]() {
        return rm_render_converging_impl(ctx, "rm_render_converging_bounce", params, lens, converge, rules_with_bounce(radii, n_lights, strength),
                                         restart, host_rgb, host_rgb8, report, timing);
    });
}

}  // extern "C"
