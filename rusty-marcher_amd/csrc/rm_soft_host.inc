// rm_soft_host.inc -- host side of the area lights' device call (include/rusty_marcher_amd.h, "area lights"); included at the end
// of rm_device.hip, behind rm_accum_host.inc whose checks (check_accum_device, check_offset_tables) and argument block
// (accum_call, accum_args) it shares.  The kernel is rm_soft.hip's.
//
// rm_accumulate_soft_device touches no render state and keeps none of its own: one launch on the caller's stream, nothing
// waited for.  The tick, rm_render_progressive_soft, stands with the other two in rm_motion_host.inc; rm_light_sequence is
// rm_sampling.cpp's.

// The launch; offsets: NULL where the scene has no lights.
static rm_status launch_soft(rm_ctx *ctx, const accum_call &c, const void *offsets) {
    SoftArgs a{};
    a.A = accum_args(ctx, c);
    a.offsets = static_cast<const double *>(offsets);
    return launch_shading(ctx, shade_family{"area lights", rm_soft_kernel}, a.A.L.max_depth, lens_extent(ctx, a.A.L), a, c.stream);
}

extern "C" rm_status rm_accumulate_soft_device(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *device_table,
                                               const void *device_offsets, uint32_t n_lights, uint32_t n_before, void *device_sum,
                                               void *device_mean, void *device_rgb8, void *hip_stream) {
    const char *who = "rm_accumulate_soft_device";
    return guarded(ctx, who, [&]() -> rm_status {
        if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
        if (rm_status cst = check_accum_device(ctx, who, p, lens, device_table, n_before, device_sum, device_mean)) return cst;
        if (rm_status ost = check_offset_tables(ctx, who, "offsets", device_offsets, n_lights)) return ost;
        if (refine_rows(p) == 0u) return RM_OK;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        return launch_soft(ctx, accum_call{p, lens, device_table, n_before, device_sum, device_mean, device_rgb8, (hipStream_t)hip_stream},
                           n_lights > 0u ? device_offsets : nullptr);
    });
}
