// rm_camera_swept_host.inc -- host side of the swept hierarchies under a moving camera (include/rusty_marcher_amd.h, "swept
// hierarchies under a moving camera"); included at the end of rm_device.hip, behind rm_swept_host.inc (rm_swept, check_swept, the
// ticks' hierarchy) and rm_camera_host.inc (check_camera_tables, launch_camera_over, launch_converge_camera_over).  The kernels
// are rm_camera_swept.hip's and rm_converge_camera_swept.hip's, the select kernel rm_converge.hip's.
//
// The two device calls are their flat camera siblings with a handle of rm_swept_build whose blob the launch walks: they touch no
// render state and keep none of their own, one launch (three steps for the converging call) on the caller's stream, nothing
// waited for.  No extents call of their own: the boxes are in world space and do not care where a ray starts.
// rm_swept_tick_info reads what the ticks left in the context and launches nothing.

extern "C" {

rm_status rm_accumulate_camera_swept_device(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *device_table,
                                            const void *device_camera_rows, const void *device_light_offsets, uint32_t n_lights,
                                            const void *device_shape_offsets, uint32_t n_shapes, const rm_swept *swept, uint32_t n_before,
                                            void *device_sum, void *device_mean, void *device_rgb8, void *hip_stream) {
    const char *who = "rm_accumulate_camera_swept_device";
    return guarded(ctx, who, [&]() -> rm_status {
        if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
        if (rm_status cst = check_accum_device(ctx, who, p, lens, device_table, n_before, device_sum, device_mean)) return cst;
        // (without a shape table nothing moves, and rm_accumulate_camera_device keeps the hierarchy)
        if (!device_shape_offsets) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL shape offsets");
        if (rm_status tst = check_camera_tables(ctx, who, device_camera_rows, device_light_offsets, n_lights, device_shape_offsets, n_shapes)) return tst;
        if (rm_status sst = check_swept(ctx, who, swept)) return sst;
        if (refine_rows(p) == 0u) return RM_OK;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        return launch_camera_over(ctx, n_shapes > 0u ? swept : nullptr,
                                  accum_call{p, lens, device_table, n_before, device_sum, device_mean, device_rgb8, (hipStream_t)hip_stream},
                                  n_lights > 0u ? device_light_offsets : nullptr, n_shapes > 0u ? device_shape_offsets : nullptr, device_camera_rows);
    });
}

rm_status rm_accumulate_converging_camera_swept_device(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c,
                                                       const void *device_table, uint32_t table_rows, const void *device_camera_rows,
                                                       const void *device_light_offsets, uint32_t n_lights, const void *device_shape_offsets,
                                                       uint32_t n_shapes, const rm_swept *swept, int fresh, const rm_converge_frame *b,
                                                       void *hip_stream) {
    const char *who = "rm_accumulate_converging_camera_swept_device";
    return guarded(ctx, who, [&]() -> rm_status {
        if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
        auto tables = [&]() -> rm_status {
            if (!device_shape_offsets) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL shape offsets");
            return check_camera_tables(ctx, who, device_camera_rows, device_light_offsets, n_lights, device_shape_offsets, n_shapes);
        };
        if (rm_status cst = check_converge_call(ctx, who, p, lens, c, device_table, table_rows, b, tables)) return cst;
        if (rm_status sst = check_swept(ctx, who, swept)) return sst;
        if (refine_rows(p) == 0u) return RM_OK;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        return launch_converge_camera_over(ctx, n_shapes > 0u ? swept : nullptr, p, lens, c, device_table, table_rows,
                                           n_lights > 0u ? device_light_offsets : nullptr, n_shapes > 0u ? device_shape_offsets : nullptr,
                                           device_camera_rows, fresh, b, (hipStream_t)hip_stream);
    });
}

rm_status rm_swept_tick_info(rm_ctx *ctx, rm_swept_tick_report *out) {
    const char *who = "rm_swept_tick_info";
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
    if (!out) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL out");
    out->walked_swept = ctx->swept_walked;
    out->builds = ctx->swept_builds;
    return RM_OK;
}

}  // extern "C"
