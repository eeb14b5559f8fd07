// rm_motion_shapes_host.inc -- host side of the moving shapes (include/rusty_marcher_amd.h, "moving shapes"); included at the end
// of rm_device.hip, behind rm_motion_host.inc whose argument block (MotionArgs), tick (rm_render_progressive_impl) and staged
// tables it uses, and rm_accum_host.inc whose checks (check_accum_device, check_offset_tables, check_rules).  The kernel is
// rm_motion_shapes.hip's.
//
// rm_accumulate_moving_device touches no render state and keeps none of its own: one launch on the caller's stream, nothing
// waited for.  rm_render_progressive_moving is rm_render_progressive_motion's tick with every shape free to move; where the
// resident image holds a hierarchy it walks one swept over the velocities and the shutter (rm_swept_host.inc), to the same bytes.

// The launch; offsets: NULL where the scene has no lights; shape_offsets: NULL where it has no shapes.
static rm_status launch_moving(rm_ctx *ctx, const accum_call &c, const void *offsets, const void *shape_offsets) {
    MotionArgs a{};
    a.S.A = accum_args(ctx, c);
    a.S.offsets = static_cast<const double *>(offsets);
    a.shape_offsets = static_cast<const double *>(shape_offsets);
    a.pid_map = ctx->d_pid_map;
    a.n_shapes = resident_shape_count(ctx);
    return launch_shading(ctx, shade_family{"moving shapes", rm_motion_shapes_kernel}, a.S.A.L.max_depth, lens_extent(ctx, a.S.A.L), a, c.stream);
}

// The ticks' hierarchy (rm_swept_host.inc, behind this file; tick_swept_prepare and tick_swept_done are declared in
// rm_motion_host.inc): the launch that walks it where it is ready -- launch_moving where it is not
static rm_status launch_moving_tick(rm_ctx *ctx, const accum_call &c, const void *offsets, const void *shape_offsets);

extern "C" {

rm_status rm_accumulate_moving_device(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *device_table,
                                      const void *device_light_offsets, uint32_t n_lights, const void *device_shape_offsets,
                                      uint32_t n_shapes, uint32_t n_before, void *device_sum, void *device_mean, void *device_rgb8,
                                      void *hip_stream) {
    const char *who = "rm_accumulate_moving_device";
    return guarded(ctx, who, [&]() -> rm_status {
        if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
        if (rm_status cst = check_accum_device(ctx, who, p, lens, device_table, n_before, device_sum, device_mean)) return cst;
        const shape_table shapes{device_shape_offsets, n_shapes};
        if (rm_status ost = check_offset_tables(ctx, who, "light offsets", device_light_offsets, n_lights, &shapes)) return ost;
        // (a row of every shape is read, not of the spheres alone)
        if (n_shapes > 0u && !device_shape_offsets) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL shape offsets");
        if (refine_rows(p) == 0u) return RM_OK;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        return launch_moving(ctx, accum_call{p, lens, device_table, n_before, device_sum, device_mean, device_rgb8, (hipStream_t)hip_stream},
                             n_lights > 0u ? device_light_offsets : nullptr, n_shapes > 0u ? device_shape_offsets : nullptr);
    });
}

rm_status rm_render_progressive_moving(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const double *radii, uint32_t n_lights,
                                       const rm_vec3 *velocities, uint32_t n_shapes, double shutter, int restart, double *host_rgb,
                                       uint8_t *host_rgb8, uint32_t *n_total, rm_timing *timing) {
    return guarded(ctx, "rm_render_progressive_moving", [&]() -> rm_status {
        const tick_swept_scope done{ctx};
        if (rm_status pst = tick_swept_prepare(ctx, "rm_render_progressive_moving", velocities, n_shapes, shutter, false)) return pst;
        const rm_status st = rm_render_progressive_impl(ctx, "rm_render_progressive_moving", params, lens,
                                                        rules_with_motion(radii, n_lights, velocities, n_shapes, shutter), restart, host_rgb,
                                                        host_rgb8, n_total, timing, launch_moving_tick);
        return st;
    });
}

}  // extern "C"
