// rm_converge_moving_host.inc -- host side of the converging frames with moving shapes (include/rusty_marcher_amd.h, "converging
// frames with moving shapes"); included at the end of rm_device.hip, behind rm_converge_motion_host.inc whose argument block
// (ConvergeMotionArgs), tick (rm_render_converging_impl) and resident prefixes it uses, rm_converge_host.inc whose checks
// (check_converge_call) and launches (converge_args, launch_converge_with), and rm_accum_host.inc whose checks
// (check_offset_tables, check_rules).  The shade kernel is rm_converge_moving.hip's, the select kernel rm_converge.hip's.
//
// rm_accumulate_converging_moving_device touches no render state and keeps all of its own in the caller's buffers, as
// rm_accumulate_converging_motion_device does.  rm_render_converging_moving is rm_render_converging_motion's tick with every
// shape free to move.

// The three steps on `stream`; everything was checked, rows > 0.  offsets: NULL where the scene has no lights; shape_offsets:
// NULL where it has no shapes.
static rm_status launch_converge_moving(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c, const void *table,
                                        uint32_t table_rows, const void *offsets, const void *shape_offsets, int fresh,
                                        const rm_converge_frame *b, hipStream_t stream) {
    ConvergeMotionArgs m{};
    m.C = converge_args(ctx, p, lens, c, table, table_rows, offsets, fresh, b);
    m.shape_offsets = static_cast<const double *>(shape_offsets);
    m.pid_map = ctx->d_pid_map;
    m.n_shapes = resident_shape_count(ctx);
    return launch_converge_with(ctx, shade_family{"converging with moving shapes", rm_converge_moving_kernel}, m, m.C, stream);
}

// The ticks' hierarchy (rm_swept_host.inc, behind this file): the launch that walks it where tick_swept_prepare made it ready --
// launch_converge_moving where not
static rm_status launch_converge_moving_tick(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c, const void *table,
                                             uint32_t table_rows, const void *offsets, const void *shape_offsets, int fresh,
                                             const rm_converge_frame *b, hipStream_t stream);

extern "C" {

rm_status rm_accumulate_converging_moving_device(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c,
                                                 const void *device_table, uint32_t table_rows, const void *device_light_offsets,
                                                 uint32_t n_lights, const void *device_shape_offsets, uint32_t n_shapes, int fresh,
                                                 const rm_converge_frame *b, void *hip_stream) {
    const char *who = "rm_accumulate_converging_moving_device";
    return guarded(ctx, who, [&]() -> rm_status {
        if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
        const shape_table shapes{device_shape_offsets, n_shapes};
        auto tables = [&]() -> rm_status {
            if (rm_status ost = check_offset_tables(ctx, who, "light offsets", device_light_offsets, n_lights, &shapes)) return ost;
            // (a row of every shape is read, not of the spheres alone)
            if (n_shapes > 0u && !device_shape_offsets) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL shape offsets");
            return RM_OK;
        };
        if (rm_status cst = check_converge_call(ctx, who, p, lens, c, device_table, table_rows, b, tables)) return cst;
        if (refine_rows(p) == 0u) return RM_OK;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        return launch_converge_moving(ctx, p, lens, c, device_table, table_rows, n_lights > 0u ? device_light_offsets : nullptr,
                                      n_shapes > 0u ? device_shape_offsets : nullptr, fresh, b, (hipStream_t)hip_stream);
    });
}

rm_status rm_render_converging_moving(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const rm_converge *converge,
                                      const double *radii, uint32_t n_lights, const rm_vec3 *velocities, uint32_t n_shapes, double shutter,
                                      int restart, double *host_rgb, uint8_t *host_rgb8, rm_converge_report *report, rm_timing *timing) {
    return guarded(ctx, "rm_render_converging_moving", [&]() -> rm_status {
        const tick_swept_scope done{ctx};
        if (rm_status pst = tick_swept_prepare(ctx, "rm_render_converging_moving", velocities, n_shapes, shutter, false)) return pst;
        const rm_status st = rm_render_converging_impl(ctx, "rm_render_converging_moving", params, lens, converge,
                                                       rules_with_motion(radii, n_lights, velocities, n_shapes, shutter), restart, host_rgb,
                                                       host_rgb8, report, timing, launch_converge_moving_tick);
        return st;
    });
}

}  // extern "C"
