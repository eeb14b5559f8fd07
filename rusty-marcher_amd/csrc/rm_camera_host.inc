// rm_camera_host.inc -- host side of the moving camera in progressive and in converging frames (include/rusty_marcher_amd.h,
// "moving camera" and "converging frames with a moving camera"); included at the end of rm_device.hip, behind every file whose
// pieces it uses: rm_accum_host.inc (check_accum_device, check_offset_tables, accum_args), rm_motion_host.inc (MotionArgs, the
// tick rm_render_progressive_impl), rm_motion_shapes_host.inc (launch_moving, which tells the tick that any shape may move),
// rm_converge_host.inc (check_converge_call, converge_args, launch_converge_with), rm_converge_motion_host.inc (the tick
// rm_render_converging_impl), rm_converge_moving_host.inc (launch_converge_moving) and rm_swept_host.inc (the ticks' swept
// hierarchy).  The kernels are rm_camera.hip's and rm_converge_camera.hip's and, over a swept hierarchy, rm_camera_swept.hip's
// and rm_converge_camera_swept.hip's; the select kernel is rm_converge.hip's; rm_camera_sequence is rm_camera_motion.cpp's.
//
// The device calls touch no render state and keep none of their own.  The ticks are their families' on the same context-owned
// state with one staged table more and frames of their own (rm_sampling_rules::camera).
//
// Which family a launch takes: the moving scene's kernels where it is handed a shape table, else the static scene's, which keep
// the hierarchy.  The moving scene's walk flat, or the hierarchy of `swept` where one is given (rm_camera_swept_host.inc's device
// calls: the caller's handle; the ticks: their own, where tick_swept_prepare made it ready).

static rm_status launch_camera_over(rm_ctx *ctx, const rm_swept *swept, const accum_call &c, const void *offsets, const void *shape_offsets,
                                    const void *camera_rows) {
    CameraArgs a{};
    a.M.S.A = accum_args(ctx, c);
    a.M.S.offsets = static_cast<const double *>(offsets);
    a.M.shape_offsets = static_cast<const double *>(shape_offsets);
    a.M.pid_map = ctx->d_pid_map;
    a.M.n_shapes = resident_shape_count(ctx);
    a.camera_rows = static_cast<const double *>(camera_rows);
    const LensArgs &L = a.M.S.A.L;
    const shade_family still{"moving camera", rm_camera_kernel}, moving{"moving camera and shapes", rm_camera_moving_kernel};
    if (swept && shape_offsets)
        return launch_shading(ctx, shade_family{"moving camera over a swept hierarchy", rm_camera_swept_kernel, swept->d_blob}, L.max_depth,
                              lens_extent(ctx, L), a, c.stream);
    return launch_shading(ctx, shape_offsets ? moving : still, L.max_depth, lens_extent(ctx, L), a, c.stream);
}

// The ticks' launch, and theirs alone (the device calls name their hierarchy, or none, to launch_camera_over themselves and
// never look at the ticks' state): the ticks' own hierarchy where tick_swept_prepare made it ready
static rm_status launch_camera(rm_ctx *ctx, const accum_call &c, const void *offsets, const void *shape_offsets, const void *camera_rows) {
    const rm_swept *s = tick_swept_ready(ctx, shape_offsets);
    if (s) ctx->swept_walked = 1u;
    return launch_camera_over(ctx, s, c, offsets, shape_offsets, camera_rows);
}

static rm_status launch_converge_camera_over(rm_ctx *ctx, const rm_swept *swept, const rm_params *p, const rm_lens *lens, const rm_converge *c,
                                             const void *table, uint32_t table_rows, const void *offsets, const void *shape_offsets,
                                             const void *camera_rows, int fresh, const rm_converge_frame *b, hipStream_t stream) {
    ConvergeCameraArgs m{};
    m.M.C = converge_args(ctx, p, lens, c, table, table_rows, offsets, fresh, b);
    m.M.shape_offsets = static_cast<const double *>(shape_offsets);
    m.M.pid_map = ctx->d_pid_map;
    m.M.n_shapes = resident_shape_count(ctx);
    m.camera_rows = static_cast<const double *>(camera_rows);
    const shade_family still{"converging with a moving camera", rm_converge_camera_kernel},
        moving{"converging with a moving camera and shapes", rm_converge_camera_moving_kernel};
    if (swept && shape_offsets)
        return launch_converge_with(ctx, shade_family{"converging with a moving camera over a swept hierarchy", rm_converge_camera_swept_kernel,
                                                      swept->d_blob}, m, m.M.C, stream);
    return launch_converge_with(ctx, shape_offsets ? moving : still, m, m.M.C, stream);
}

static rm_status launch_converge_camera(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c, const void *table,
                                        uint32_t table_rows, const void *offsets, const void *shape_offsets, const void *camera_rows, int fresh,
                                        const rm_converge_frame *b, hipStream_t stream) {
    const rm_swept *s = tick_swept_ready(ctx, shape_offsets);
    if (s) ctx->swept_walked = 1u;
    return launch_converge_camera_over(ctx, s, p, lens, c, table, table_rows, offsets, shape_offsets, camera_rows, fresh, b, stream);
}

// The tables of both device calls: rm_accumulate_moving_device's checks, but that a NULL shape table is "no shape moves" (n_shapes
// is not looked at then), and the camera's rows
static rm_status check_camera_tables(rm_ctx *ctx, const char *who, const void *camera_rows, const void *light_offsets, uint32_t n_lights,
                                     const void *shape_offsets, uint32_t n_shapes) {
    const shape_table shapes{shape_offsets, n_shapes};
    if (rm_status ost = check_offset_tables(ctx, who, "light offsets", light_offsets, n_lights, shape_offsets ? &shapes : nullptr)) return ost;
    if (!camera_rows) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL camera rows");
    return RM_OK;
}

// The rules of a camera tick: the siblings' with the motion.  velocities == NULL: no shape moves, no shape table is staged and
// the launch takes the static scene's kernels; velocities given, zeros included, are the moving shapes' rules.
static rm_sampling_rules rules_with_camera(const double *radii, uint32_t n_lights, const rm_vec3 *velocities, uint32_t n_shapes, double shutter,
                                           const rm_camera_motion *motion) {
    rm_sampling_rules r = velocities ? rules_with_motion(radii, n_lights, velocities, n_shapes, shutter) : rules_with_radii(radii, n_lights);
    r.shutter = shutter;
    r.camera = motion;
    return r;
}

extern "C" {

rm_status rm_accumulate_camera_device(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *device_table,
                                      const void *device_camera_rows, const void *device_light_offsets, uint32_t n_lights,
                                      const void *device_shape_offsets, uint32_t n_shapes, uint32_t n_before, void *device_sum,
                                      void *device_mean, void *device_rgb8, void *hip_stream) {
    const char *who = "rm_accumulate_camera_device";
    return guarded(ctx, who, [&]() -> rm_status {
        if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
        if (rm_status cst = check_accum_device(ctx, who, p, lens, device_table, n_before, device_sum, device_mean)) return cst;
        if (rm_status tst = check_camera_tables(ctx, who, device_camera_rows, device_light_offsets, n_lights, device_shape_offsets, n_shapes)) return tst;
        if (refine_rows(p) == 0u) return RM_OK;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        return launch_camera_over(ctx, nullptr, accum_call{p, lens, device_table, n_before, device_sum, device_mean, device_rgb8, (hipStream_t)hip_stream},
                                  n_lights > 0u ? device_light_offsets : nullptr, n_shapes > 0u ? device_shape_offsets : nullptr, device_camera_rows);
    });
}

rm_status rm_accumulate_converging_camera_device(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c,
                                                 const void *device_table, uint32_t table_rows, const void *device_camera_rows,
                                                 const void *device_light_offsets, uint32_t n_lights, const void *device_shape_offsets,
                                                 uint32_t n_shapes, int fresh, const rm_converge_frame *b, void *hip_stream) {
    const char *who = "rm_accumulate_converging_camera_device";
    return guarded(ctx, who, [&]() -> rm_status {
        if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
        auto tables = [&]() {
            return check_camera_tables(ctx, who, device_camera_rows, device_light_offsets, n_lights, device_shape_offsets, n_shapes);
        };
        if (rm_status cst = check_converge_call(ctx, who, p, lens, c, device_table, table_rows, b, tables)) return cst;
        if (refine_rows(p) == 0u) return RM_OK;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        return launch_converge_camera_over(ctx, nullptr, p, lens, c, device_table, table_rows, n_lights > 0u ? device_light_offsets : nullptr,
                                           n_shapes > 0u ? device_shape_offsets : nullptr, device_camera_rows, fresh, b, (hipStream_t)hip_stream);
    });
}

rm_status rm_render_progressive_camera(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const double *radii, uint32_t n_lights,
                                       const rm_vec3 *velocities, uint32_t n_shapes, double shutter, const rm_camera_motion *motion,
                                       int restart, double *host_rgb, uint8_t *host_rgb8, uint32_t *n_total, rm_timing *timing) {
    return guarded(ctx, "rm_render_progressive_camera", [&]() -> rm_status {
        const char *who = "rm_render_progressive_camera";
        if (!motion) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL motion");
        // (velocities: any shape may move, so where the image holds a hierarchy the tick walks one swept over them)
        const tick_swept_scope done{ctx};                                  // (however the tick body is left, the hierarchy is no longer ready)
        if (velocities)
            if (rm_status pst = tick_swept_prepare(ctx, who, velocities, n_shapes, shutter, false)) return pst;
        const rm_status st =
            rm_render_progressive_impl(ctx, who, params, lens, rules_with_camera(radii, n_lights, velocities, n_shapes, shutter, motion), restart,
                                       host_rgb, host_rgb8, n_total, timing, velocities ? launch_moving : nullptr);
        return st;
    });
}

rm_status rm_render_converging_camera(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const rm_converge *converge,
                                      const double *radii, uint32_t n_lights, const rm_vec3 *velocities, uint32_t n_shapes, double shutter,
                                      const rm_camera_motion *motion, int restart, double *host_rgb, uint8_t *host_rgb8,
                                      rm_converge_report *report, rm_timing *timing) {
    return guarded(ctx, "rm_render_converging_camera", [&]() -> rm_status {
        const char *who = "rm_render_converging_camera";
        if (!motion) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL motion");
        const tick_swept_scope done{ctx};                                  // (however the tick body is left, the hierarchy is no longer ready)
        if (velocities)
            if (rm_status pst = tick_swept_prepare(ctx, who, velocities, n_shapes, shutter, false)) return pst;
        const rm_status st = rm_render_converging_impl(ctx, who, params, lens, converge,
                                                       rules_with_camera(radii, n_lights, velocities, n_shapes, shutter, motion), restart, host_rgb,
                                                       host_rgb8, report, timing, velocities ? launch_converge_moving : nullptr);
        return st;
    });
}

}  // extern "C"
