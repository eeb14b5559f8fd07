// rm_converge_motion_host.inc -- host side of the converging frames with moving spheres (include/rusty_marcher_amd.h,
// "converging frames with moving spheres"); included at the end of rm_device.hip, behind rm_converge_host.inc whose checks
// (check_converge), argument block (converge_args), three steps (launch_converge_with) and tick (rm_render_converging_impl, which
// keeps the three resident prefixes and calls launch_converge_motion below) it shares, and rm_motion_host.inc whose checks
// (check_motion_shapes, check_motion_tick).  The shade kernel is rm_converge_motion.hip's, the select kernel rm_converge.hip's.
//
// rm_accumulate_converging_motion_device touches no render state and keeps all of its own in the caller's buffers, as
// rm_accumulate_converging_device does.  rm_render_converging_motion is rm_render_converging with the velocities and the shutter
// in the frame's key, on the same state (rm_ctx::converging).

// The three steps on `stream`; everything was checked, rows > 0.  offsets: NULL where the scene has no lights; shape_offsets:
// NULL where it has no spheres.
static rm_status launch_converge_motion(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c, const void *table,
                                        uint32_t table_rows, const void *offsets, const void *shape_offsets, int fresh,
                                        const rm_converge_frame *b, hipStream_t stream) {
    ConvergeMotionArgs m{};
    m.C = converge_args(ctx, p, lens, c, table, table_rows, offsets, fresh, b);
    m.shape_offsets = static_cast<const double *>(shape_offsets);
    m.pid_map = ctx->d_pid_map;
    m.n_shapes = resident_shape_count(ctx);
    return launch_converge_with(ctx, shade_family{"converging with moving spheres", rm_converge_motion_kernel}, m, m.C, stream);
}

static rm_status rm_accumulate_converging_motion_device_impl(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c,
                                                             const void *device_table, uint32_t table_rows,
                                                             const void *device_light_offsets, uint32_t n_lights,
                                                             const void *device_shape_offsets, uint32_t n_shapes, int fresh,
                                                             const rm_converge_frame *b, void *hip_stream) {
    const char *who = "rm_accumulate_converging_motion_device";
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
    if (!b) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL buffers");
    if (rm_status cst = check_accum_device(ctx, who, p, lens, device_table, 0u, b->sum, b->mean)) return cst;
    if (rm_status lst = check_soft_lights(ctx, who, n_lights)) return lst;
    if (n_lights > 0u && !device_light_offsets) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL light offsets");
    if (rm_status sst = check_motion_shapes(ctx, who, n_shapes)) return sst;
    const bool has_spheres = ctx->image.H.n_spheres > 0u;
    if (has_spheres && !device_shape_offsets) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL shape offsets");
    if (rm_status vst = check_converge(ctx, who, lens, c, table_rows)) return vst;
    if (!b->stats) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL stats");
    if (!b->count) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL count");
    if (!b->workspace) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL workspace");
    if (refine_rows(p) == 0u) return RM_OK;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    return launch_converge_motion(ctx, p, lens, c, device_table, table_rows, n_lights > 0u ? device_light_offsets : nullptr,
                                  has_spheres ? device_shape_offsets : nullptr, fresh, b, (hipStream_t)hip_stream);
}

extern "C" {

rm_status rm_accumulate_converging_motion_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const rm_converge *converge,
                                                 const void *device_table, uint32_t table_rows, const void *device_light_offsets,
                                                 uint32_t n_lights, const void *device_shape_offsets, uint32_t n_shapes, int fresh,
                                                 const rm_converge_frame *buffers, void *hip_stream) {
    return guarded(ctx, "rm_accumulate_converging_motion_device", [&]() {
        return rm_accumulate_converging_motion_device_impl(ctx, params, lens, converge, device_table, table_rows, device_light_offsets, n_lights,
                                                           device_shape_offsets, n_shapes, fresh, buffers, hip_stream);
    });
}

rm_status rm_render_converging_motion(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const rm_converge *converge,
                                      const double *radii, uint32_t n_lights, const rm_vec3 *velocities, uint32_t n_shapes, double shutter,
                                      int restart, double *host_rgb, uint8_t *host_rgb8, rm_converge_report *report, rm_timing *timing) {
    return guarded(ctx, "rm_render_converging_motion", [&]() {
        const rm_motion_tick motion{velocities, n_shapes, shutter};
        return rm_render_converging_impl(ctx, "rm_render_converging_motion", params, lens, converge, radii, n_lights, restart, host_rgb,
                                         host_rgb8, report, timing, &motion);
    });
}

}  // extern "C"
