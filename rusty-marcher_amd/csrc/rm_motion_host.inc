// rm_motion_host.inc -- host side of the moving spheres (include/rusty_marcher_amd.h, "moving spheres"); included at the end of
// rm_device.hip, behind rm_soft_host.inc whose checks (check_soft_lights, and through it check_accum_device) it shares, and
// rm_accum_host.inc whose sequence arithmetic (radical_inverse) and tick (rm_render_progressive_impl, which stages the three
// slices and calls launch_motion below) it shares.  The kernel is rm_motion.hip's.
//
// rm_accumulate_motion_device touches no render state and keeps none of its own: one launch on the caller's stream, nothing
// waited for.  rm_render_progressive_motion is rm_render_progressive_soft with the velocities and the shutter in the frame's key.

// The shape list of the resident scene: the description's first array, kept by the upload (rm_ctx::desc_bytes)
static uint32_t resident_shape_count(const rm_ctx *ctx) { return (uint32_t)(ctx->desc_sizes[0] / sizeof(rm_shape_ref)); }

static rm_shape_ref resident_shape(const rm_ctx *ctx, uint32_t k) {
    rm_shape_ref r;
    std::memcpy(&r, ctx->desc_bytes.data() + (size_t)k * sizeof(rm_shape_ref), sizeof r);
    return r;
}

// n_shapes of a motion call: the resident scene's
static rm_status check_motion_shapes(rm_ctx *ctx, const char *who, uint32_t n_shapes) {
    if (n_shapes != resident_shape_count(ctx)) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "%s: n_shapes %u, the resident scene has %u", who, n_shapes, resident_shape_count(ctx));
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    return RM_OK;
}

// Velocities are finite and the shutter is a finite number >= 0 (a NaN fails the comparison); ctx may be NULL (rm_motion_sequence
// has none)
static rm_status check_velocities(rm_ctx *ctx, const char *who, const rm_vec3 *velocities, uint32_t n_shapes, double shutter) {
    if (n_shapes > 0u && !velocities) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL velocities");
    for (uint32_t k = 0; k < n_shapes; k++)
        if (!finite3(velocities[k])) {
            char buf[192];
            std::snprintf(buf, sizeof buf, "%s: velocities[%u] = (%g, %g, %g) is not finite", who, k, velocities[k].x, velocities[k].y, velocities[k].z);
            return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
        }
    if (!std::isfinite(shutter) || !(shutter >= 0.)) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "%s: shutter = %g is not a finite number >= 0", who, shutter);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    return RM_OK;
}

// What the tick checks of its velocities (behind check_accum: a scene is resident): the count, the numbers, and that only spheres move
static rm_status check_motion_tick(rm_ctx *ctx, const char *who, const rm_motion_tick &m) {
    if (rm_status sst = check_motion_shapes(ctx, who, m.n_shapes)) return sst;
    if (rm_status vst = check_velocities(ctx, who, m.velocities, m.n_shapes, m.shutter)) return vst;
    for (uint32_t k = 0; k < m.n_shapes; k++) {
        const rm_vec3 &v = m.velocities[k];
        if (resident_shape(ctx, k).kind != RM_SHAPE_SPHERE && (v.x != 0. || v.y != 0. || v.z != 0.)) {
            char buf[192];
            std::snprintf(buf, sizeof buf, "%s: velocities[%u] is not zero and shape %u is not a sphere (only spheres move)", who, k, k);
            return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
        }
    }
    return RM_OK;
}

// The launch on `stream`; everything was checked, rows > 0.  offsets: NULL where the scene has no lights; shape_offsets: NULL
// where it has no spheres.
static rm_status launch_motion(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *table, const void *offsets,
                               const void *shape_offsets, uint32_t n_before, void *sum, void *mean, void *rgb8, hipStream_t stream) {
    MotionArgs a{};
    a.S.A.L = lens_args(ctx, p, lens, table, nullptr);
    a.S.A.n_before = n_before;
    a.S.A.sum = static_cast<double *>(sum);
    a.S.A.mean = static_cast<double *>(mean);
    a.S.A.rgb8 = static_cast<uint8_t *>(rgb8);
    a.S.offsets = static_cast<const double *>(offsets);
    a.shape_offsets = static_cast<const double *>(shape_offsets);
    a.pid_map = ctx->d_pid_map;
    a.n_shapes = resident_shape_count(ctx);
    return launch_shading(ctx, shade_family{"moving spheres", rm_motion_kernel}, a.S.A.L.max_depth, lens_extent(ctx, a.S.A.L), a, stream);
}

static rm_status rm_accumulate_motion_device_impl(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *device_table,
                                                  const void *device_light_offsets, uint32_t n_lights, const void *device_shape_offsets,
                                                  uint32_t n_shapes, uint32_t n_before, void *device_sum, void *device_mean,
                                                  void *device_rgb8, void *hip_stream) {
    const char *who = "rm_accumulate_motion_device";
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
    if (rm_status cst = check_accum_device(ctx, who, p, lens, device_table, n_before, device_sum, device_mean)) return cst;
    if (rm_status lst = check_soft_lights(ctx, who, n_lights)) return lst;
    if (n_lights > 0u && !device_light_offsets) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL light offsets");
    if (rm_status sst = check_motion_shapes(ctx, who, n_shapes)) return sst;
    const bool has_spheres = ctx->image.H.n_spheres > 0u;
    if (has_spheres && !device_shape_offsets) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL shape offsets");
    if (refine_rows(p) == 0u) return RM_OK;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    return launch_motion(ctx, p, lens, device_table, n_lights > 0u ? device_light_offsets : nullptr,
                         has_spheres ? device_shape_offsets : nullptr, n_before, device_sum, device_mean, device_rgb8, (hipStream_t)hip_stream);
}

extern "C" {

rm_status rm_motion_sequence(uint32_t first, uint32_t count, const rm_vec3 *velocities, uint32_t n_shapes, double shutter, double *offsets) {
    const char *who = "rm_motion_sequence";
    if ((uint64_t)first + count > RM_PROGRESSIVE_MAX_SAMPLES) {
        char buf[128];
        std::snprintf(buf, sizeof buf, "%s: first + count = %u + %u is more than %u", who, first, count, RM_PROGRESSIVE_MAX_SAMPLES);
        return ctx_fail(nullptr, RM_ERR_INVALID_ARG, buf);
    }
    if (count == 0u || n_shapes == 0u) return RM_OK;
    if (rm_status vst = check_velocities(nullptr, who, velocities, n_shapes, shutter)) return vst;
    if (!offsets) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL offsets");
    for (uint32_t k = 0; k < count; k++) {
        const double t = shutter * radical_inverse(first + k, 17u);      // (row 0: t = 0, the scene as uploaded)
        for (uint32_t j = 0; j < n_shapes; j++) {
            double *o = offsets + ((size_t)k * n_shapes + j) * 3u;
            o[0] = velocities[j].x * t;
            o[1] = velocities[j].y * t;
            o[2] = velocities[j].z * t;
        }
    }
    return RM_OK;
}

rm_status rm_accumulate_motion_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const void *device_table,
                                      const void *device_light_offsets, uint32_t n_lights, const void *device_shape_offsets,
                                      uint32_t n_shapes, uint32_t n_before, void *device_sum, void *device_mean, void *device_rgb8,
                                      void *hip_stream) {
    return guarded(ctx, "rm_accumulate_motion_device", [&]() {
        return rm_accumulate_motion_device_impl(ctx, params, lens, device_table, device_light_offsets, n_lights, device_shape_offsets, n_shapes,
                                                n_before, device_sum, device_mean, device_rgb8, hip_stream);
    });
}

rm_status rm_render_progressive_motion(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const double *radii, uint32_t n_lights,
                                       const rm_vec3 *velocities, uint32_t n_shapes, double shutter, int restart, double *host_rgb,
                                       uint8_t *host_rgb8, uint32_t *n_total, rm_timing *timing) {
    return guarded(ctx, "rm_render_progressive_motion", [&]() {
        const rm_motion_tick motion{velocities, n_shapes, shutter};
        const bool soft = radii != nullptr;                              // (NULL: point lights, n_lights is not looked at)
        return rm_render_progressive_impl(ctx, "rm_render_progressive_motion", params, lens, soft, radii, soft ? n_lights : 0u, restart, host_rgb,
                                          host_rgb8, n_total, timing, &motion);
    });
}

}  // extern "C"
