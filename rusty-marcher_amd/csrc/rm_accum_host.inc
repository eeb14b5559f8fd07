// rm_accum_host.inc -- host side of the progressive frames' device call (include/rusty_marcher_amd.h, "progressive frames"), and
// what the sampled frames behind it share: included at the end of rm_device.hip, behind rm_lens_host.inc whose checks
// (check_lens), argument block (lens_args) and grid (lens_extent, with RM_LENS_MAX_BLOCKS) it reuses.  The kernel is rm_accum.hip's.
//
// Here: the checks of params and lens (check_accum), of a device call's own arguments (check_accum_device) and of its offset
// tables (check_offset_tables), of a tick's sampling rules (check_rules); the AccumArgs part of an argument block (accum_args);
// and rm_accumulate_lens_device, which touches no render state and keeps none of its own: one launch on the caller's stream,
// nothing waited for.  The area lights (rm_soft_host.inc) and the moving spheres (rm_motion_host.inc) add their launches; the
// tick of all three, rm_render_progressive*, stands behind them in rm_motion_host.inc.  The sequences and the frame's identity
// are rm_sampling.cpp's.

// What the entry points check of params and lens (ctx is not NULL): check_lens with a table and a frame that are there.
static rm_status check_accum(rm_ctx *ctx, const char *who, const rm_params *p, const rm_lens *lens) {
    const char present = 0;
    return check_lens(ctx, who, p, lens, &present, &present);
}

// A refusal of rm_sampling.cpp's checks, which know no context: its text becomes the context's
static rm_status host_refusal(rm_ctx *ctx, rm_status st) { return st ? ctx_fail(ctx, st, rm_get_host_error()) : RM_OK; }

// n_lights of a call with a light table or radii: the resident scene's, as rm_lights_visible requires
static rm_status check_soft_lights(rm_ctx *ctx, const char *who, uint32_t n_lights) {
    if (n_lights != ctx->image.H.n_lights) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "%s: n_lights %u, the resident scene has %u", who, n_lights, ctx->image.H.n_lights);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    return RM_OK;
}

// The shape list of the resident scene: the description's first array, kept by the upload (rm_ctx::desc_bytes)
static uint32_t resident_shape_count(const rm_ctx *ctx) { return (uint32_t)(ctx->desc_sizes[0] / sizeof(rm_shape_ref)); }

static rm_shape_ref resident_shape(const rm_ctx *ctx, uint32_t k) {
    rm_shape_ref r;
    std::memcpy(&r, ctx->desc_bytes.data() + (size_t)k * sizeof(rm_shape_ref), sizeof r);
    return r;
}

// n_shapes of a call with a shape table or velocities: the resident scene's
static rm_status check_motion_shapes(rm_ctx *ctx, const char *who, uint32_t n_shapes) {
    if (n_shapes != resident_shape_count(ctx)) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "%s: n_shapes %u, the resident scene has %u", who, n_shapes, resident_shape_count(ctx));
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    return RM_OK;
}

// The offset tables of a device call (behind check_accum_device: a scene is resident): the light table `lights`, which the call
// names `light_name`, and, where `shapes` is not NULL, the shape table *shapes -- read only where the scene has spheres
struct shape_table {
    const void *offsets;
    uint32_t n_shapes;
};
static rm_status check_offset_tables(rm_ctx *ctx, const char *who, const char *light_name, const void *lights, uint32_t n_lights,
                                     const shape_table *shapes = nullptr) {
    if (rm_status lst = check_soft_lights(ctx, who, n_lights)) return lst;
    if (n_lights > 0u && !lights) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL " + light_name);
    if (!shapes) return RM_OK;
    if (rm_status sst = check_motion_shapes(ctx, who, shapes->n_shapes)) return sst;
    if (ctx->image.H.n_spheres > 0u && !shapes->offsets) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL shape offsets");
    return RM_OK;
}

// What a tick checks of its sampling rules (behind check_accum: a scene is resident): the counts, the numbers, and that only
// spheres move -- but in the moving shapes' tick (any_shape; rm_motion_shapes_host.inc), where every shape may
static rm_status check_rules(rm_ctx *ctx, const char *who, const rm_sampling_rules &r, bool any_shape = false) {
    if (r.soft) {
        if (rm_status lst = check_soft_lights(ctx, who, r.n_lights)) return lst;
        if (rm_status rst = host_refusal(ctx, rm_check_radii(who, r.radii, r.n_lights))) return rst;
    }
    if (r.bounce)
        if (rm_status bst = host_refusal(ctx, rm_check_strength(who, r.strength))) return bst;
    if (r.camera) {                                                        // (the moving camera's ticks: a shutter without velocities too)
        if (rm_status mst = host_refusal(ctx, rm_check_camera_motion(who, r.camera))) return mst;
        if (!r.motion)
            if (rm_status sst = host_refusal(ctx, rm_check_velocities(who, nullptr, 0u, r.shutter))) return sst;
    }
    if (!r.motion) return RM_OK;
    if (rm_status sst = check_motion_shapes(ctx, who, r.n_shapes)) return sst;
    if (rm_status vst = host_refusal(ctx, rm_check_velocities(who, r.velocities, r.n_shapes, r.shutter))) return vst;
    for (uint32_t k = 0; k < r.n_shapes && !any_shape; k++) {
        const rm_vec3 &v = r.velocities[k];
        if (resident_shape(ctx, k).kind != RM_SHAPE_SPHERE && (v.x != 0. || v.y != 0. || v.z != 0.)) {
            char buf[192];
            std::snprintf(buf, sizeof buf, "%s: velocities[%u] is not zero and shape %u is not a sphere (only spheres move)", who, k, k);
            return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
        }
    }
    return RM_OK;
}

// The rules of a call that takes radii: NULL is point lights, n_lights is not looked at then
static rm_sampling_rules rules_with_radii(const double *radii, uint32_t n_lights) {
    rm_sampling_rules r;
    r.soft = radii != nullptr;
    r.radii = radii;
    r.n_lights = r.soft ? n_lights : 0u;
    return r;
}

// ... and velocities
static rm_sampling_rules rules_with_motion(const double *radii, uint32_t n_lights, const rm_vec3 *velocities, uint32_t n_shapes, double shutter) {
    rm_sampling_rules r = rules_with_radii(radii, n_lights);
    r.motion = true;
    r.velocities = velocities;
    r.n_shapes = n_shapes;
    r.shutter = shutter;
    return r;
}

// What a launch of the three kernels adds to: the table's slice and the running sum, on `stream`; everything was checked, rows > 0
struct accum_call {
    const rm_params *p;
    const rm_lens *lens;
    const void *table;
    uint32_t n_before;
    void *sum, *mean, *rgb8;
    hipStream_t stream;
};

// The AccumArgs part of an argument block (AccumArgs, SoftArgs::A, MotionArgs::S.A)
static AccumArgs accum_args(rm_ctx *ctx, const accum_call &c) {
    AccumArgs a{};
    a.L = lens_args(ctx, c.p, c.lens, c.table, nullptr);
    a.n_before = c.n_before;
    a.sum = static_cast<double *>(c.sum);
    a.mean = static_cast<double *>(c.mean);
    a.rgb8 = static_cast<uint8_t *>(c.rgb8);
    return a;
}

static rm_status launch_accum(rm_ctx *ctx, const accum_call &c) {
    AccumArgs a = accum_args(ctx, c);
    return launch_shading(ctx, shade_family{"progressive", rm_accum_kernel}, a.L.max_depth, lens_extent(ctx, a.L), a, c.stream);
}

// What the device calls (this one, the area lights', the moving spheres' and the converging frames') check of their own
// arguments (ctx is not NULL).
static rm_status check_accum_device(rm_ctx *ctx, const char *who, const rm_params *p, const rm_lens *lens, const void *device_table,
                                    uint32_t n_before, const void *device_sum, const void *device_mean) {
    if (rm_status cst = check_accum(ctx, who, p, lens)) return cst;
    if (!device_table) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL table");
    if (!device_sum) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL sum");
    if (device_mean == device_sum) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": the mean would overwrite the sum (device_mean == device_sum)");
    if ((uint64_t)n_before + lens->n_samples > RM_PROGRESSIVE_MAX_SAMPLES) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "%s: n_before + n_samples = %u + %u is more than %u", who, n_before, lens->n_samples, RM_PROGRESSIVE_MAX_SAMPLES);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    return RM_OK;
}

extern "C" rm_status rm_accumulate_lens_device(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *device_table, uint32_t n_before,
                                               void *device_sum, void *device_mean, void *device_rgb8, void *hip_stream) {
    const char *who = "rm_accumulate_lens_device";
    return guarded(ctx, who, [&]() -> rm_status {
        if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
        if (rm_status cst = check_accum_device(ctx, who, p, lens, device_table, n_before, device_sum, device_mean)) return cst;
        if (refine_rows(p) == 0u) return RM_OK;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        return launch_accum(ctx, accum_call{p, lens, device_table, n_before, device_sum, device_mean, device_rgb8, (hipStream_t)hip_stream});
    });
}
