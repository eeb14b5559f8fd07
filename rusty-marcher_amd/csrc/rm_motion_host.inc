// rm_motion_host.inc -- host side of the moving spheres (include/rusty_marcher_amd.h, "moving spheres") and, behind all three
// launches it can end in, the tick of the progressive frames, the area lights and the moving spheres; included at the end of
// rm_device.hip, behind rm_accum_host.inc whose checks (check_accum, check_accum_device, check_offset_tables, check_rules) and
// argument block (accum_call, accum_args) and rm_soft_host.inc whose launch (launch_soft) it uses.  The kernel is rm_motion.hip's.
//
// rm_accumulate_motion_device touches no render state and keeps none of its own: one launch on the caller's stream, nothing
// waited for.  rm_render_progressive is a launch on the context's stream with a staged slice of rm_lens_sequence and three
// buffers the context owns (sum, mean, bytes: not the resident frame, not the lens frame), the count of samples in the sum and
// the identity of the frame the sum belongs to (rm_sampling.hpp).  rm_render_progressive_soft is that with radii in the rules
// and a slice of rm_light_sequence staged, rm_render_progressive_motion with velocities and a shutter as well and a slice of
// rm_motion_sequence: which tables a tick stages is rm_staging_of's rule.  rm_render_progressive_moving
// (rm_motion_shapes_host.inc, behind this file) is the fourth: the motion tick with every shape free to move.

// The launch; offsets: NULL where the scene has no lights; shape_offsets: NULL where it has no spheres.
static rm_status launch_motion(rm_ctx *ctx, const accum_call &c, const void *offsets, const void *shape_offsets) {
    MotionArgs a{};
    a.S.A = accum_args(ctx, c);
    a.S.offsets = static_cast<const double *>(offsets);
    a.shape_offsets = static_cast<const double *>(shape_offsets);
    a.pid_map = ctx->d_pid_map;
    a.n_shapes = resident_shape_count(ctx);
    return launch_shading(ctx, shade_family{"moving spheres", rm_motion_kernel}, a.S.A.L.max_depth, lens_extent(ctx, a.S.A.L), a, c.stream);
}

// A launch with launch_motion's arguments: the moving shapes' tick (rm_motion_shapes_host.inc) hands the tick below its own
using motion_launch = rm_status (*)(rm_ctx *ctx, const accum_call &c, const void *offsets, const void *shape_offsets);

// The moving camera's launch (rm_camera_host.inc, behind this file): launch_moving's with the camera's rows; shape_offsets NULL:
// no shape moves
static rm_status launch_camera(rm_ctx *ctx, const accum_call &c, const void *offsets, const void *shape_offsets, const void *camera_rows);

// The diffuse bounce's launch (rm_bounce_host.inc, behind this file): launch_soft's with the bounce table and the strength
static rm_status launch_bounce(rm_ctx *ctx, const accum_call &c, const void *offsets, const void *bounce, double strength);

// The ticks' swept hierarchy (rm_swept_host.inc, behind this file): made ready in front of a tick that moves a shape for its
// velocities and shutter (`spheres_only`: the moving spheres' ticks, whose rule it applies), and the moving spheres' launch that
// walks it where it is ready -- launch_motion where it is not
static rm_status tick_swept_prepare(rm_ctx *ctx, const char *who, const rm_vec3 *velocities, uint32_t n_shapes, double shutter,
                                    bool spheres_only);
static void tick_swept_done(rm_ctx *ctx);
// ... and tick_swept_done when the scope is left, by a return or by an exception on its way to `guarded`: a hierarchy left ready
// would be walked by the next tick that prepared none
struct tick_swept_scope {
    rm_ctx *ctx;
    ~tick_swept_scope() { tick_swept_done(ctx); }
};
static rm_status launch_motion_tick(rm_ctx *ctx, const accum_call &c, const void *offsets, const void *shape_offsets);

// The basis rm_camera_get reports: the context's where it is oriented, else the fixed view's
static rm_camera_basis reported_basis(const rm_ctx *ctx) {
    const rm_camera_basis fixed{{1., 0., 0.}, {0., 1., 0.}, {0., 0., -1.}};
    return ctx->oriented ? ctx->basis : fixed;
}

// A staged slice of an offset sequence: host side and device side, grown on demand
struct rm_staged_slice {
    std::vector<double> host;
    void *d = nullptr;
    size_t bytes = 0;                        // d has room for that many
};

// The progressive state of a context (rm_ctx::progressive; made on the first call, released by rm_destroy)
struct rm_progressive {
    void *d_table = nullptr;                 // RM_LENS_MAX_SAMPLES rows
    void *d_sum = nullptr, *d_mean = nullptr, *d_rgb8 = nullptr;
    size_t pixels = 0;                       // the three buffers have room for that many
    double table[RM_LENS_MAX_SAMPLES * 4u];  // the slice as staged
    bool have_key = false;                   // a call has succeeded, and nothing failed half-way since
    rm_frame_identity id;                    // the frame the sum belongs to
    uint32_t n = 0;                          // samples a pixel in the sum
    rm_staged_slice lights, shapes;          // the slices of rm_light_sequence (or zeros) and of rm_motion_sequence
    rm_staged_slice camera;                  // ... and of rm_camera_sequence (the moving camera's tick)
    rm_staged_slice bounce;                  // ... and of rm_bounce_sequence (the diffuse bounce's tick)
};

static void progressive_destroy(rm_ctx *ctx, bool device_ok) {
    rm_progressive *g = ctx->progressive;
    if (!g) return;
    for (void *b : {g->d_table, g->d_sum, g->d_mean, g->d_rgb8, g->lights.d, g->shapes.d, g->camera.d, g->bounce.d})
        if (b && device_ok) (void)hipFree(b);
    delete g;
    ctx->progressive = nullptr;
}

// `doubles` doubles of fill(out) into the slice and on their way to the device, on the context's stream; 0: nothing is staged
template <class FILL>
static rm_status stage_slice(rm_ctx *ctx, rm_staged_slice &s, size_t doubles, FILL fill) {
    if (doubles == 0u) return RM_OK;
    if (rm_status gst = grow_device_buffer(ctx, &s.d, &s.bytes, doubles * sizeof(double))) return gst;
    s.host.resize(doubles);
    if (rm_status sst = fill(s.host.data())) return sst;
    RM_HIP(ctx, hipMemcpyAsync(s.d, s.host.data(), doubles * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return RM_OK;
}

// The tick of the six calls; `rules` says which (rules.bounce: the diffuse bounce's, rm_bounce_host.inc, which stages a slice of
// rm_bounce_sequence as well and launches its own kernel; rules.camera: the moving camera's, rm_camera_host.inc, which stages a slice
// of rm_camera_sequence as well and launches its own kernels), and `any_shape`, the moving shapes' launch, tells their tick (a motion tick in
// which a velocity on any shape is obeyed; key.motion = 2 keeps its frames apart from the moving spheres') from the moving
// spheres': checked here, the tables they ask for staged, the launch by them.
static rm_status rm_render_progressive_impl(rm_ctx *ctx, const char *who, const rm_params *p, const rm_lens *lens, const rm_sampling_rules &rules,
                                            int restart, double *host_rgb, uint8_t *host_rgb8, uint32_t *n_total, rm_timing *timing,
                                            motion_launch any_shape = nullptr) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
    ctx->swept_walked = 0u;                                                // (until a launch of this tick walks a swept hierarchy)
    const auto t_begin = std::chrono::steady_clock::now();
    if (rm_status cst = check_accum(ctx, who, p, lens)) return cst;
    if (rm_status rst = check_rules(ctx, who, rules, any_shape != nullptr)) return rst;
    const uint32_t rows = refine_rows(p), ns = lens->n_samples;
    const size_t pixels = (size_t)rows * p->frame_width;
    double kernel_ms = 0.;
    if (rows > 0u) {
        if (!ctx->progressive) ctx->progressive = new rm_progressive();
        rm_progressive &g = *ctx->progressive;
        rm_frame_identity id = rm_frame_identity_of(*p, *lens, ctx->camera, ctx->basis, ctx->oriented, ctx->upload_copies, rules);
        if (any_shape) id.key.motion = 2u;
        const uint32_t n_before = !restart && g.have_key && rm_same_frame(g.id, id) ? g.n : 0u;
        const bool saturated = n_before + ns > RM_PROGRESSIVE_MAX_SAMPLES;     // (then n_before > 0: the frame stands)
        RM_HIP(ctx, hipSetDevice(ctx->device));
        if (!saturated) {
            g.have_key = false;                                            // (until this call is through)
            if (!g.d_table) RM_HIP(ctx, hipMalloc(&g.d_table, sizeof g.table));
            if (rm_status gst = grow_frame_buffers(ctx, &g.pixels, pixels, {{&g.d_sum, pixels * 3u * sizeof(double)},
                                                                            {&g.d_mean, pixels * 3u * sizeof(double)}, {&g.d_rgb8, pixels * 3u}}))
                return gst;
            if (rm_status sst = rm_fill_lens_rows(n_before, ns, g.table)) return sst;
            RM_HIP(ctx, hipMemcpyAsync(g.d_table, g.table, (size_t)ns * 4u * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            const rm_staging staged = rm_staging_of(RM_TICK_PROGRESSIVE, rules, ctx->image.H.n_lights, ctx->image.H.n_spheres, resident_shape_count(ctx));
            if (rm_status sst = stage_slice(ctx, g.lights, (size_t)ns * staged.light_columns * 3u,
                                            [&](double *out) { return rm_fill_light_rows(rules, staged, n_before, ns, out); }))
                return sst;
            if (rm_status sst = stage_slice(ctx, g.shapes, (size_t)ns * staged.shape_columns * 3u,
                                            [&](double *out) { return rm_fill_shape_rows(rules, n_before, ns, out); }))
                return sst;
            if (rules.camera) {
                const rm_camera_basis basis = reported_basis(ctx);
                if (rm_status sst = stage_slice(ctx, g.camera, (size_t)ns * 12u, [&](double *out) {
                        return host_refusal(ctx, rm_camera_sequence(n_before, ns, rules.camera, &basis, rules.shutter, out));
                    }))
                    return sst;
            }
            if (rm_status sst = stage_slice(ctx, g.bounce, (size_t)ns * staged.bounce_columns,
                                            [&](double *out) { return rm_fill_bounce_rows(n_before, ns, out); }))
                return sst;
            const accum_call call{p, lens, g.d_table, n_before, g.d_sum, g.d_mean, g.d_rgb8, ctx->stream};
            const void *lights = staged.light_columns > 0u ? g.lights.d : nullptr, *shapes = staged.shape_columns > 0u ? g.shapes.d : nullptr;
            auto launch = [&]() {
                if (rules.camera) return launch_camera(ctx, call, lights, shapes, g.camera.d);
                if (any_shape) return any_shape(ctx, call, lights, shapes);
                if (rules.bounce) return launch_bounce(ctx, call, lights, g.bounce.d, rules.strength);
                return rules.motion ? launch_motion_tick(ctx, call, lights, shapes) : rules.soft ? launch_soft(ctx, call, lights) : launch_accum(ctx, call);
            };
            if (rm_status lst = timed_launch(ctx, &kernel_ms, launch)) return lst;
            g.id = std::move(id);
            g.n = n_before + ns;
            g.have_key = true;
        }
    }
    const rm_progressive *g = rows > 0u ? ctx->progressive : nullptr;
    if (rm_status fst = finish_tick(ctx, pixels, g ? g->d_mean : nullptr, g ? g->d_rgb8 : nullptr, host_rgb, host_rgb8, kernel_ms, timing, t_begin))
        return fst;
    if (n_total) *n_total = g ? g->n : 0u;
    return RM_OK;
}

extern "C" {

rm_status rm_accumulate_motion_device(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *device_table,
                                      const void *device_light_offsets, uint32_t n_lights, const void *device_shape_offsets,
                                      uint32_t n_shapes, uint32_t n_before, void *device_sum, void *device_mean, void *device_rgb8,
                                      void *hip_stream) {
    const char *who = "rm_accumulate_motion_device";
    return guarded(ctx, who, [&]() -> rm_status {
        if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
        if (rm_status cst = check_accum_device(ctx, who, p, lens, device_table, n_before, device_sum, device_mean)) return cst;
        const shape_table shapes{device_shape_offsets, n_shapes};
        if (rm_status ost = check_offset_tables(ctx, who, "light offsets", device_light_offsets, n_lights, &shapes)) return ost;
        if (refine_rows(p) == 0u) return RM_OK;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        return launch_motion(ctx, accum_call{p, lens, device_table, n_before, device_sum, device_mean, device_rgb8, (hipStream_t)hip_stream},
                             n_lights > 0u ? device_light_offsets : nullptr, ctx->image.H.n_spheres > 0u ? device_shape_offsets : nullptr);
    });
}

rm_status rm_render_progressive(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, int restart, double *host_rgb, uint8_t *host_rgb8,
                                uint32_t *n_total, rm_timing *timing) {
    return guarded(ctx, "rm_render_progressive", [&]() {
        return rm_render_progressive_impl(ctx, "rm_render_progressive", params, lens, rm_sampling_rules{}, restart, host_rgb, host_rgb8, n_total, timing);
    });
}

rm_status rm_render_progressive_soft(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const double *radii, uint32_t n_lights,
                                     int restart, double *host_rgb, uint8_t *host_rgb8, uint32_t *n_total, rm_timing *timing) {
    return guarded(ctx, "rm_render_progressive_soft", [&]() {
        rm_sampling_rules rules;
        rules.soft = true;                                               // (NULL radii are no point lights here: refused where the scene has lights)
        rules.radii = radii;
        rules.n_lights = n_lights;
        return rm_render_progressive_impl(ctx, "rm_render_progressive_soft", params, lens, rules, restart, host_rgb, host_rgb8, n_total, timing);
    });
}

rm_status rm_render_progressive_motion(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const double *radii, uint32_t n_lights,
                                       const rm_vec3 *velocities, uint32_t n_shapes, double shutter, int restart, double *host_rgb,
                                       uint8_t *host_rgb8, uint32_t *n_total, rm_timing *timing) {
    return guarded(ctx, "rm_render_progressive_motion", [&]() -> rm_status {
        const tick_swept_scope done{ctx};
        if (rm_status pst = tick_swept_prepare(ctx, "rm_render_progressive_motion", velocities, n_shapes, shutter, true)) return pst;
        return rm_render_progressive_impl(ctx, "rm_render_progressive_motion", params, lens,
                                          rules_with_motion(radii, n_lights, velocities, n_shapes, shutter), restart, host_rgb, host_rgb8, n_total,
                                          timing);
    });
}

}  // extern "C"
