// rm_lens_host.inc -- host side of the thin-lens camera (include/rusty_marcher_amd.h, "thin-lens camera"); included at the end
// of rm_device.hip, behind rm_refine_host.inc whose row count it shares and rm_radiance_host.inc whose checks.  The kernel is
// rm_lens.hip's.
//
// rm_render_lens_device touches no render state and keeps none of its own: one launch on the caller's stream, nothing waited
// for.  rm_render_lens is that on the context's stream with a table buffer and a frame buffer the context owns, and the copy;
// the resident frame of rm_render is not used.

#define RM_LENS_MAX_SAMPLES 64u

// What both entry points check before anything is launched (ctx is not NULL).
static rm_status check_lens(rm_ctx *ctx, const char *who, const rm_params *p, const rm_lens *lens, const void *table, const void *frame) {
    if (rm_status pst = check_query_params(ctx, p, who)) return pst;
    if (p->frame_width % RM_PATCH_SIZE != 0)
        return ctx_fail(ctx, RM_ERR_DIMENSIONS, std::string(who) + ": frame width is not a multiple of 32 (no render writes such a frame)");
    if ((uint64_t)refine_rows(p) * p->frame_width > 0x7fffffffull)
        return ctx_fail(ctx, RM_ERR_DIMENSIONS, std::string(who) + ": more than 2^31 - 1 pixels");
    if (rm_status cst = check_shading(ctx, who, p->background, p->max_depth)) return cst;
    if (!lens) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL lens");
    char buf[160];
    if (!std::isfinite(lens->aperture) || !(lens->aperture >= 0.)) {
        std::snprintf(buf, sizeof buf, "%s: lens.aperture = %g is not a finite number >= 0", who, lens->aperture);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    if (!std::isfinite(lens->focus) || !(lens->focus > 0.)) {
        std::snprintf(buf, sizeof buf, "%s: lens.focus = %g is not a finite number > 0", who, lens->focus);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    if (lens->n_samples < 1u || lens->n_samples > RM_LENS_MAX_SAMPLES) {
        std::snprintf(buf, sizeof buf, "%s: lens.n_samples = %u is outside 1..64", who, lens->n_samples);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    if (!table) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL table");
    if (!frame) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL frame");
    return RM_OK;
}

// The host variant's check of the table's rows (dx, dy, u, v); a NaN fails the comparisons of its line
static rm_status check_lens_table(rm_ctx *ctx, const char *who, const double *t, uint32_t n) {
    for (uint32_t s = 0; s < n; s++) {
        const double dx = t[4u * s], dy = t[4u * s + 1u], u = t[4u * s + 2u], v = t[4u * s + 3u];
        const bool finite = std::isfinite(dx) && std::isfinite(dy) && std::isfinite(u) && std::isfinite(v);
        const bool offset = dx >= 0. && dx < 1. && dy >= 0. && dy < 1.;
        const bool disc = u * u + v * v <= 1. + 1e-12;
        if (!finite || !offset || !disc) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "%s: table row %u: (%g, %g, %g, %g): %s", who, s, dx, dy, u, v,
                          !finite ? "not finite" : !offset ? "the offset (dx, dy) is outside [0, 1) x [0, 1)" : "the lens point (u, v) is outside the unit disc");
            return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
        }
    }
    return RM_OK;
}

// Workgroups of the launch: what the device holds at once (CUs x the kernel's occupancy, asked once per kernel and context), at
// most what the frame needs, at most RM_LENS_MAX_BLOCKS where that is set.
static rm_status lens_grid(rm_ctx *ctx, const void *fn, uint32_t total, uint32_t n_samples, uint32_t *grid) {
    int per_cu = 0;
    for (const auto &e : ctx->lens_occupancy)
        if (e.first == fn) per_cu = e.second;
    if (per_cu == 0) {
        RM_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64, 0));
        per_cu = std::max(1, per_cu);
        ctx->lens_occupancy.emplace_back(fn, per_cu);
    }
    const uint32_t P = 64u / n_samples;
    const uint64_t need = ((uint64_t)total + P - 1u) / P;
    uint64_t g = std::min<uint64_t>(need, (uint64_t)std::max(1, ctx->prop.multiProcessorCount) * (uint64_t)per_cu);
    if (ctx->knobs.lens_max_blocks > 0u) g = std::min<uint64_t>(g, ctx->knobs.lens_max_blocks);
    *grid = (uint32_t)std::max<uint64_t>(g, 1u);
    return RM_OK;
}

// The argument block of a launch (rm_accum_host.inc's launches carry one too); everything was checked.
static LensArgs lens_args(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *table, void *frame) {
    LensArgs q{};
    q.H = ctx->image.H;
    q.H.off_occ = 0u;                                                      // (as launch_radiance)
    q.frame_width = p->frame_width;
    q.rows = refine_rows(p);
    q.n_samples = lens->n_samples;
    q.max_depth = p->max_depth;
    q.oriented = ctx->oriented ? 1u : 0u;
    q.aperture = lens->aperture;
    q.focus = lens->focus;
    q.bg_x = p->background.x; q.bg_y = p->background.y; q.bg_z = p->background.z;
    q.width = p->width; q.height = p->height; q.half_fov = p->half_fov; q.ratio = p->ratio;
    q.cam_x = ctx->camera.x; q.cam_y = ctx->camera.y; q.cam_z = ctx->camera.z;
    const rm_camera_basis fixed{{1., 0., 0.}, {0., 1., 0.}, {0., 0., -1.}};
    const rm_camera_basis &cb = ctx->oriented ? ctx->basis : fixed;
    q.cam_rx = cb.right.x; q.cam_ry = cb.right.y; q.cam_rz = cb.right.z;
    q.cam_ux = cb.up.x; q.cam_uy = cb.up.y; q.cam_uz = cb.up.z;
    q.cam_fx = cb.forward.x; q.cam_fy = cb.forward.y; q.cam_fz = cb.forward.z;
    q.table = static_cast<const double *>(table);
    q.frame = static_cast<double *>(frame);
    return q;
}

// The launch on `stream`; everything was checked, rows > 0.
static rm_status launch_lens(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *table, void *frame, hipStream_t stream) {
    LensArgs q = lens_args(ctx, p, lens, table, frame);
    const bool bvh = ctx->image.H.off_bvh_spheres != 0 || ctx->image.H.off_bvh_triangles != 0;   // (the radiance kernels' rules: launch_radiance)
    const int pow_mode = (ctx->image.integer_exponents && !ctx->knobs.force_generic_pow) ? POW_INTEGER : POW_GENERIC;
    const void *fn = rm_lens_kernel(bvh, pow_mode, q.max_depth <= 5u ? 4 : 32);
    if (!fn) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "lens: no such kernel");
    uint32_t grid = 0;
    if (rm_status gst = lens_grid(ctx, fn, q.rows * q.frame_width, q.n_samples, &grid)) return gst;
    void *args[] = {(void *)&ctx->d_scene, (void *)&q};
    RM_HIP(ctx, hipLaunchKernel(fn, dim3(grid), dim3(64), args, 0, stream));
    return RM_OK;
}

static rm_status rm_render_lens_device_impl(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *device_table, void *device_rgb,
                                            void *hip_stream) {
    const char *who = "rm_render_lens_device";
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
    if (rm_status cst = check_lens(ctx, who, p, lens, device_table, device_rgb)) return cst;
    if (refine_rows(p) == 0u) return RM_OK;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    return launch_lens(ctx, p, lens, device_table, device_rgb, (hipStream_t)hip_stream);   // NULL: HIP's default stream
}

static rm_status rm_render_lens_impl(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const double *table, double *host_rgb,
                                     rm_timing *timing) {
    const char *who = "rm_render_lens";
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
    const auto t_begin = std::chrono::steady_clock::now();
    if (rm_status cst = check_lens(ctx, who, p, lens, table, host_rgb)) return cst;
    if (rm_status tst = check_lens_table(ctx, who, table, lens->n_samples)) return tst;
    const uint32_t rows = refine_rows(p);
    double kernel_ms = 0., d2h_ms = 0.;
    if (rows > 0u) {
        RM_HIP(ctx, hipSetDevice(ctx->device));
        if (!ctx->d_lens_table) RM_HIP(ctx, hipMalloc(&ctx->d_lens_table, RM_LENS_MAX_SAMPLES * 4u * sizeof(double)));
        const size_t need = (size_t)rows * p->frame_width * 3u * sizeof(double);
        if (ctx->lens_frame_bytes < need) {
            if (ctx->d_lens_frame) RM_HIP(ctx, hipFree(ctx->d_lens_frame));
            ctx->d_lens_frame = nullptr;
            ctx->lens_frame_bytes = 0;
            RM_HIP(ctx, hipMalloc(&ctx->d_lens_frame, need));
            ctx->lens_frame_bytes = need;
        }
        RM_HIP(ctx, hipMemcpyAsync(ctx->d_lens_table, table, (size_t)lens->n_samples * 4u * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        RM_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        if (rm_status lst = launch_lens(ctx, p, lens, ctx->d_lens_table, ctx->d_lens_frame, ctx->stream)) return lst;
        RM_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const auto t0 = std::chrono::steady_clock::now();
        RM_HIP(ctx, hipMemcpy(host_rgb, ctx->d_lens_frame, need, hipMemcpyDeviceToHost));
        d2h_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        float ms = 0.f;
        RM_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        kernel_ms = ms;
    }
    if (timing) {
        timing->kernel_ms = kernel_ms;
        timing->d2h_ms = d2h_ms;
        timing->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    }
    return RM_OK;
}

extern "C" {

rm_status rm_lens_table(uint32_t n_samples, double *table) {
    if (n_samples < 1u || n_samples > RM_LENS_MAX_SAMPLES) {
        char buf[96];
        std::snprintf(buf, sizeof buf, "rm_lens_table: n_samples = %u is outside 1..64", n_samples);
        return ctx_fail(nullptr, RM_ERR_INVALID_ARG, buf);
    }
    if (!table) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_lens_table: NULL table");
    uint32_t m = 1u;                                                       // ceil(sqrt(n_samples)), in integers
    while (m * m < n_samples) m++;
    const double dm = (double)m;
    for (uint32_t s = 0; s < n_samples; s++) {
        const uint32_t i = s % m, j = s / m;
        const double a = (double)(2u * j + 1u) / dm - 1.;
        const double b = (double)(2u * (m - 1u - i) + 1u) / dm - 1.;
        double *r = table + 4u * (size_t)s;
        r[0] = (double)i / dm;
        r[1] = (double)j / dm;
        r[2] = a * std::sqrt(1. - b * b / 2.);
        r[3] = b * std::sqrt(1. - a * a / 2.);
    }
    return RM_OK;
}

rm_status rm_render_lens_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const void *device_table, void *device_rgb,
                                void *hip_stream) {
    return guarded(ctx, "rm_render_lens_device",
                   [&]() { return rm_render_lens_device_impl(ctx, params, lens, device_table, device_rgb, hip_stream); });
}

rm_status rm_render_lens(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const double *table, double *host_rgb, rm_timing *timing) {
    return guarded(ctx, "rm_render_lens", [&]() { return rm_render_lens_impl(ctx, params, lens, table, host_rgb, timing); });
}

}  // extern "C"
