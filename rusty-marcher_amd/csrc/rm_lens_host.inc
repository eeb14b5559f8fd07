// rm_lens_host.inc -- host side of the thin-lens camera (include/rusty_marcher_amd.h, "thin-lens camera"); included at the end
// of rm_device.hip, behind rm_shade_host.inc whose checks and launch path it shares.  The kernel is rm_lens.hip's.
//
// rm_render_lens_device touches no render state and keeps none of its own: one launch on the caller's stream, nothing waited
// for.  rm_render_lens is that on the context's stream with a table buffer and a frame buffer the context owns, and the copy;
// the resident frame of rm_render is not used.

#define RM_LENS_MAX_SAMPLES 64u

// What both entry points check before anything is launched (ctx is not NULL).
static rm_status check_lens(rm_ctx *ctx, const char *who, const rm_params *p, const rm_lens *lens, const void *table, const void *frame) {
    if (rm_status fst = check_sample_frame(ctx, who, p)) return fst;
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

// The argument block of a launch (the progressive, soft and converging launches carry one too); everything was checked.
static LensArgs lens_args(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *table, void *frame) {
    LensArgs q{};
    q.H = shading_header(ctx);
    q.frame_width = p->frame_width;
    q.rows = refine_rows(p);
    q.n_samples = lens->n_samples;
    q.max_depth = p->max_depth;
    q.oriented = ctx->oriented ? 1u : 0u;
    q.aperture = lens->aperture;
    q.focus = lens->focus;
    const rm_camera_basis fixed{{1., 0., 0.}, {0., 1., 0.}, {0., 0., -1.}};
    fill_view(q, ctx, p, ctx->oriented ? ctx->basis : fixed);               // (the lens point is formed from the basis in either view)
    q.table = static_cast<const double *>(table);
    q.frame = static_cast<double *>(frame);
    return q;
}

// The workgroups of a launch over the pixels of `q`, n_samples rays each: what the frame needs, capped by RM_LENS_MAX_BLOCKS
static shade_extent lens_extent(const rm_ctx *ctx, const LensArgs &q) {
    return shade_extent{0u, q.rows * q.frame_width, q.n_samples, ctx->knobs.lens_max_blocks};
}

// The launch on `stream`; everything was checked, rows > 0.
static rm_status launch_lens(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *table, void *frame, hipStream_t stream) {
    LensArgs q = lens_args(ctx, p, lens, table, frame);
    return launch_shading(ctx, shade_family{"lens", rm_lens_kernel}, q.max_depth, lens_extent(ctx, q), q, stream);
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
        if (rm_status gst = grow_device_buffer(ctx, &ctx->d_lens_frame, &ctx->lens_frame_bytes, need)) return gst;
        RM_HIP(ctx, hipMemcpyAsync(ctx->d_lens_table, table, (size_t)lens->n_samples * 4u * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        if (rm_status lst = timed_launch(ctx, &kernel_ms, [&]() { return launch_lens(ctx, p, lens, ctx->d_lens_table, ctx->d_lens_frame, ctx->stream); }))
            return lst;
        const auto t0 = std::chrono::steady_clock::now();
        RM_HIP(ctx, hipMemcpy(host_rgb, ctx->d_lens_frame, need, hipMemcpyDeviceToHost));
        d2h_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    fill_timing(timing, kernel_ms, d2h_ms, t_begin);
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
