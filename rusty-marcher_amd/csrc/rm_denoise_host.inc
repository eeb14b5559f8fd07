// rm_denoise_host.inc -- host side of the variance-guided filter (include/rusty_marcher_amd.h, "variance-guided filter");
// included at the end of rm_device.hip, behind rm_converge_motion_host.inc whose converging state (rm_converging) the tick
// reads, rm_query_host.inc whose pixel query (rm_primary_hits_device_impl) fills the tick's guide, and rm_shade_host.inc whose
// timed launch and tick tail (timed_launch, fill_timing).  The kernels are rm_denoise.hip's.
//
// rm_denoise_device touches no render state and keeps all of its own in the caller's buffers: the prepare launch and one
// launch an iteration on the caller's stream, nothing waited for.  rm_render_denoised is that on the context's stream over the
// converging frame's buffers, read only, into buffers the context owns for it (rm_ctx::denoising).

// Which path an iteration of step `step` takes (rm_denoise.hpp).  RM_DENOISE_TILED (A/B knob, read at every call) is the sum of
// the steps that stage their tile in LDS -- 0: none, every step gathers; 1: step 1; 2: step 2; 3: both --; unset: the choice the
// measurements made (profiles/denoise_figures.txt), RM_DENOISE_TILED_CHOSEN.
#define RM_DENOISE_TILED_CHOSEN 3u                                       // steps 1 and 2: each takes about 0.6 of the gather's time, guided or not
static int denoise_path(uint32_t step) {
    const char *e = std::getenv("RM_DENOISE_TILED");
    const uint32_t tiled = e && e[0] >= '0' && e[0] <= '3' && e[1] == '\0' ? (uint32_t)(e[0] - '0') : RM_DENOISE_TILED_CHOSEN;
    return step <= 2u && (tiled & step) != 0u ? 1 : 0;
}

// What the filter checks of rm_params: what the converging frames' device call does, but for the resident scene, the depth and
// the background, which it never looks at
static rm_status check_denoise_params(rm_ctx *ctx, const char *who, const rm_params *p) {
    if (!p) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL params");
    if (p->flags & ~RM_FLAG_FAST_FP)
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": params.flags may carry RM_FLAG_FAST_FP only (the filter is always strict)");
    if (p->patch_row_begin != 0u || p->patch_row_end != 0u || p->patch_row_stride > 1u)
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": the filter takes the default patch-row band only");
    if (p->patch_size != RM_PATCH_SIZE) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": patch_size must be 32 (renderer.rs:47)");
    if (p->frame_width == 0 || p->frame_height == 0) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": empty frame");
    if (p->frame_width % RM_PATCH_SIZE != 0)
        return ctx_fail(ctx, RM_ERR_DIMENSIONS, std::string(who) + ": frame width is not a multiple of 32 (no render writes such a frame)");
    if ((uint64_t)refine_rows(p) * p->frame_width > 0x7fffffffull)
        return ctx_fail(ctx, RM_ERR_DIMENSIONS, std::string(who) + ": more than 2^31 - 1 pixels");
    return RM_OK;
}

// The ranges of rm_denoise; a NaN fails the comparison of its line
static rm_status check_denoise(rm_ctx *ctx, const char *who, const rm_denoise *d) {
    if (!d) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL denoise");
    char buf[192];
    const struct { const char *name; double v; bool positive; } numbers[] = {
        {"sigma_l", d->sigma_l, false}, {"sigma_z", d->sigma_z, true}, {"epsilon", d->epsilon, true}, {"fallback_variance", d->fallback_variance, false}};
    for (const auto &n : numbers)
        if (!std::isfinite(n.v) || !(n.positive ? n.v > 0. : n.v >= 0.)) {
            std::snprintf(buf, sizeof buf, "%s: denoise.%s = %g is not a finite number %s 0", who, n.name, n.v, n.positive ? ">" : ">=");
            return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
        }
    if (d->iterations > RM_DENOISE_MAX_ITERATIONS) {
        std::snprintf(buf, sizeof buf, "%s: denoise.iterations = %u is outside 0..%u", who, d->iterations, RM_DENOISE_MAX_ITERATIONS);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    if (d->normal_squarings > RM_DENOISE_MAX_SQUARINGS) {
        std::snprintf(buf, sizeof buf, "%s: denoise.normal_squarings = %u is outside 0..%u", who, d->normal_squarings, RM_DENOISE_MAX_SQUARINGS);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    return RM_OK;
}

// The buffers of a call; hits, variance and rgb8 may be NULL
struct denoise_buffers {
    const void *sum, *stats, *count, *hits;
    void *workspace, *out, *variance, *rgb8;
};

static rm_status check_denoise_buffers(rm_ctx *ctx, const char *who, const denoise_buffers &b) {
    const struct { const char *name; const void *p; } required[] = {
        {"sum", b.sum}, {"stats", b.stats}, {"count", b.count}, {"workspace", b.workspace}, {"out", b.out}};
    for (const auto &r : required)
        if (!r.p) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL " + r.name);
    const struct { const char *name; const void *p; } inputs[] = {{"sum", b.sum}, {"stats", b.stats}, {"count", b.count}, {"hits", b.hits}};
    for (const auto &i : inputs)
        if (b.out == i.p)
            return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": the output would overwrite an input (device_out == device_" + i.name + ")");
    return RM_OK;
}

// The launches on `stream`; everything was checked, rows > 0
static rm_status launch_denoise(rm_ctx *ctx, const rm_params *p, const rm_denoise *d, const denoise_buffers &b, hipStream_t stream) {
    DenoiseArgs a{};
    a.frame_width = p->frame_width;
    a.rows = refine_rows(p);
    a.squarings = d->normal_squarings;
    a.sigma_l = d->sigma_l; a.sigma_z = d->sigma_z; a.epsilon = d->epsilon; a.fallback_variance = d->fallback_variance;
    a.sum = static_cast<const double *>(b.sum);
    a.stats = static_cast<const double *>(b.stats);
    a.count = static_cast<const uint32_t *>(b.count);
    a.hits = static_cast<const double *>(b.hits);
    a.out = static_cast<double *>(b.out);
    a.variance = static_cast<double *>(b.variance);
    a.rgb8 = static_cast<uint8_t *>(b.rgb8);
    const size_t pixels = (size_t)a.rows * a.frame_width;
    double *plane[2] = {static_cast<double *>(b.workspace), static_cast<double *>(b.workspace) + pixels * RM_DENOISE_PLANE_WORDS};
    a.guide = plane[1] + pixels * RM_DENOISE_PLANE_WORDS;
    a.dst = plane[0];
    a.last = d->iterations == 0u ? 1u : 0u;
    void *args[] = {(void *)&a};
    RM_HIP(ctx, hipLaunchKernel(rm_denoise_prepare_kernel(), dim3((uint32_t)((pixels + RM_DENOISE_PREPARE_LANES - 1u) / RM_DENOISE_PREPARE_LANES)),
                                dim3(RM_DENOISE_PREPARE_LANES), args, 0, stream));
    const dim3 grid(a.frame_width / RM_DENOISE_TILE_W, a.rows / RM_DENOISE_TILE_H), block(RM_DENOISE_TILE_W * RM_DENOISE_TILE_H);
    for (uint32_t i = 0; i < d->iterations; i++) {
        a.step = 1u << i;
        a.src = plane[i & 1u];
        a.dst = plane[(i + 1u) & 1u];
        a.last = i + 1u == d->iterations ? 1u : 0u;
        const void *fn = rm_denoise_iteration_kernel(b.hits != nullptr, denoise_path(a.step), a.step);
        if (!fn) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "denoise: no such kernel");
        RM_HIP(ctx, hipLaunchKernel(fn, grid, block, args, 0, stream));
    }
    return RM_OK;
}

// The filter's state of a context (rm_ctx::denoising; made by the first rm_render_denoised, released by rm_destroy)
struct rm_denoising {
    void *d_ws = nullptr, *d_hits = nullptr, *d_out = nullptr, *d_rgb8 = nullptr;
    size_t ws_bytes = 0, hits_bytes = 0, out_bytes = 0, rgb8_bytes = 0;
};

static void denoising_destroy(rm_ctx *ctx, bool device_ok) {
    rm_denoising *g = ctx->denoising;
    if (!g) return;
    for (void *b : {g->d_ws, g->d_hits, g->d_out, g->d_rgb8})
        if (b && device_ok) (void)hipFree(b);
    delete g;
    ctx->denoising = nullptr;
}

static rm_status rm_render_denoised_impl(rm_ctx *ctx, const rm_params *p, const rm_denoise *d, int guides, double *host_rgb, uint8_t *host_rgb8,
                                         rm_timing *timing) {
    const char *who = "rm_render_denoised";
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
    const auto t_begin = std::chrono::steady_clock::now();
    if (rm_status pst = check_denoise_params(ctx, who, p)) return pst;
    if (rm_status dst = check_denoise(ctx, who, d)) return dst;
    const rm_converging *c = ctx->converging;
    if (!c || !c->have_key) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": no converging frame (rm_render_converging* has not run)");
    if (c->id.key.frame_width != p->frame_width || c->id.key.frame_height != p->frame_height) {
        char buf[192];
        std::snprintf(buf, sizeof buf, "%s: the converging frame is %u x %u, params say %u x %u", who, c->id.key.frame_width, c->id.key.frame_height,
                      p->frame_width, p->frame_height);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    const uint32_t rows = refine_rows(p);
    const size_t pixels = (size_t)rows * p->frame_width;
    double kernel_ms = 0.;
    if (rows > 0u) {
        RM_HIP(ctx, hipSetDevice(ctx->device));
        if (!ctx->denoising) ctx->denoising = new rm_denoising();
        rm_denoising &g = *ctx->denoising;
        if (rm_status gst = grow_device_buffer(ctx, &g.d_ws, &g.ws_bytes, rm_denoise_workspace_bytes(pixels))) return gst;
        if (rm_status gst = grow_device_buffer(ctx, &g.d_out, &g.out_bytes, pixels * 3u * sizeof(double))) return gst;
        if (rm_status gst = grow_device_buffer(ctx, &g.d_rgb8, &g.rgb8_bytes, pixels * 3u)) return gst;
        if (guides)
            if (rm_status gst = grow_device_buffer(ctx, &g.d_hits, &g.hits_bytes, (size_t)p->frame_height * p->frame_width * sizeof(rm_hit))) return gst;
        const denoise_buffers b{c->d_sum, c->d_stats, c->d_count, guides ? g.d_hits : nullptr, g.d_ws, g.d_out, nullptr, g.d_rgb8};
        auto launch = [&]() -> rm_status {
            if (guides)
                if (rm_status hst = rm_primary_hits_device_impl(ctx, p, g.d_hits, ctx->stream)) return hst;
            return launch_denoise(ctx, p, d, b, ctx->stream);
        };
        if (rm_status lst = timed_launch(ctx, &kernel_ms, launch)) return lst;
    }
    const rm_denoising *g = rows > 0u ? ctx->denoising : nullptr;
    return finish_tick(ctx, pixels, g ? g->d_out : nullptr, g ? g->d_rgb8 : nullptr, host_rgb, host_rgb8, kernel_ms, timing, t_begin);
}

extern "C" {

rm_status rm_denoise_workspace(const rm_params *params, size_t *bytes) {
    if (!params || !bytes) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_denoise_workspace: NULL argument");
    if (params->frame_width % RM_PATCH_SIZE != 0)
        return ctx_fail(nullptr, RM_ERR_DIMENSIONS, "rm_denoise_workspace: frame width is not a multiple of 32");
    *bytes = rm_denoise_workspace_bytes((size_t)refine_rows(params) * params->frame_width);
    return RM_OK;
}

rm_status rm_denoise_device(rm_ctx *ctx, const rm_params *p, const rm_denoise *d, const void *device_sum, const void *device_stats,
                            const void *device_count, const void *device_hits, void *device_workspace, void *device_out, void *device_variance,
                            void *device_rgb8, void *hip_stream) {
    const char *who = "rm_denoise_device";
    return guarded(ctx, who, [&]() -> rm_status {
        if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
        if (rm_status pst = check_denoise_params(ctx, who, p)) return pst;
        if (rm_status dst = check_denoise(ctx, who, d)) return dst;
        const denoise_buffers b{device_sum, device_stats, device_count, device_hits, device_workspace, device_out, device_variance, device_rgb8};
        if (rm_status bst = check_denoise_buffers(ctx, who, b)) return bst;
        if (refine_rows(p) == 0u) return RM_OK;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        return launch_denoise(ctx, p, d, b, (hipStream_t)hip_stream);
    });
}

rm_status rm_render_denoised(rm_ctx *ctx, const rm_params *params, const rm_denoise *denoise, int guides, double *host_rgb, uint8_t *host_rgb8,
                             rm_timing *timing) {
    return guarded(ctx, "rm_render_denoised", [&]() { return rm_render_denoised_impl(ctx, params, denoise, guides, host_rgb, host_rgb8, timing); });
}

}  // extern "C"
