// rm_refine_host.inc -- host side of the adaptive anti-aliasing (include/rusty_marcher_amd.h, "adaptive anti-aliasing");
// included at the end of rm_device.hip, behind rm_shade_host.inc whose checks and launch path it shares.  The kernels are
// rm_refine.hip's.
//
// rm_refine_device touches no render state and keeps all of its own in the caller's workspace: a memset of the counter, the
// mark launch, the shade launch, all on the caller's stream, nothing waited for.  rm_render_antialiased is rm_render, that on
// the context's frame and stream with a workspace the context owns, and the copy.

static size_t refine_workspace_bytes(const rm_params *p) {
    const size_t bytes = 4u * (1u + (size_t)refine_rows(p) * p->frame_width);
    return (bytes + 255u) & ~(size_t)255u;
}

// What both entry points check before anything is launched (ctx is not NULL).
static rm_status check_refine(rm_ctx *ctx, const char *who, const rm_params *p, const rm_refine *r) {
    if (rm_status fst = check_sample_frame(ctx, who, p)) return fst;
    if (!r) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL refine");
    if (r->n < 1u || r->n > 8u) {
        char buf[128];
        std::snprintf(buf, sizeof buf, "%s: refine.n = %u is outside 1..8", who, r->n);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    if (std::isnan(r->threshold)) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": refine.threshold is NaN");
    return RM_OK;
}

// The three steps on `stream`; everything was checked, rows > 0.  The shade launch's grid is what a list of every pixel needs
// (the list's length is the device's alone), capped by RM_REFINE_MAX_BLOCKS.
static rm_status launch_refine(rm_ctx *ctx, const rm_params *p, const rm_refine *r, void *frame, void *ws, void *mask, hipStream_t stream) {
    RefineArgs q{};
    q.H = shading_header(ctx);
    q.frame_width = p->frame_width;
    q.rows = refine_rows(p);
    q.n = r->n;
    q.max_depth = p->max_depth;
    q.oriented = ctx->oriented ? 1u : 0u;
    q.threshold = r->threshold;
    fill_view(q, ctx, p, ctx->basis);
    q.frame = static_cast<double *>(frame);
    q.ws = static_cast<uint32_t *>(ws);
    q.mask = static_cast<uint8_t *>(mask);

    const uint32_t total = q.rows * q.frame_width;
    auto mark = [&]() -> rm_status {
        RM_HIP(ctx, hipMemsetAsync(ws, 0, sizeof(uint32_t), stream));
        void *mark_args[] = {(void *)&q};
        RM_HIP(ctx, hipLaunchKernel(rm_refine_mark_kernel(), dim3((total + RM_REFINE_MARK_LANES - 1u) / RM_REFINE_MARK_LANES),
                                    dim3(RM_REFINE_MARK_LANES), mark_args, 0, stream));
        return RM_OK;
    };
    return launch_shading(ctx, shade_family{"refine", rm_refine_shade_kernel}, q.max_depth,
                          shade_extent{0u, total, q.n * q.n, ctx->knobs.refine_max_blocks}, q, stream, mark);
}

static rm_status rm_refine_device_impl(rm_ctx *ctx, const rm_params *p, const rm_refine *r, void *device_rgb, void *device_workspace,
                                       void *device_mask, void *hip_stream) {
    const char *who = "rm_refine_device";
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
    if (rm_status cst = check_refine(ctx, who, p, r)) return cst;
    if (!device_rgb) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL frame (device_rgb)");
    if (!device_workspace) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL workspace (device_workspace)");
    if (refine_rows(p) == 0u) return RM_OK;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    return launch_refine(ctx, p, r, device_rgb, device_workspace, device_mask, (hipStream_t)hip_stream);   // NULL: HIP's default stream
}

static rm_status rm_render_antialiased_impl(rm_ctx *ctx, const rm_params *p, const rm_refine *r, double *host_rgb, uint32_t *n_refined,
                                            rm_timing *timing) {
    const char *who = "rm_render_antialiased";
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
    const auto t_begin = std::chrono::steady_clock::now();
    // (compact flags and a non-default band fail here as they do for every query: nothing is rendered)
    if (rm_status cst = check_refine(ctx, who, p, r)) return cst;
    rm_timing rendered{};
    if (rm_status rst = rm_render_impl(ctx, p, nullptr, &rendered)) return rst;   // into the resident frame, waited for
    const uint32_t rows = refine_rows(p);
    uint32_t count = 0;
    double refine_ms = 0., d2h_ms = 0.;
    if (rows > 0u) {
        if (rm_status gst = grow_device_buffer(ctx, &ctx->d_refine_ws, &ctx->refine_ws_bytes, refine_workspace_bytes(p))) return gst;
        if (rm_status lst = timed_launch(ctx, &refine_ms, [&]() { return launch_refine(ctx, p, r, ctx->d_frame, ctx->d_refine_ws, nullptr, ctx->stream); }))
            return lst;
        const auto t0 = std::chrono::steady_clock::now();
        RM_HIP(ctx, hipMemcpy(&count, ctx->d_refine_ws, sizeof count, hipMemcpyDeviceToHost));
        if (host_rgb)
            RM_HIP(ctx, hipMemcpy(host_rgb, ctx->d_frame, (size_t)rows * p->frame_width * 3u * sizeof(double), hipMemcpyDeviceToHost));
        d2h_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    if (n_refined) *n_refined = count;
    fill_timing(timing, rendered.kernel_ms + refine_ms, d2h_ms, t_begin);
    return RM_OK;
}

extern "C" {

rm_status rm_refine_workspace(const rm_params *params, size_t *bytes) {
    if (!params || !bytes) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_refine_workspace: NULL argument");
    if (params->frame_width % RM_PATCH_SIZE != 0)
        return ctx_fail(nullptr, RM_ERR_DIMENSIONS, "rm_refine_workspace: frame width is not a multiple of 32");
    *bytes = refine_workspace_bytes(params);
    return RM_OK;
}

rm_status rm_refine_device(rm_ctx *ctx, const rm_params *params, const rm_refine *refine, void *device_rgb, void *device_workspace,
                           void *device_mask, void *hip_stream) {
    return guarded(ctx, "rm_refine_device",
                   [&]() { return rm_refine_device_impl(ctx, params, refine, device_rgb, device_workspace, device_mask, hip_stream); });
}

rm_status rm_render_antialiased(rm_ctx *ctx, const rm_params *params, const rm_refine *refine, double *host_rgb, uint32_t *n_refined,
                                rm_timing *timing) {
    return guarded(ctx, "rm_render_antialiased",
                   [&]() { return rm_render_antialiased_impl(ctx, params, refine, host_rgb, n_refined, timing); });
}

}  // extern "C"
