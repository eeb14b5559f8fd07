// rm_refine_host.inc -- host side of the adaptive anti-aliasing (include/rusty_marcher_amd.h, "adaptive anti-aliasing");
// included at the end of rm_device.hip, behind rm_radiance_host.inc whose checks it shares.  The kernels are rm_refine.hip's.
//
// rm_refine_device touches no render state and keeps all of its own in the caller's workspace: a memset of the counter, the
// mark launch, the shade launch, all on the caller's stream, nothing waited for.  rm_render_antialiased is rm_render, that on
// the context's frame and stream with a workspace the context owns, and the copy.

static uint32_t refine_rows(const rm_params *p) { return p->frame_height - p->frame_height % RM_PATCH_SIZE; }

static size_t refine_workspace_bytes(const rm_params *p) {
    const size_t bytes = 4u * (1u + (size_t)refine_rows(p) * p->frame_width);
    return (bytes + 255u) & ~(size_t)255u;
}

// What both entry points check before anything is launched (ctx is not NULL).
static rm_status check_refine(rm_ctx *ctx, const char *who, const rm_params *p, const rm_refine *r) {
    if (rm_status pst = check_query_params(ctx, p, who)) return pst;
    if (p->frame_width % RM_PATCH_SIZE != 0)
        return ctx_fail(ctx, RM_ERR_DIMENSIONS, std::string(who) + ": frame width is not a multiple of 32 (no render writes such a frame)");
    if ((uint64_t)refine_rows(p) * p->frame_width > 0x7fffffffull)
        return ctx_fail(ctx, RM_ERR_DIMENSIONS, std::string(who) + ": more than 2^31 - 1 pixels");
    if (rm_status cst = check_shading(ctx, who, p->background, p->max_depth)) return cst;
    if (!r) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL refine");
    if (r->n < 1u || r->n > 8u) {
        char buf[128];
        std::snprintf(buf, sizeof buf, "%s: refine.n = %u is outside 1..8", who, r->n);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    if (std::isnan(r->threshold)) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": refine.threshold is NaN");
    return RM_OK;
}

// Workgroups of the shade launch: what the device holds at once (CUs x the kernel's occupancy), at most what a list of every
// pixel needs, at most RM_REFINE_MAX_BLOCKS where that is set.
static rm_status refine_grid(rm_ctx *ctx, const void *fn, uint32_t total, uint32_t n, uint32_t *grid) {
    int per_cu = 0;
    for (const auto &e : ctx->refine_occupancy)
        if (e.first == fn) per_cu = e.second;
    if (per_cu == 0) {
        RM_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64, 0));
        per_cu = std::max(1, per_cu);
        ctx->refine_occupancy.emplace_back(fn, per_cu);
    }
    const uint32_t P = 64u / (n * n);
    const uint64_t worst = ((uint64_t)total + P - 1u) / P;
    uint64_t g = std::min<uint64_t>(worst, (uint64_t)std::max(1, ctx->prop.multiProcessorCount) * (uint64_t)per_cu);
    if (ctx->knobs.refine_max_blocks > 0u) g = std::min<uint64_t>(g, ctx->knobs.refine_max_blocks);
    *grid = (uint32_t)std::max<uint64_t>(g, 1u);
    return RM_OK;
}

// The three steps on `stream`; everything was checked, rows > 0.
static rm_status launch_refine(rm_ctx *ctx, const rm_params *p, const rm_refine *r, void *frame, void *ws, void *mask, hipStream_t stream) {
    RefineArgs q{};
    q.H = ctx->image.H;
    q.H.off_occ = 0u;                                                      // (as launch_radiance)
    q.frame_width = p->frame_width;
    q.rows = refine_rows(p);
    q.n = r->n;
    q.max_depth = p->max_depth;
    q.oriented = ctx->oriented ? 1u : 0u;
    q.threshold = r->threshold;
    q.bg_x = p->background.x; q.bg_y = p->background.y; q.bg_z = p->background.z;
    q.width = p->width; q.height = p->height; q.half_fov = p->half_fov; q.ratio = p->ratio;
    q.cam_x = ctx->camera.x; q.cam_y = ctx->camera.y; q.cam_z = ctx->camera.z;
    const rm_camera_basis &cb = ctx->basis;
    q.cam_rx = cb.right.x; q.cam_ry = cb.right.y; q.cam_rz = cb.right.z;
    q.cam_ux = cb.up.x; q.cam_uy = cb.up.y; q.cam_uz = cb.up.z;
    q.cam_fx = cb.forward.x; q.cam_fy = cb.forward.y; q.cam_fz = cb.forward.z;
    q.frame = static_cast<double *>(frame);
    q.ws = static_cast<uint32_t *>(ws);
    q.mask = static_cast<uint8_t *>(mask);

    const bool bvh = ctx->image.H.off_bvh_spheres != 0 || ctx->image.H.off_bvh_triangles != 0;   // (the radiance kernels' rules: launch_radiance)
    const int pow_mode = (ctx->image.integer_exponents && !ctx->knobs.force_generic_pow) ? POW_INTEGER : POW_GENERIC;
    const void *shade = rm_refine_shade_kernel(bvh, pow_mode, q.max_depth <= 5u ? 4 : 32);
    if (!shade) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "refine: no such kernel");
    const uint32_t total = q.rows * q.frame_width;
    uint32_t grid = 0;
    if (rm_status gst = refine_grid(ctx, shade, total, q.n, &grid)) return gst;

    RM_HIP(ctx, hipMemsetAsync(ws, 0, sizeof(uint32_t), stream));
    void *mark_args[] = {(void *)&q};
    RM_HIP(ctx, hipLaunchKernel(rm_refine_mark_kernel(), dim3((total + RM_REFINE_MARK_LANES - 1u) / RM_REFINE_MARK_LANES),
                                dim3(RM_REFINE_MARK_LANES), mark_args, 0, stream));
    void *shade_args[] = {(void *)&ctx->d_scene, (void *)&q};
    RM_HIP(ctx, hipLaunchKernel(shade, dim3(grid), dim3(64), shade_args, 0, stream));
    return RM_OK;
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
        const size_t need = refine_workspace_bytes(p);
        if (ctx->refine_ws_bytes < need) {
            if (ctx->d_refine_ws) RM_HIP(ctx, hipFree(ctx->d_refine_ws));
            ctx->d_refine_ws = nullptr;
            ctx->refine_ws_bytes = 0;
            RM_HIP(ctx, hipMalloc(&ctx->d_refine_ws, need));
            ctx->refine_ws_bytes = need;
        }
        RM_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        if (rm_status lst = launch_refine(ctx, p, r, ctx->d_frame, ctx->d_refine_ws, nullptr, ctx->stream)) return lst;
        RM_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const auto t0 = std::chrono::steady_clock::now();
        RM_HIP(ctx, hipMemcpy(&count, ctx->d_refine_ws, sizeof count, hipMemcpyDeviceToHost));
        if (host_rgb)
            RM_HIP(ctx, hipMemcpy(host_rgb, ctx->d_frame, (size_t)rows * p->frame_width * 3u * sizeof(double), hipMemcpyDeviceToHost));
        d2h_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        float ms = 0.f;
        RM_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        refine_ms = ms;
    }
    if (n_refined) *n_refined = count;
    if (timing) {
        timing->kernel_ms = rendered.kernel_ms + refine_ms;
        timing->d2h_ms = d2h_ms;
        timing->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    }
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
