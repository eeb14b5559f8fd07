// rm_shade_host.inc -- what the host sides of the shading kernels share: the radiance queries (rm_radiance_host.inc), adaptive
// anti-aliasing (rm_refine_host.inc), the thin-lens camera (rm_lens_host.inc), progressive frames (rm_accum_host.inc), area
// lights (rm_soft_host.inc), moving spheres (rm_motion_host.inc), converging frames (rm_converge_host.inc) and converging frames with
// moving spheres (rm_converge_motion_host.inc).  Included at the end of rm_device.hip in front of them,
// behind rm_query_host.inc whose check of the params it uses.
//
// One launch path (launch_shading): the variant and the grid are rm_plan.cpp's arithmetic (rm_shading_variant_of,
// rm_shading_grid), the kernel is the family's picker's, the occupancy is asked here and nowhere else.  A family's launcher fills
// its argument block and calls it.  Beside it the checks every sampled frame passes, the view fields every argument block
// carries, the timed launch of the calls that own their buffers, and what the two ticks (rm_motion_host.inc,
// rm_converge_motion_host.inc) do alike around theirs: grow their output buffers, copy mean and bytes back.

// The rows a render writes, and so a sampled frame covers (renderer.rs:53: the bottom frame_height % 32 rows are never rendered)
static uint32_t refine_rows(const rm_params *p) { return p->frame_height - p->frame_height % RM_PATCH_SIZE; }

// max_depth and background of a call: what a host can get wrong without touching an element
static rm_status check_shading(rm_ctx *ctx, const char *who, const rm_vec3 &bg, uint32_t max_depth) {
    if (max_depth > RM_MAX_DEPTH) return ctx_fail(ctx, RM_ERR_DEPTH, std::string(who) + ": max_depth above RM_MAX_DEPTH");
    if (!finite3(bg)) {
        char buf[192];
        std::snprintf(buf, sizeof buf, "%s: background (%g, %g, %g) is not finite", who, bg.x, bg.y, bg.z);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    return RM_OK;
}

// What every call that samples a frame's pixels checks of its params first (ctx is not NULL)
static rm_status check_sample_frame(rm_ctx *ctx, const char *who, const rm_params *p) {
    if (rm_status pst = check_query_params(ctx, p, who)) return pst;
    if (p->frame_width % RM_PATCH_SIZE != 0)
        return ctx_fail(ctx, RM_ERR_DIMENSIONS, std::string(who) + ": frame width is not a multiple of 32 (no render writes such a frame)");
    if ((uint64_t)refine_rows(p) * p->frame_width > 0x7fffffffull)
        return ctx_fail(ctx, RM_ERR_DIMENSIONS, std::string(who) + ": more than 2^31 - 1 pixels");
    return check_shading(ctx, who, p->background, p->max_depth);
}

// The header the shading kernels walk the resident scene by: the occluder masks hold near the scene only, never for rays of a
// caller's making (rm_radiance.hip), so it says there are none
static rm_dev_header shading_header(const rm_ctx *ctx) {
    rm_dev_header H = ctx->image.H;
    H.off_occ = 0u;
    return H;
}

// The view fields of an argument block (RadianceArgs, RefineArgs, LensArgs): the params' background and Renderer, the context's
// camera and the basis `cb` -- the caller's choice, since a kernel may read it in the fixed view too
template <class ARGS>
static void fill_view(ARGS &q, const rm_ctx *ctx, const rm_params *p, const rm_camera_basis &cb) {
    q.bg_x = p->background.x; q.bg_y = p->background.y; q.bg_z = p->background.z;
    q.width = p->width; q.height = p->height; q.half_fov = p->half_fov; q.ratio = p->ratio;
    q.cam_x = ctx->camera.x; q.cam_y = ctx->camera.y; q.cam_z = ctx->camera.z;
    q.cam_rx = cb.right.x; q.cam_ry = cb.right.y; q.cam_rz = cb.right.z;
    q.cam_ux = cb.up.x; q.cam_uy = cb.up.y; q.cam_uz = cb.up.z;
    q.cam_fx = cb.forward.x; q.cam_fy = cb.forward.y; q.cam_fz = cb.forward.z;
}

// A family of shading kernels: its name in "<name>: no such kernel", and its table of instantiations
struct shade_family {
    const char *name;
    const void *(*pick)(bool bvh, int pow_mode, int stack);
    const double *scene = nullptr;   // the blob its kernels are handed; NULL: the resident one (a swept one: rm_swept_host.inc)
};

// The workgroups of a shading launch: `blocks` where that is not 0 (the radiance queries: a lane an answer), else what
// rm_shading_grid makes of `total` pixels with `rays_per_pixel` rays each, the kernel's occupancy and the cap `max_blocks`
struct shade_extent {
    uint32_t blocks;
    uint32_t total, rays_per_pixel, max_blocks;
};

// The launch of family `f` with the depth cap `max_depth` on `stream`, arguments: the scene blob and `a`.  `before` runs once
// the kernel and the grid are known and nothing has failed, in front of the launch: the steps that make the list a kernel shades.
template <class ARGS, class BEFORE>
static rm_status launch_shading(rm_ctx *ctx, const shade_family &f, uint32_t max_depth, const shade_extent &x, ARGS &a, hipStream_t stream,
                                BEFORE before) {
    const rm_shading_variant v = rm_shading_variant_of(ctx->knobs, ctx->image.H, ctx->image.integer_exponents, max_depth);
    const void *fn = f.pick(v.bvh, v.pow_mode, v.stack);
    if (!fn) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(f.name) + ": no such kernel");
    uint32_t grid = x.blocks;
    if (grid == 0u) {
        int per_cu = 0;
        for (const auto &e : ctx->shade_occupancy)
            if (e.first == fn) per_cu = e.second;
        if (per_cu == 0) {
            RM_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64, 0));
            per_cu = std::max(1, per_cu);
            ctx->shade_occupancy.emplace_back(fn, per_cu);
        }
        grid = rm_shading_grid(x.total, x.rays_per_pixel, ctx->prop.multiProcessorCount, per_cu, x.max_blocks);
    }
    if (rm_status bst = before()) return bst;
    const double *scene = f.scene ? f.scene : ctx->d_scene;
    void *args[] = {(void *)&scene, (void *)&a};
    RM_HIP(ctx, hipLaunchKernel(fn, dim3(grid), dim3(64), args, 0, stream));
    return RM_OK;
}

template <class ARGS>
static rm_status launch_shading(rm_ctx *ctx, const shade_family &f, uint32_t max_depth, const shade_extent &x, ARGS &a, hipStream_t stream) {
    return launch_shading(ctx, f, max_depth, x, a, stream, []() -> rm_status { return RM_OK; });
}

// `launch` on the context's stream between the context's two events, waited for; *ms: the time between them
template <class LAUNCH>
static rm_status timed_launch(rm_ctx *ctx, double *ms, LAUNCH launch) {
    RM_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    if (rm_status lst = launch()) return lst;
    RM_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float elapsed = 0.f;
    RM_HIP(ctx, hipEventElapsedTime(&elapsed, ctx->ev0, ctx->ev1));
    *ms = elapsed;
    return RM_OK;
}

// ... and what such a call reports: total_ms runs from t_begin to now
static void fill_timing(rm_timing *timing, double kernel_ms, double d2h_ms, std::chrono::steady_clock::time_point t_begin) {
    if (!timing) return;
    timing->kernel_ms = kernel_ms;
    timing->d2h_ms = d2h_ms;
    timing->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
}

// Makes the output buffers a tick owns hold `pixels` pixels (*have: what they have room for).  They share one shape, so where
// one is too small every one is replaced; a failed allocation leaves *have 0.
static rm_status grow_frame_buffers(rm_ctx *ctx, size_t *have, size_t pixels, std::initializer_list<std::pair<void **, size_t>> buffers) {
    if (*have >= pixels) return RM_OK;
    *have = 0;
    for (const auto &b : buffers) {
        size_t none = 0;
        if (rm_status gst = grow_device_buffer(ctx, b.first, &none, b.second)) return gst;
    }
    *have = pixels;
    return RM_OK;
}

// The tail of a tick: mean and display bytes of `pixels` pixels (0: a frame without a whole patch row, nothing to copy) back to
// the host where asked, timed, and the timing filled in
static rm_status finish_tick(rm_ctx *ctx, size_t pixels, const void *d_mean, const void *d_rgb8, double *host_rgb, uint8_t *host_rgb8,
                             double kernel_ms, rm_timing *timing, std::chrono::steady_clock::time_point t_begin) {
    double d2h_ms = 0.;
    if (pixels > 0u) {
        const auto t0 = std::chrono::steady_clock::now();
        if (host_rgb) RM_HIP(ctx, hipMemcpy(host_rgb, d_mean, pixels * 3u * sizeof(double), hipMemcpyDeviceToHost));
        if (host_rgb8) RM_HIP(ctx, hipMemcpy(host_rgb8, d_rgb8, pixels * 3u, hipMemcpyDeviceToHost));
        d2h_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    fill_timing(timing, kernel_ms, d2h_ms, t_begin);
    return RM_OK;
}
