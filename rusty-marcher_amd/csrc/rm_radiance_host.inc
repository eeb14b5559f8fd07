// rm_radiance_host.inc -- host side of the radiance queries (include/rusty_marcher_amd.h, "radiance queries"); included at
// the end of rm_device.hip, behind rm_query_host.inc whose checks and staging buffer it shares and rm_shade_host.inc whose
// launch path.  The kernels are rm_radiance.hip's.
//
// Nothing here touches render state: the calls read the resident scene blob and -- the sample calls -- the context's camera
// and basis.  The sample rays are formed in the kernel, so the backproject tables are neither read nor rebuilt.

// One lane an answer (n > 0): the grid is the list's, no occupancy is asked
static rm_status launch_radiance(rm_ctx *ctx, RadianceArgs &q, hipStream_t stream) {
    q.H = shading_header(ctx);
    return launch_shading(ctx, shade_family{"radiance", rm_radiance_kernel}, q.max_depth, shade_extent{(uint32_t)((q.n + 63u) / 64u), 0u, 0u, 0u}, q,
                          stream);
}

static rm_status check_samples(rm_ctx *ctx, const char *who, const rm_params *p, const double *xy, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) {
        const double sx = xy[2u * (size_t)i], sy = xy[2u * (size_t)i + 1u];
        // (a NaN fails both comparisons of its line)
        if (!(sx >= 0. && sx < (double)p->frame_width) || !(sy >= 0. && sy < (double)p->frame_height)) {
            char buf[224];
            std::snprintf(buf, sizeof buf, "%s: sample %u: (%g, %g) outside [0, %u) x [0, %u)", who, i, sx, sy, p->frame_width, p->frame_height);
            return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
        }
    }
    return RM_OK;
}

static rm_status radiance_rays_impl(rm_ctx *ctx, const char *who, bool device, const void *origins, const void *directions, uint32_t n_rays,
                                    const rm_shading *shading, void *rgb, void *hip_stream) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
    if (!ctx->have_scene) return ctx_fail(ctx, RM_ERR_NO_SCENE, std::string(who) + ": no scene uploaded (rm_scene_upload)");
    if (n_rays == 0) return RM_OK;
    if (!shading) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL shading");
    if (rm_status cst = check_shading(ctx, who, shading->background, shading->max_depth)) return cst;
    if (!origins || !directions || !rgb) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + (device ? ": NULL device buffer" : ": NULL array"));
    RadianceArgs q{};
    q.n = n_rays;
    q.mode = RM_RADIANCE_RAYS;
    q.max_depth = shading->max_depth;
    q.bg_x = shading->background.x; q.bg_y = shading->background.y; q.bg_z = shading->background.z;
    if (device) {
        RM_HIP(ctx, hipSetDevice(ctx->device));
        q.origins = static_cast<const rm_vec3 *>(origins);
        q.directions = static_cast<const rm_vec3 *>(directions);
        q.rgb = static_cast<rm_vec3 *>(rgb);
        return launch_radiance(ctx, q, (hipStream_t)hip_stream);           // NULL: HIP's default stream, as rm_render_device
    }
    if (rm_status cst = check_rays(ctx, who, static_cast<const rm_vec3 *>(origins), static_cast<const rm_vec3 *>(directions), n_rays)) return cst;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    const size_t vb = (size_t)n_rays * sizeof(rm_vec3);
    char *buf = nullptr;
    if (rm_status sst = query_staging(ctx, 3u * vb, &buf)) return sst;
    RM_HIP(ctx, hipMemcpyAsync(buf, origins, vb, hipMemcpyHostToDevice, ctx->stream));
    RM_HIP(ctx, hipMemcpyAsync(buf + vb, directions, vb, hipMemcpyHostToDevice, ctx->stream));
    q.origins = reinterpret_cast<const rm_vec3 *>(buf);
    q.directions = reinterpret_cast<const rm_vec3 *>(buf + vb);
    q.rgb = reinterpret_cast<rm_vec3 *>(buf + 2u * vb);
    if (rm_status qst = launch_radiance(ctx, q, ctx->stream)) return qst;
    RM_HIP(ctx, hipMemcpyAsync(rgb, buf + 2u * vb, vb, hipMemcpyDeviceToHost, ctx->stream));
    RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RM_OK;
}

static rm_status radiance_samples_impl(rm_ctx *ctx, const char *who, bool device, const rm_params *p, const void *xy, uint32_t n, void *rgb,
                                       void *hip_stream) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
    if (rm_status pst = check_query_params(ctx, p, who)) return pst;
    if (n == 0) return RM_OK;
    if (rm_status cst = check_shading(ctx, who, p->background, p->max_depth)) return cst;
    if (!xy || !rgb) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + (device ? ": NULL device buffer" : ": NULL array"));
    RadianceArgs q{};
    q.n = n;
    q.mode = ctx->oriented ? RM_RADIANCE_SAMPLES_ORIENTED : RM_RADIANCE_SAMPLES;
    q.max_depth = p->max_depth;
    fill_view(q, ctx, p, ctx->basis);                                      // (the basis: read in the oriented mode only)
    if (device) {
        RM_HIP(ctx, hipSetDevice(ctx->device));
        q.xy = static_cast<const double *>(xy);
        q.rgb = static_cast<rm_vec3 *>(rgb);
        return launch_radiance(ctx, q, (hipStream_t)hip_stream);
    }
    if (rm_status cst = check_samples(ctx, who, p, static_cast<const double *>(xy), n)) return cst;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    const size_t in_bytes = (size_t)n * 2u * sizeof(double), out_bytes = (size_t)n * sizeof(rm_vec3);
    char *buf = nullptr;
    if (rm_status sst = query_staging(ctx, in_bytes + out_bytes, &buf)) return sst;
    RM_HIP(ctx, hipMemcpyAsync(buf, xy, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    q.xy = reinterpret_cast<const double *>(buf);
    q.rgb = reinterpret_cast<rm_vec3 *>(buf + in_bytes);
    if (rm_status qst = launch_radiance(ctx, q, ctx->stream)) return qst;
    RM_HIP(ctx, hipMemcpyAsync(rgb, buf + in_bytes, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RM_OK;
}

extern "C" {

rm_status rm_radiance_rays(rm_ctx *ctx, const rm_vec3 *origins, const rm_vec3 *directions, uint32_t n_rays, const rm_shading *shading,
                           rm_vec3 *rgb) {
    return guarded(ctx, "rm_radiance_rays",
                   [&]() { return radiance_rays_impl(ctx, "rm_radiance_rays", false, origins, directions, n_rays, shading, rgb, nullptr); });
}

rm_status rm_radiance_rays_device(rm_ctx *ctx, const void *device_origins, const void *device_directions, uint32_t n_rays,
                                  const rm_shading *shading, void *device_rgb, void *hip_stream) {
    return guarded(ctx, "rm_radiance_rays_device", [&]() {
        return radiance_rays_impl(ctx, "rm_radiance_rays_device", true, device_origins, device_directions, n_rays, shading, device_rgb, hip_stream);
    });
}

rm_status rm_radiance_samples(rm_ctx *ctx, const rm_params *params, const double *xy, uint32_t n, rm_vec3 *rgb) {
    return guarded(ctx, "rm_radiance_samples", [&]() { return radiance_samples_impl(ctx, "rm_radiance_samples", false, params, xy, n, rgb, nullptr); });
}

rm_status rm_radiance_samples_device(rm_ctx *ctx, const rm_params *params, const void *device_xy, uint32_t n, void *device_rgb,
                                     void *hip_stream) {
    return guarded(ctx, "rm_radiance_samples_device",
                   [&]() { return radiance_samples_impl(ctx, "rm_radiance_samples_device", true, params, device_xy, n, device_rgb, hip_stream); });
}

}  // extern "C"
