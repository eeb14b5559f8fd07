// rm_query_host.inc -- host side of the ray queries (include/rusty_marcher_amd.h, "ray queries"); included at the end of
// rm_device.hip.  The kernels are rm_query.hip's.
//
// Nothing here touches render state: the queries read the resident scene blob, the pid map the upload builds next to it
// (rm_ctx::d_pid_map) and -- the pixel queries -- the backproject tables of the render (rebuilt for another frame geometry
// exactly as a render would: the next render at its own geometry rebuilds them again, with the same values).  The host
// variants stage their rays and answers in a buffer of their own on the context's stream.

// What the queries accept of rm_params: the default band, no flag but RM_FLAG_FAST_FP (which they ignore: the queries
// are the strict flavour).
static rm_status check_query_params(rm_ctx *ctx, const rm_params *p, const char *who) {
    if (!p) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL params");
    if (!ctx->have_scene) return ctx_fail(ctx, RM_ERR_NO_SCENE, std::string(who) + ": no scene uploaded (rm_scene_upload)");
    if (p->flags & ~RM_FLAG_FAST_FP)
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": params.flags may carry RM_FLAG_FAST_FP only (queries are always strict)");
    if (p->patch_row_begin != 0u || p->patch_row_end != 0u || p->patch_row_stride > 1u)
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": queries take the default patch-row band only");
    if (p->patch_size != RM_PATCH_SIZE) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": patch_size must be 32 (renderer.rs:47)");
    if (p->frame_width == 0 || p->frame_height == 0) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": empty frame");
    return RM_OK;
}

// The host variants' check of the reference's assert (sphere.rs:31, polygon.rs:62, triangle.rs:53): |d.d - 1| < 1e-4, with
// d.d = (x x + y y) + z z as geometry.rs:180-182 forms it; every component of origin and direction finite.
static rm_status check_rays(rm_ctx *ctx, const char *who, const rm_vec3 *o, const rm_vec3 *d, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) {
        const bool finite = std::isfinite(o[i].x) && std::isfinite(o[i].y) && std::isfinite(o[i].z) && std::isfinite(d[i].x) &&
                            std::isfinite(d[i].y) && std::isfinite(d[i].z);
        const double nn = d[i].x * d[i].x + d[i].y * d[i].y + d[i].z * d[i].z;
        if (!finite || !(std::fabs(nn - 1.) < 1e-4)) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "%s: ray %u: origin (%g, %g, %g), direction (%g, %g, %g): %s", who, i, o[i].x, o[i].y, o[i].z,
                          d[i].x, d[i].y, d[i].z, finite ? "direction is not of unit length (|d.d - 1| >= 1e-4)" : "not finite");
            return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
        }
    }
    return RM_OK;
}

static rm_status launch_query(rm_ctx *ctx, int kind, QueryArgs &q, uint32_t blocks, hipStream_t stream) {
    q.H = ctx->image.H;
    q.pid_map = ctx->d_pid_map;
    const bool bvh = ctx->image.H.off_bvh_spheres != 0 || ctx->image.H.off_bvh_triangles != 0;   // (as launch_render picks its kernels)
    const void *fn = rm_query_kernel(kind, bvh, kind == RM_QUERY_PIXELS && ctx->oriented);
    if (!fn) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "query: no such kernel");
    void *args[] = {(void *)&ctx->d_scene, (void *)&q};
    RM_HIP(ctx, hipLaunchKernel(fn, dim3(blocks), dim3(64), args, 0, stream));
    return RM_OK;
}

static uint32_t ray_blocks(uint32_t n_rays) { return (uint32_t)(((uint64_t)n_rays + 63u) / 64u); }

// The ray-list queries on device buffers, on `stream`.
static rm_status query_rays(rm_ctx *ctx, bool occlusion, const void *origins, const void *directions, uint32_t n_rays, void *out,
                            hipStream_t stream) {
    QueryArgs q{};
    q.origins = static_cast<const rm_vec3 *>(origins);
    q.directions = static_cast<const rm_vec3 *>(directions);
    q.n_rays = n_rays;
    if (occlusion) q.occluded = static_cast<uint8_t *>(out);
    else q.hits = static_cast<rm_hit *>(out);
    return launch_query(ctx, occlusion ? RM_QUERY_OCCLUDED : RM_QUERY_CLOSEST, q, ray_blocks(n_rays), stream);
}

// The host variants' staging buffer: rays in, answers out (grown as needed; only synchronous calls use it).
static rm_status query_staging(rm_ctx *ctx, size_t bytes, char **out) {
    if (rm_status gst = grow_device_buffer(ctx, &ctx->d_query, &ctx->query_bytes, bytes)) return gst;
    *out = static_cast<char *>(ctx->d_query);
    return RM_OK;
}

static rm_status rays_host_impl(rm_ctx *ctx, const char *who, bool occlusion, const rm_vec3 *origins, const rm_vec3 *directions,
                                uint32_t n_rays, void *out) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
    if (!ctx->have_scene) return ctx_fail(ctx, RM_ERR_NO_SCENE, std::string(who) + ": no scene uploaded (rm_scene_upload)");
    if (n_rays == 0) return RM_OK;
    if (!origins || !directions || !out) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL array");
    if (rm_status cst = check_rays(ctx, who, origins, directions, n_rays)) return cst;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ray_bytes = (size_t)n_rays * sizeof(rm_vec3);
    const size_t out_bytes = (size_t)n_rays * (occlusion ? sizeof(uint8_t) : sizeof(rm_hit));
    char *buf = nullptr;
    if (rm_status sst = query_staging(ctx, 2u * ray_bytes + out_bytes, &buf)) return sst;
    RM_HIP(ctx, hipMemcpyAsync(buf, origins, ray_bytes, hipMemcpyHostToDevice, ctx->stream));
    RM_HIP(ctx, hipMemcpyAsync(buf + ray_bytes, directions, ray_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (rm_status qst = query_rays(ctx, occlusion, buf, buf + ray_bytes, n_rays, buf + 2u * ray_bytes, ctx->stream)) return qst;
    RM_HIP(ctx, hipMemcpyAsync(out, buf + 2u * ray_bytes, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RM_OK;
}

static rm_status rays_device_impl(rm_ctx *ctx, const char *who, bool occlusion, const void *origins, const void *directions,
                                  uint32_t n_rays, void *out, void *hip_stream) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
    if (!ctx->have_scene) return ctx_fail(ctx, RM_ERR_NO_SCENE, std::string(who) + ": no scene uploaded (rm_scene_upload)");
    if (n_rays == 0) return RM_OK;
    if (!origins || !directions || !out) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL device buffer");
    RM_HIP(ctx, hipSetDevice(ctx->device));
    return query_rays(ctx, occlusion, origins, directions, n_rays, out, (hipStream_t)hip_stream);   // NULL: HIP's default stream, as rm_render_device
}

// The pixel queries: one pixel (n_tiles == 0) or the tiles of the whole patch rows.
static rm_status query_pixels(rm_ctx *ctx, const rm_params *p, uint32_t x, uint32_t y, uint32_t n_tiles, rm_hit *out,
                              hipStream_t stream) {
    if (rm_status bst = backproject_tables(ctx, p)) return bst;
    QueryArgs q{};
    q.frame_width = p->frame_width;
    q.tiles_per_row = p->frame_width / TILE_W;
    q.n_tiles = n_tiles;
    q.pick_x = x;
    q.pick_y = y;
    q.bp_x = ctx->d_backproject;
    q.bp_y = ctx->d_backproject + p->frame_width;
    q.cam_x = ctx->camera.x; q.cam_y = ctx->camera.y; q.cam_z = ctx->camera.z;
    const rm_camera_basis &cb = ctx->basis;                          // (read by the oriented kernel only)
    q.cam_rx = cb.right.x; q.cam_ry = cb.right.y; q.cam_rz = cb.right.z;
    q.cam_ux = cb.up.x; q.cam_uy = cb.up.y; q.cam_uz = cb.up.z;
    q.cam_fx = cb.forward.x; q.cam_fy = cb.forward.y; q.cam_fz = cb.forward.z;
    q.hits = out;
    return launch_query(ctx, RM_QUERY_PIXELS, q, n_tiles ? n_tiles : 1u, stream);
}

static rm_status rm_pick_impl(rm_ctx *ctx, const rm_params *params, uint32_t x, uint32_t y, rm_hit *hit) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_pick: NULL ctx");
    if (rm_status pst = check_query_params(ctx, params, "rm_pick")) return pst;
    if (!hit) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "rm_pick: NULL hit");
    if (x >= params->frame_width || y >= params->frame_height) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "rm_pick: pixel (%u, %u) outside the %u x %u frame", x, y, params->frame_width, params->frame_height);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    RM_HIP(ctx, hipSetDevice(ctx->device));
    char *buf = nullptr;
    if (rm_status sst = query_staging(ctx, sizeof(rm_hit), &buf)) return sst;
    if (rm_status qst = query_pixels(ctx, params, x, y, 0u, reinterpret_cast<rm_hit *>(buf), ctx->stream)) return qst;
    RM_HIP(ctx, hipMemcpyAsync(hit, buf, sizeof(rm_hit), hipMemcpyDeviceToHost, ctx->stream));
    RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RM_OK;
}

static rm_status rm_primary_hits_device_impl(rm_ctx *ctx, const rm_params *params, void *device_hits, void *hip_stream) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_primary_hits_device: NULL ctx");
    if (rm_status pst = check_query_params(ctx, params, "rm_primary_hits_device")) return pst;
    if (params->frame_width % RM_PATCH_SIZE != 0)
        return ctx_fail(ctx, RM_ERR_DIMENSIONS,
                        "rm_primary_hits_device: frame width is not a multiple of 32; the reference's scatter "
                        "(renderer.rs:92-108) indexes out of bounds and panics");
    if (!device_hits) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "rm_primary_hits_device: NULL device buffer");
    const uint32_t n_rows = params->frame_height / RM_PATCH_SIZE;     // renderer.rs:53: the bottom H % 32 rows are not rendered
    if (n_rows == 0) return RM_OK;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n_tiles = (uint64_t)(params->frame_width / TILE_W) * (n_rows * RM_PATCH_SIZE / TILE_H);
    if (n_tiles > 0x7FFFFFFFull) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "rm_primary_hits_device: frame too large for one launch");
    return query_pixels(ctx, params, 0u, 0u, (uint32_t)n_tiles, static_cast<rm_hit *>(device_hits), (hipStream_t)hip_stream);
}

extern "C" {

rm_status rm_intersect_rays(rm_ctx *ctx, const rm_vec3 *origins, const rm_vec3 *directions, uint32_t n_rays, rm_hit *hits) {
    return guarded(ctx, "rm_intersect_rays", [&]() { return rays_host_impl(ctx, "rm_intersect_rays", false, origins, directions, n_rays, hits); });
}

rm_status rm_occluded_rays(rm_ctx *ctx, const rm_vec3 *origins, const rm_vec3 *directions, uint32_t n_rays, uint8_t *occluded) {
    return guarded(ctx, "rm_occluded_rays", [&]() { return rays_host_impl(ctx, "rm_occluded_rays", true, origins, directions, n_rays, occluded); });
}

rm_status rm_intersect_rays_device(rm_ctx *ctx, const void *device_origins, const void *device_directions, uint32_t n_rays,
                                   void *device_hits, void *hip_stream) {
    return guarded(ctx, "rm_intersect_rays_device", [&]() {
        return rays_device_impl(ctx, "rm_intersect_rays_device", false, device_origins, device_directions, n_rays, device_hits, hip_stream);
    });
}

rm_status rm_occluded_rays_device(rm_ctx *ctx, const void *device_origins, const void *device_directions, uint32_t n_rays,
                                  void *device_occluded, void *hip_stream) {
    return guarded(ctx, "rm_occluded_rays_device", [&]() {
        return rays_device_impl(ctx, "rm_occluded_rays_device", true, device_origins, device_directions, n_rays, device_occluded, hip_stream);
    });
}

rm_status rm_pick(rm_ctx *ctx, const rm_params *params, uint32_t x, uint32_t y, rm_hit *hit) {
    return guarded(ctx, "rm_pick", [&]() { return rm_pick_impl(ctx, params, x, y, hit); });
}

rm_status rm_primary_hits_device(rm_ctx *ctx, const rm_params *params, void *device_hits, void *hip_stream) {
    return guarded(ctx, "rm_primary_hits_device", [&]() { return rm_primary_hits_device_impl(ctx, params, device_hits, hip_stream); });
}

}  // extern "C"

// ---- ranged queries: rays with a range, segments, lights (rm_query.hip's ranged kernels) ----------------------------------
static rm_status launch_ranged(rm_ctx *ctx, const char *who, int kind, RangedArgs &q, hipStream_t stream) {
    q.H = ctx->image.H;
    q.pid_map = ctx->d_pid_map;
    const uint64_t blocks = (q.n + 63u) / 64u;
    if (blocks > 0x7FFFFFFFull) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": too many answers for one launch");
    const bool bvh = ctx->image.H.off_bvh_spheres != 0 || ctx->image.H.off_bvh_triangles != 0;   // (as launch_query)
    const void *fn = rm_ranged_kernel(kind, bvh);
    if (!fn) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "ranged query: no such kernel");
    void *args[] = {(void *)&ctx->d_scene, (void *)&q};
    RM_HIP(ctx, hipLaunchKernel(fn, dim3((uint32_t)blocks), dim3(64), args, 0, stream));
    return RM_OK;
}

static bool finite3(const rm_vec3 &v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); }

static rm_status check_ranges(rm_ctx *ctx, const char *who, const rm_range *r, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) {
        const bool nan = std::isnan(r[i].t_min) || std::isnan(r[i].t_max);
        if (nan || !(r[i].t_min >= 0.) || !(r[i].t_max >= r[i].t_min)) {
            char buf[224];
            std::snprintf(buf, sizeof buf, "%s: ray %u: range [%g, %g]: %s", who, i, r[i].t_min, r[i].t_max,
                          nan ? "not a number" : !(r[i].t_min >= 0.) ? "t_min < 0" : "t_max < t_min");
            return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
        }
    }
    return RM_OK;
}

static rm_status check_skin(rm_ctx *ctx, const char *who, double skin) {
    if (std::isfinite(skin) && skin >= 0.) return RM_OK;
    char buf[160];
    std::snprintf(buf, sizeof buf, "%s: skin %g must be finite and >= 0", who, skin);
    return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
}

static rm_status check_segments(rm_ctx *ctx, const char *who, const rm_vec3 *a, const rm_vec3 *b, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) {
        const bool finite = finite3(a[i]) && finite3(b[i]);
        if (!finite || (a[i].x == b[i].x && a[i].y == b[i].y && a[i].z == b[i].z)) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "%s: segment %u: from (%g, %g, %g) to (%g, %g, %g): %s", who, i, a[i].x, a[i].y, a[i].z,
                          b[i].x, b[i].y, b[i].z, finite ? "from == to" : "not finite");
            return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
        }
    }
    return RM_OK;
}

static rm_status check_points(rm_ctx *ctx, const char *who, const rm_vec3 *p, const rm_vec3 *nrm, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) {
        const bool finite = finite3(p[i]) && finite3(nrm[i]);
        if (!finite || (nrm[i].x == 0. && nrm[i].y == 0. && nrm[i].z == 0.)) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "%s: point %u: (%g, %g, %g), normal (%g, %g, %g): %s", who, i, p[i].x, p[i].y, p[i].z,
                          nrm[i].x, nrm[i].y, nrm[i].z, finite ? "the normal is zero" : "not finite");
            return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
        }
    }
    return RM_OK;
}

// mode and n_lights of rm_lights_visible*: what a host can get wrong without touching an element
static rm_status check_lights_call(rm_ctx *ctx, const char *who, uint32_t n_lights, uint32_t mode) {
    if (mode != RM_LIGHTS_AS_RENDERED && mode != RM_LIGHTS_CLIPPED) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "%s: mode %u is neither RM_LIGHTS_AS_RENDERED (0) nor RM_LIGHTS_CLIPPED (1)", who, mode);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    if (n_lights != ctx->image.H.n_lights) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "%s: n_lights %u, the resident scene has %u", who, n_lights, ctx->image.H.n_lights);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    return RM_OK;
}

// What every ranged entry point asks first.  *done: nothing (more) to do, return the status.
static rm_status ranged_preamble(rm_ctx *ctx, const char *who, uint64_t n, bool *done) {
    *done = true;
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
    if (!ctx->have_scene) return ctx_fail(ctx, RM_ERR_NO_SCENE, std::string(who) + ": no scene uploaded (rm_scene_upload)");
    *done = n == 0;
    return RM_OK;
}

// Host variant: `n_in` arrays of n elements go across (sizes in `in_bytes`), the kernel runs, out_bytes come back.
struct RangedHostIn { const void *src; size_t bytes; };
static rm_status ranged_host_run(rm_ctx *ctx, const char *who, int kind, RangedArgs &q, const RangedHostIn (&in)[3], void *out,
                                 size_t out_bytes) {
    RM_HIP(ctx, hipSetDevice(ctx->device));
    char *buf = nullptr;
    if (rm_status sst = query_staging(ctx, in[0].bytes + in[1].bytes + in[2].bytes + out_bytes, &buf)) return sst;
    char *at[4] = {buf, buf + in[0].bytes, buf + in[0].bytes + in[1].bytes, buf + in[0].bytes + in[1].bytes + in[2].bytes};
    for (int k = 0; k < 3; k++)
        if (in[k].bytes) RM_HIP(ctx, hipMemcpyAsync(at[k], in[k].src, in[k].bytes, hipMemcpyHostToDevice, ctx->stream));
    q.a = reinterpret_cast<const rm_vec3 *>(at[0]);
    q.b = reinterpret_cast<const rm_vec3 *>(at[1]);
    q.ranges = reinterpret_cast<const rm_range *>(at[2]);
    if (kind == RM_RANGED_CLOSEST) q.hits = reinterpret_cast<rm_hit *>(at[3]);
    else q.out = reinterpret_cast<uint8_t *>(at[3]);
    if (rm_status qst = launch_ranged(ctx, who, kind, q, ctx->stream)) return qst;
    RM_HIP(ctx, hipMemcpyAsync(out, at[3], out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RM_OK;
}

static rm_status rays_ranged_host_impl(rm_ctx *ctx, const char *who, bool occlusion, const rm_vec3 *origins, const rm_vec3 *directions,
                                       const rm_range *ranges, uint32_t n_rays, void *out) {
    bool done;
    if (rm_status st = ranged_preamble(ctx, who, n_rays, &done)) return st;
    if (done) return RM_OK;
    if (!origins || !directions || !ranges || !out) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL array");
    if (rm_status cst = check_rays(ctx, who, origins, directions, n_rays)) return cst;
    if (rm_status cst = check_ranges(ctx, who, ranges, n_rays)) return cst;
    RangedArgs q{};
    q.n = n_rays;
    const size_t vb = (size_t)n_rays * sizeof(rm_vec3);
    return ranged_host_run(ctx, who, occlusion ? RM_RANGED_OCCLUDED : RM_RANGED_CLOSEST, q,
                           {{origins, vb}, {directions, vb}, {ranges, (size_t)n_rays * sizeof(rm_range)}}, out,
                           (size_t)n_rays * (occlusion ? sizeof(uint8_t) : sizeof(rm_hit)));
}

static rm_status rays_ranged_device_impl(rm_ctx *ctx, const char *who, bool occlusion, const void *origins, const void *directions,
                                         const void *ranges, uint32_t n_rays, void *out, void *hip_stream) {
    bool done;
    if (rm_status st = ranged_preamble(ctx, who, n_rays, &done)) return st;
    if (done) return RM_OK;
    if (!origins || !directions || !ranges || !out) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL device buffer");
    RM_HIP(ctx, hipSetDevice(ctx->device));
    RangedArgs q{};
    q.n = n_rays;
    q.a = static_cast<const rm_vec3 *>(origins);
    q.b = static_cast<const rm_vec3 *>(directions);
    q.ranges = static_cast<const rm_range *>(ranges);
    if (occlusion) q.out = static_cast<uint8_t *>(out);
    else q.hits = static_cast<rm_hit *>(out);
    return launch_ranged(ctx, who, occlusion ? RM_RANGED_OCCLUDED : RM_RANGED_CLOSEST, q, (hipStream_t)hip_stream);
}

static rm_status segments_impl(rm_ctx *ctx, const char *who, bool device, const void *from, const void *to, uint32_t n, double skin,
                               void *visible, void *hip_stream) {
    bool done;
    if (rm_status st = ranged_preamble(ctx, who, n, &done)) return st;
    if (done) return RM_OK;
    if (!from || !to || !visible) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + (device ? ": NULL device buffer" : ": NULL array"));
    if (rm_status cst = check_skin(ctx, who, skin)) return cst;
    RangedArgs q{};
    q.n = n;
    q.skin = skin;
    if (!device) {
        if (rm_status cst = check_segments(ctx, who, static_cast<const rm_vec3 *>(from), static_cast<const rm_vec3 *>(to), n)) return cst;
        const size_t vb = (size_t)n * sizeof(rm_vec3);
        return ranged_host_run(ctx, who, RM_RANGED_SEGMENTS, q, {{from, vb}, {to, vb}, {nullptr, 0}}, visible, (size_t)n);
    }
    RM_HIP(ctx, hipSetDevice(ctx->device));
    q.a = static_cast<const rm_vec3 *>(from);
    q.b = static_cast<const rm_vec3 *>(to);
    q.out = static_cast<uint8_t *>(visible);
    return launch_ranged(ctx, who, RM_RANGED_SEGMENTS, q, (hipStream_t)hip_stream);
}

static rm_status lights_impl(rm_ctx *ctx, const char *who, bool device, const void *points, const void *normals, uint32_t n_points,
                             uint32_t n_lights, uint32_t mode, void *lit, void *hip_stream) {
    bool done;
    if (rm_status st = ranged_preamble(ctx, who, n_points, &done)) return st;
    if (done) return RM_OK;
    if (rm_status cst = check_lights_call(ctx, who, n_lights, mode)) return cst;
    if (n_lights == 0) return RM_OK;                                  // a scene without lights: nothing to write
    if (!points || !normals || !lit) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + (device ? ": NULL device buffer" : ": NULL array"));
    RangedArgs q{};
    q.n = (uint64_t)n_points * n_lights;
    q.n_lights = n_lights;
    q.mode = mode;
    if (!device) {
        if (rm_status cst = check_points(ctx, who, static_cast<const rm_vec3 *>(points), static_cast<const rm_vec3 *>(normals), n_points)) return cst;
        const size_t vb = (size_t)n_points * sizeof(rm_vec3);
        return ranged_host_run(ctx, who, RM_RANGED_LIGHTS, q, {{points, vb}, {normals, vb}, {nullptr, 0}}, lit, (size_t)q.n);
    }
    RM_HIP(ctx, hipSetDevice(ctx->device));
    q.a = static_cast<const rm_vec3 *>(points);
    q.b = static_cast<const rm_vec3 *>(normals);
    q.out = static_cast<uint8_t *>(lit);
    return launch_ranged(ctx, who, RM_RANGED_LIGHTS, q, (hipStream_t)hip_stream);
}

extern "C" {

rm_status rm_intersect_rays_ranged(rm_ctx *ctx, const rm_vec3 *origins, const rm_vec3 *directions, const rm_range *ranges, uint32_t n_rays,
                                   rm_hit *hits) {
    return guarded(ctx, "rm_intersect_rays_ranged",
                   [&]() { return rays_ranged_host_impl(ctx, "rm_intersect_rays_ranged", false, origins, directions, ranges, n_rays, hits); });
}

rm_status rm_occluded_rays_ranged(rm_ctx *ctx, const rm_vec3 *origins, const rm_vec3 *directions, const rm_range *ranges, uint32_t n_rays,
                                  uint8_t *occluded) {
    return guarded(ctx, "rm_occluded_rays_ranged",
                   [&]() { return rays_ranged_host_impl(ctx, "rm_occluded_rays_ranged", true, origins, directions, ranges, n_rays, occluded); });
}

rm_status rm_intersect_rays_ranged_device(rm_ctx *ctx, const void *device_origins, const void *device_directions, const void *device_ranges,
                                          uint32_t n_rays, void *device_hits, void *hip_stream) {
    return guarded(ctx, "rm_intersect_rays_ranged_device", [&]() {
        return rays_ranged_device_impl(ctx, "rm_intersect_rays_ranged_device", false, device_origins, device_directions, device_ranges, n_rays,
                                       device_hits, hip_stream);
    });
}

rm_status rm_occluded_rays_ranged_device(rm_ctx *ctx, const void *device_origins, const void *device_directions, const void *device_ranges,
                                         uint32_t n_rays, void *device_occluded, void *hip_stream) {
    return guarded(ctx, "rm_occluded_rays_ranged_device", [&]() {
        return rays_ranged_device_impl(ctx, "rm_occluded_rays_ranged_device", true, device_origins, device_directions, device_ranges, n_rays,
                                       device_occluded, hip_stream);
    });
}

rm_status rm_visible_segments(rm_ctx *ctx, const rm_vec3 *from, const rm_vec3 *to, uint32_t n, double skin, uint8_t *visible) {
    return guarded(ctx, "rm_visible_segments", [&]() { return segments_impl(ctx, "rm_visible_segments", false, from, to, n, skin, visible, nullptr); });
}

rm_status rm_visible_segments_device(rm_ctx *ctx, const void *device_from, const void *device_to, uint32_t n, double skin,
                                     void *device_visible, void *hip_stream) {
    return guarded(ctx, "rm_visible_segments_device",
                   [&]() { return segments_impl(ctx, "rm_visible_segments_device", true, device_from, device_to, n, skin, device_visible, hip_stream); });
}

rm_status rm_lights_visible(rm_ctx *ctx, const rm_vec3 *points, const rm_vec3 *normals, uint32_t n_points, uint32_t n_lights, uint32_t mode,
                            uint8_t *lit) {
    return guarded(ctx, "rm_lights_visible",
                   [&]() { return lights_impl(ctx, "rm_lights_visible", false, points, normals, n_points, n_lights, mode, lit, nullptr); });
}

rm_status rm_lights_visible_device(rm_ctx *ctx, const void *device_points, const void *device_normals, uint32_t n_points, uint32_t n_lights,
                                   uint32_t mode, void *device_lit, void *hip_stream) {
    return guarded(ctx, "rm_lights_visible_device", [&]() {
        return lights_impl(ctx, "rm_lights_visible_device", true, device_points, device_normals, n_points, n_lights, mode, device_lit, hip_stream);
    });
}

}  // extern "C"
