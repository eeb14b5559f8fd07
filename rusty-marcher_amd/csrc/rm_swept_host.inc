// rm_swept_host.inc -- host side of the swept hierarchies (include/rusty_marcher_amd.h, "swept hierarchies"); included at the end
// of rm_device.hip, behind rm_motion_shapes_host.inc and rm_converge_moving_host.inc whose argument blocks, checks and flat
// launches (launch_moving, launch_converge_moving) it uses and whose ticks it serves.  The refit is rm_swept_image.cpp's (host
// arithmetic), the kernels are rm_swept.hip's and rm_converge_swept.hip's.
//
// A swept hierarchy (rm_swept) is a device copy of the resident image's blob with refitted boxes, and the image epoch it was built
// at.  The two device calls are their moving-shapes siblings with that blob in place of the resident one: they touch no render
// state and keep none of their own, one launch (three steps for the converging call) on the caller's stream, nothing waited for.
// The ticks that move a shape -- the moving shapes', the moving spheres' (rm_motion_host.inc, rm_converge_motion_host.inc) and
// the moving camera's given velocities (rm_camera_host.inc, behind this file) -- build one of their own from the velocities and
// the shutter (rm_tick_swept) and keep it until the image, a velocity or the shutter changes: one for all six, so a camera tick
// behind a moving shapes' tick with the same velocities and shutter builds nothing.  What the last tick's launch walked, and how
// many were built, rm_swept_tick_info reports (rm_camera_swept_host.inc).

struct rm_swept {
    double *d_blob = nullptr;
    uint64_t image_epoch = 0;                // rm_ctx::image_epoch when it was built
};

// The ticks' own: the hierarchy, and the velocities and shutter its extents came from
struct rm_tick_swept {
    rm_swept *swept = nullptr;
    std::vector<rm_vec3> velocities;
    double shutter = 0.;
    bool ready = false;                      // the tick in progress may walk `swept`: built for its image, velocities and shutter
};

// The description the resident image was built from, as the upload kept it (rm_ctx::desc_bytes): a view, valid until the next upload
static rm_scene_desc resident_desc(const rm_ctx *ctx) {
    rm_scene_desc d{};
    const unsigned char *p = ctx->desc_bytes.data();
    const size_t *n = ctx->desc_sizes;
    d.shapes = reinterpret_cast<const rm_shape_ref *>(p); d.n_shapes = (uint32_t)(n[0] / sizeof(rm_shape_ref)); p += n[0];
    d.spheres = reinterpret_cast<const rm_sphere *>(p); d.n_spheres = (uint32_t)(n[1] / sizeof(rm_sphere)); p += n[1];
    d.polygons = reinterpret_cast<const rm_polygon *>(p); d.n_polygons = (uint32_t)(n[2] / sizeof(rm_polygon)); p += n[2];
    d.polygon_vertices = reinterpret_cast<const rm_vec3 *>(p); d.n_polygon_vertices = (uint32_t)(n[3] / sizeof(rm_vec3)); p += n[3];
    d.triangles = reinterpret_cast<const rm_triangle *>(p); d.n_triangles = (uint32_t)(n[4] / sizeof(rm_triangle)); p += n[4];
    d.lights = reinterpret_cast<const rm_light *>(p); d.n_lights = (uint32_t)(n[5] / sizeof(rm_light));
    d.camera = ctx->camera;
    return d;
}

static void swept_release(rm_swept *s, bool device_ok) {
    if (!s) return;
    if (s->d_blob && device_ok) (void)hipFree(s->d_blob);
    delete s;
}

// Refits the resident image over lo..hi and copies the blob across (waits for the copy; a scene is resident)
static rm_status swept_build(rm_ctx *ctx, const char *who, const double *lo, const double *hi, uint32_t n_shapes, rm_swept **out) {
    const rm_scene_desc d = resident_desc(ctx);
    std::vector<double> blob;
    std::string refusal;
    if (rm_status rst = rm_swept_refit(who, &d, ctx->image, lo, hi, n_shapes, blob, refusal)) return ctx_fail(ctx, rst, refusal);
    RM_HIP(ctx, hipSetDevice(ctx->device));
    rm_swept *s = new rm_swept();
    s->image_epoch = ctx->image_epoch;
    hipError_t e = hipMalloc(&s->d_blob, blob.size() * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(s->d_blob, blob.data(), blob.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        swept_release(s, true);
        return ctx_fail(ctx, RM_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
    *out = s;
    return RM_OK;
}

// What both device calls check of their handle, behind every other check: there, this context's, and of the resident image
static rm_status check_swept(rm_ctx *ctx, const char *who, const rm_swept *s) {
    if (!s) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL swept");
    // (looked up, not looked into: a handle of another context, or one already freed, is not read)
    if (std::find(ctx->swept_handles.begin(), ctx->swept_handles.end(), s) == ctx->swept_handles.end())
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": swept is not a handle of this context");
    if (s->image_epoch != ctx->image_epoch)
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": swept was built before the scene last changed (build it again)");
    return RM_OK;
}

// launch_moving over the blob of `s`
static rm_status launch_swept(rm_ctx *ctx, const rm_swept *s, const accum_call &c, const void *offsets, const void *shape_offsets) {
    MotionArgs a{};
    a.S.A = accum_args(ctx, c);
    a.S.offsets = static_cast<const double *>(offsets);
    a.shape_offsets = static_cast<const double *>(shape_offsets);
    a.pid_map = ctx->d_pid_map;
    a.n_shapes = resident_shape_count(ctx);
    return launch_shading(ctx, shade_family{"swept hierarchy", rm_swept_kernel, s->d_blob}, a.S.A.L.max_depth, lens_extent(ctx, a.S.A.L), a, c.stream);
}

// launch_converge_moving over the blob of `s`
static rm_status launch_converge_swept(rm_ctx *ctx, const rm_swept *s, const rm_params *p, const rm_lens *lens, const rm_converge *c,
                                       const void *table, uint32_t table_rows, const void *offsets, const void *shape_offsets, int fresh,
                                       const rm_converge_frame *b, hipStream_t stream) {
    ConvergeMotionArgs m{};
    m.C = converge_args(ctx, p, lens, c, table, table_rows, offsets, fresh, b);
    m.shape_offsets = static_cast<const double *>(shape_offsets);
    m.pid_map = ctx->d_pid_map;
    m.n_shapes = resident_shape_count(ctx);
    return launch_converge_with(ctx, shade_family{"converging over a swept hierarchy", rm_converge_swept_kernel, s->d_blob}, m, m.C, stream);
}

// ---- the ticks' own hierarchy ----

static void tick_swept_destroy(rm_ctx *ctx, bool device_ok) {
    for (rm_swept *s : ctx->swept_handles) swept_release(s, device_ok);   // (the callers' handles nobody freed)
    ctx->swept_handles.clear();
    if (!ctx->tick_swept) return;
    swept_release(ctx->tick_swept->swept, device_ok);
    delete ctx->tick_swept;
    ctx->tick_swept = nullptr;
}

// Whether the ticks that move a shape walk a swept hierarchy over the resident image: wherever it holds a hierarchy, unless
// RM_SWEPT_BVH=0 (rm_knobs::swept_bvh).  No primitive-count threshold: on the smallest hierarchy of the suite, the Cornell box's 36
// triangles, the swept pass takes 0.50 to 0.73 of the flat pass's time (profiles/swept_figures.txt; under a moving camera and for
// the moving spheres' ticks: profiles/camera_swept_figures.txt).
static bool tick_walks_swept(const rm_ctx *ctx) {
    const rm_dev_header &H = ctx->image.H;
    return ctx->knobs.swept_bvh && (H.off_bvh_spheres || H.off_bvh_triangles);
}

// In front of a tick that moves a shape: makes the ticks' hierarchy the one of the resident image, `velocities` and `shutter`, and
// says so in `ready`.  Arguments the tick is about to refuse build nothing and are left for it to name -- with `spheres_only`
// (the moving spheres' ticks) a velocity on anything but a sphere is among them, and a scene without spheres, where those ticks
// need not stage a shape table, is left alone; so are extents that are not finite (a product that overflows): that tick walks
// flat.  The streams the ticks launch on were waited for, so the old blob is free to go.
static rm_status tick_swept_prepare(rm_ctx *ctx, const char *who, const rm_vec3 *velocities, uint32_t n_shapes, double shutter,
                                    bool spheres_only) {
    if (!ctx) return RM_OK;
    if (!ctx->tick_swept) ctx->tick_swept = new rm_tick_swept();
    rm_tick_swept &t = *ctx->tick_swept;
    t.ready = false;
    if (!ctx->have_scene || !tick_walks_swept(ctx)) return RM_OK;
    if (n_shapes != resident_shape_count(ctx) || n_shapes == 0u || !velocities) return RM_OK;
    if (rm_check_velocities(who, velocities, n_shapes, shutter) != RM_OK) return RM_OK;
    if (spheres_only) {
        if (ctx->image.H.n_spheres == 0u) return RM_OK;
        for (uint32_t k = 0; k < n_shapes; k++) {                         // (check_rules' rule: only spheres move)
            const rm_vec3 &v = velocities[k];
            if (resident_shape(ctx, k).kind != RM_SHAPE_SPHERE && (v.x != 0. || v.y != 0. || v.z != 0.)) return RM_OK;
        }
    }
    const bool same = t.swept && t.swept->image_epoch == ctx->image_epoch && t.velocities.size() == n_shapes &&
                      std::memcmp(t.velocities.data(), velocities, (size_t)n_shapes * sizeof(rm_vec3)) == 0 &&
                      std::memcmp(&t.shutter, &shutter, sizeof shutter) == 0;
    if (!same) {
        std::vector<double> lo(3u * (size_t)n_shapes), hi(lo.size());
        if (rm_swept_motion_extents(velocities, n_shapes, shutter, lo.data(), hi.data()) != RM_OK) return RM_OK;
        for (size_t w = 0; w < lo.size(); w++)
            if (!std::isfinite(lo[w]) || !std::isfinite(hi[w])) return RM_OK;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        swept_release(t.swept, true);
        t.swept = nullptr;
        if (rm_status bst = swept_build(ctx, who, lo.data(), hi.data(), n_shapes, &t.swept)) return bst;
        t.velocities.assign(velocities, velocities + n_shapes);
        t.shutter = shutter;
        ctx->swept_builds += 1u;
    }
    t.ready = true;
    return RM_OK;
}

static void tick_swept_done(rm_ctx *ctx) {
    if (ctx && ctx->tick_swept) ctx->tick_swept->ready = false;
}

// The hierarchy the tick in progress may walk: the ticks' own where tick_swept_prepare made it ready and the pass has a shape
// table, else NULL (the flat walk).  A launch that takes it says so (rm_swept_tick_info).
static const rm_swept *tick_swept_ready(const rm_ctx *ctx, const void *shape_offsets) {
    const rm_tick_swept *t = ctx->tick_swept;
    return t && t->ready && shape_offsets ? t->swept : nullptr;
}

// The launches the moving shapes' ticks hand their tick bodies: the swept walk where tick_swept_prepare made one ready (and the
// pass has a shape table), else the flat one
static rm_status launch_moving_tick(rm_ctx *ctx, const accum_call &c, const void *offsets, const void *shape_offsets) {
    if (const rm_swept *s = tick_swept_ready(ctx, shape_offsets)) {
        ctx->swept_walked = 1u;
        return launch_swept(ctx, s, c, offsets, shape_offsets);
    }
    return launch_moving(ctx, c, offsets, shape_offsets);
}

// ... and the moving spheres' ticks theirs: check_rules refused a velocity on anything but a sphere, so the staged table's other
// rows are zeros, and a moving shapes' pass with such rows writes the moving spheres' bytes (include/rusty_marcher_amd.h, "moving
// shapes"): the swept walk is rm_swept.hip's, no kernel of its own
static rm_status launch_motion_tick(rm_ctx *ctx, const accum_call &c, const void *offsets, const void *shape_offsets) {
    if (const rm_swept *s = tick_swept_ready(ctx, shape_offsets)) {
        ctx->swept_walked = 1u;
        return launch_swept(ctx, s, c, offsets, shape_offsets);
    }
    return launch_motion(ctx, c, offsets, shape_offsets);
}

static rm_status launch_converge_moving_tick(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c, const void *table,
                                             uint32_t table_rows, const void *offsets, const void *shape_offsets, int fresh,
                                             const rm_converge_frame *b, hipStream_t stream) {
    if (const rm_swept *s = tick_swept_ready(ctx, shape_offsets)) {
        ctx->swept_walked = 1u;
        return launch_converge_swept(ctx, s, p, lens, c, table, table_rows, offsets, shape_offsets, fresh, b, stream);
    }
    return launch_converge_moving(ctx, p, lens, c, table, table_rows, offsets, shape_offsets, fresh, b, stream);
}

static rm_status launch_converge_motion_tick(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c, const void *table,
                                             uint32_t table_rows, const void *offsets, const void *shape_offsets, int fresh,
                                             const rm_converge_frame *b, hipStream_t stream) {
    if (const rm_swept *s = tick_swept_ready(ctx, shape_offsets)) {
        ctx->swept_walked = 1u;
        return launch_converge_swept(ctx, s, p, lens, c, table, table_rows, offsets, shape_offsets, fresh, b, stream);
    }
    return launch_converge_motion(ctx, p, lens, c, table, table_rows, offsets, shape_offsets, fresh, b, stream);
}

extern "C" {

rm_status rm_swept_build(rm_ctx *ctx, const double *lo, const double *hi, uint32_t n_shapes, rm_swept **out) {
    const char *who = "rm_swept_build";
    return guarded(ctx, who, [&]() -> rm_status {
        if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
        if (!out) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL out");
        *out = nullptr;
        if (!ctx->have_scene) return ctx_fail(ctx, RM_ERR_NO_SCENE, std::string(who) + ": no scene uploaded");
        ctx->swept_handles.reserve(ctx->swept_handles.size() + 1u);
        if (rm_status bst = swept_build(ctx, who, lo, hi, n_shapes, out)) return bst;
        ctx->swept_handles.push_back(*out);
        return RM_OK;
    });
}

void rm_swept_free(rm_ctx *ctx, rm_swept *swept) {
    if (!ctx || !swept) return;
    const auto it = std::find(ctx->swept_handles.begin(), ctx->swept_handles.end(), swept);
    if (it == ctx->swept_handles.end()) return;
    ctx->swept_handles.erase(it);
    const bool device_ok = !ctx->comm_stuck;
    if (device_ok && hipSetDevice(ctx->device) == hipSuccess) (void)hipDeviceSynchronize();   // a pass may still be walking it
    swept_release(swept, device_ok);
}

rm_status rm_accumulate_swept_device(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *device_table,
                                     const void *device_light_offsets, uint32_t n_lights, const void *device_shape_offsets,
                                     uint32_t n_shapes, const rm_swept *swept, uint32_t n_before, void *device_sum, void *device_mean,
                                     void *device_rgb8, void *hip_stream) {
    const char *who = "rm_accumulate_swept_device";
    return guarded(ctx, who, [&]() -> rm_status {
        if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
        if (rm_status cst = check_accum_device(ctx, who, p, lens, device_table, n_before, device_sum, device_mean)) return cst;
        const shape_table shapes{device_shape_offsets, n_shapes};
        if (rm_status ost = check_offset_tables(ctx, who, "light offsets", device_light_offsets, n_lights, &shapes)) return ost;
        if (n_shapes > 0u && !device_shape_offsets) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL shape offsets");
        if (rm_status sst = check_swept(ctx, who, swept)) return sst;
        if (refine_rows(p) == 0u) return RM_OK;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        return launch_swept(ctx, swept, accum_call{p, lens, device_table, n_before, device_sum, device_mean, device_rgb8, (hipStream_t)hip_stream},
                            n_lights > 0u ? device_light_offsets : nullptr, n_shapes > 0u ? device_shape_offsets : nullptr);
    });
}

rm_status rm_accumulate_converging_swept_device(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c,
                                                const void *device_table, uint32_t table_rows, const void *device_light_offsets,
                                                uint32_t n_lights, const void *device_shape_offsets, uint32_t n_shapes,
                                                const rm_swept *swept, int fresh, const rm_converge_frame *b, void *hip_stream) {
    const char *who = "rm_accumulate_converging_swept_device";
    return guarded(ctx, who, [&]() -> rm_status {
        if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
        const shape_table shapes{device_shape_offsets, n_shapes};
        auto tables = [&]() -> rm_status {
            if (rm_status ost = check_offset_tables(ctx, who, "light offsets", device_light_offsets, n_lights, &shapes)) return ost;
            if (n_shapes > 0u && !device_shape_offsets) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL shape offsets");
            return RM_OK;
        };
        if (rm_status cst = check_converge_call(ctx, who, p, lens, c, device_table, table_rows, b, tables)) return cst;
        if (rm_status sst = check_swept(ctx, who, swept)) return sst;
        if (refine_rows(p) == 0u) return RM_OK;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        return launch_converge_swept(ctx, swept, p, lens, c, device_table, table_rows, n_lights > 0u ? device_light_offsets : nullptr,
                                     n_shapes > 0u ? device_shape_offsets : nullptr, fresh, b, (hipStream_t)hip_stream);
    });
}

}  // extern "C"
