// rm_accum_host.inc -- host side of the progressive frames (include/rusty_marcher_amd.h, "progressive frames"); included at the
// end of rm_device.hip, behind rm_lens_host.inc whose checks (check_lens), argument block (lens_args) and grid (lens_extent, with
// RM_LENS_MAX_BLOCKS) it reuses.  The kernel is rm_accum.hip's.
//
// rm_accumulate_lens_device touches no render state and keeps none of its own: one launch on the caller's stream, nothing
// waited for.  rm_render_progressive is that on the context's stream with a staged slice of rm_lens_sequence and three
// buffers the context owns (sum, mean, bytes: not the resident frame, not the lens frame), the count of samples in the sum
// and the key that says which view the sum belongs to.

// phi_b(s): the digits of s in base b mirrored at the point, as the integer pair (r, q) -- r / q is the value
static void digit_reversed(uint32_t s, uint32_t b, uint64_t *r, uint64_t *q) {
    uint64_t rr = 0, qq = 1;
    while (s > 0u) {
        rr = rr * b + s % b;
        qq *= b;
        s /= b;
    }
    *r = rr;
    *q = qq;
}

static double radical_inverse(uint32_t s, uint32_t b) {
    uint64_t r, q;
    digit_reversed(s, b, &r, &q);
    return (double)r / (double)q;
}

// What both entry points check of params and lens (ctx is not NULL): check_lens with a table and a frame that are there.
static rm_status check_accum(rm_ctx *ctx, const char *who, const rm_params *p, const rm_lens *lens) {
    const char present = 0;
    return check_lens(ctx, who, p, lens, &present, &present);
}

// The launch on `stream`; everything was checked, rows > 0.
static rm_status launch_accum(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *table, uint32_t n_before, void *sum,
                              void *mean, void *rgb8, hipStream_t stream) {
    AccumArgs a{};
    a.L = lens_args(ctx, p, lens, table, nullptr);
    a.n_before = n_before;
    a.sum = static_cast<double *>(sum);
    a.mean = static_cast<double *>(mean);
    a.rgb8 = static_cast<uint8_t *>(rgb8);
    return launch_shading(ctx, shade_family{"progressive", rm_accum_kernel}, a.L.max_depth, lens_extent(ctx, a.L), a, stream);
}

// What the device calls (this one and rm_accumulate_soft_device) check of their own arguments (ctx is not NULL).
static rm_status check_accum_device(rm_ctx *ctx, const char *who, const rm_params *p, const rm_lens *lens, const void *device_table,
                                    uint32_t n_before, const void *device_sum, const void *device_mean) {
    if (rm_status cst = check_accum(ctx, who, p, lens)) return cst;
    if (!device_table) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL table");
    if (!device_sum) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL sum");
    if (device_mean == device_sum) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": the mean would overwrite the sum (device_mean == device_sum)");
    if ((uint64_t)n_before + lens->n_samples > RM_PROGRESSIVE_MAX_SAMPLES) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "%s: n_before + n_samples = %u + %u is more than %u", who, n_before, lens->n_samples, RM_PROGRESSIVE_MAX_SAMPLES);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    return RM_OK;
}

static rm_status rm_accumulate_lens_device_impl(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *device_table,
                                                uint32_t n_before, void *device_sum, void *device_mean, void *device_rgb8, void *hip_stream) {
    const char *who = "rm_accumulate_lens_device";
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
    if (rm_status cst = check_accum_device(ctx, who, p, lens, device_table, n_before, device_sum, device_mean)) return cst;
    if (refine_rows(p) == 0u) return RM_OK;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    return launch_accum(ctx, p, lens, device_table, n_before, device_sum, device_mean, device_rgb8, (hipStream_t)hip_stream);
}

// The view a sum belongs to, byte for byte (no padding: doubles and pairs of words)
struct rm_progressive_key {
    double fov, half_fov, height, width, ratio;
    uint32_t frame_width, frame_height, max_depth, oriented;
    rm_vec3 background;
    double aperture, focus;
    rm_vec3 camera;
    rm_camera_basis basis;
    uint64_t copies;
    uint32_t soft, n_lights;                 // frames with radii: 1 and the radii's count (their bytes: rm_progressive::radii); else 0, 0
    uint32_t motion, n_shapes;               // rm_render_progressive_motion's frames: 1 and the velocities' count (their bytes:
    double shutter;                          // rm_progressive::velocities) and the shutter; else 0, 0, 0
};

// A tick's moving spheres (rm_motion_host.inc): rm_render_progressive_motion's arguments; the other ticks pass none
struct rm_motion_tick {
    const rm_vec3 *velocities;
    uint32_t n_shapes;
    double shutter;
};

static rm_progressive_key progressive_key_of(const rm_ctx *ctx, const rm_params *p, const rm_lens *lens, bool soft, uint32_t n_lights,
                                             const rm_motion_tick *motion = nullptr) {
    rm_progressive_key key;
    std::memset(&key, 0, sizeof key);
    key.fov = p->fov; key.half_fov = p->half_fov; key.height = p->height; key.width = p->width; key.ratio = p->ratio;
    key.frame_width = p->frame_width; key.frame_height = p->frame_height; key.max_depth = p->max_depth;
    key.oriented = ctx->oriented ? 1u : 0u;
    key.background = p->background;
    key.aperture = lens->aperture; key.focus = lens->focus;
    key.camera = ctx->camera;
    key.basis = ctx->basis;
    key.copies = ctx->upload_copies;
    key.soft = soft ? 1u : 0u; key.n_lights = n_lights;
    if (motion) { key.motion = 1u; key.n_shapes = motion->n_shapes; key.shutter = motion->shutter; }
    return key;
}

// The progressive state of a context (rm_ctx::progressive; made on the first call, released by rm_destroy)
struct rm_progressive {
    void *d_table = nullptr;                 // RM_LENS_MAX_SAMPLES rows
    void *d_sum = nullptr, *d_mean = nullptr, *d_rgb8 = nullptr;
    size_t pixels = 0;                       // the three buffers have room for that many
    double table[RM_LENS_MAX_SAMPLES * 4u];  // the slice as staged
    bool have_key = false;                   // a call has succeeded, and nothing failed half-way since
    rm_progressive_key key;
    uint32_t n = 0;                          // samples a pixel in the sum
    // area lights (rm_soft_host.inc): the radii the sum belongs to, beside the key, and the staged slice of rm_light_sequence
    std::vector<double> radii, offsets;
    void *d_offsets = nullptr;
    size_t offsets_bytes = 0;                // d_offsets has room for that many
    // moving spheres (rm_motion_host.inc): the velocities the sum belongs to, and the staged slice of rm_motion_sequence
    std::vector<rm_vec3> velocities;
    std::vector<double> shape_offsets;
    void *d_shape_offsets = nullptr;
    size_t shape_offsets_bytes = 0;          // d_shape_offsets has room for that many
};

// rm_soft_host.inc: the check of a soft tick's radii, and the launch with an offset table
static rm_status check_soft_radii(rm_ctx *ctx, const char *who, const double *radii, uint32_t n_lights);
static rm_status launch_soft(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *table, const void *offsets, uint32_t n_before,
                             void *sum, void *mean, void *rgb8, hipStream_t stream);

// rm_motion_host.inc: the check of a motion tick's velocities and shutter, and the launch with both offset tables
static rm_status check_motion_tick(rm_ctx *ctx, const char *who, const rm_motion_tick &m);
static rm_status launch_motion(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const void *table, const void *offsets,
                               const void *shape_offsets, uint32_t n_before, void *sum, void *mean, void *rgb8, hipStream_t stream);

static void progressive_destroy(rm_ctx *ctx, bool device_ok) {
    rm_progressive *g = ctx->progressive;
    if (!g) return;
    for (void *b : {g->d_table, g->d_sum, g->d_mean, g->d_rgb8, g->d_offsets, g->d_shape_offsets})
        if (b && device_ok) (void)hipFree(b);
    delete g;
    ctx->progressive = nullptr;
}

// `soft`: rm_render_progressive_soft's tick -- n_lights radii (checked here), the slice of rm_light_sequence staged beside the
// table's and the kernel of rm_soft.hip; else radii is NULL, n_lights 0 and everything as it was before there were area lights.
// `motion`: rm_render_progressive_motion's tick -- the velocities and the shutter (checked here), the slice of rm_motion_sequence
// staged as well, light offsets for every light of the scene (zeros where `soft` is off) and the kernel of rm_motion.hip; else NULL.
static rm_status rm_render_progressive_impl(rm_ctx *ctx, const char *who, const rm_params *p, const rm_lens *lens, bool soft, const double *radii,
                                            uint32_t n_lights, int restart, double *host_rgb, uint8_t *host_rgb8, uint32_t *n_total,
                                            rm_timing *timing, const rm_motion_tick *motion = nullptr) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
    const auto t_begin = std::chrono::steady_clock::now();
    if (rm_status cst = check_accum(ctx, who, p, lens)) return cst;
    if (soft)
        if (rm_status rst = check_soft_radii(ctx, who, radii, n_lights)) return rst;
    if (motion)
        if (rm_status mst = check_motion_tick(ctx, who, *motion)) return mst;
    const uint32_t n_shapes = motion ? motion->n_shapes : 0u;
    const uint32_t rows = refine_rows(p);
    double kernel_ms = 0., d2h_ms = 0.;
    uint32_t total = 0u;
    if (rows > 0u) {
        if (!ctx->progressive) ctx->progressive = new rm_progressive();
        rm_progressive &g = *ctx->progressive;
        const rm_progressive_key key = progressive_key_of(ctx, p, lens, soft, n_lights, motion);
        const bool same = !restart && g.have_key && std::memcmp(&key, &g.key, sizeof key) == 0 && g.radii.size() == n_lights &&
                          (n_lights == 0u || std::memcmp(g.radii.data(), radii, n_lights * sizeof(double)) == 0) &&
                          g.velocities.size() == n_shapes &&
                          (n_shapes == 0u || std::memcmp(g.velocities.data(), motion->velocities, n_shapes * sizeof(rm_vec3)) == 0);
        const uint32_t n_before = same ? g.n : 0u;
        const size_t pixels = (size_t)rows * p->frame_width;
        const bool saturated = n_before + lens->n_samples > RM_PROGRESSIVE_MAX_SAMPLES;   // (then n_before > 0: the frame stands)
        RM_HIP(ctx, hipSetDevice(ctx->device));
        if (!saturated) {
            g.have_key = false;                                            // (until this call is through)
            if (!g.d_table) RM_HIP(ctx, hipMalloc(&g.d_table, sizeof g.table));
            if (g.pixels < pixels) {
                g.pixels = 0;
                const std::pair<void **, size_t> buffers[] = {{&g.d_sum, pixels * 3u * sizeof(double)}, {&g.d_mean, pixels * 3u * sizeof(double)},
                                                              {&g.d_rgb8, pixels * 3u}};
                for (const auto &b : buffers) {
                    size_t none = 0;                                       // (every one is replaced: they share one size)
                    if (rm_status gst = grow_device_buffer(ctx, b.first, &none, b.second)) return gst;
                }
                g.pixels = pixels;
            }
            if (rm_status sst = rm_lens_sequence(n_before, lens->n_samples, g.table)) return sst;
            RM_HIP(ctx, hipMemcpyAsync(g.d_table, g.table, (size_t)lens->n_samples * 4u * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            // (a motion tick's kernel reads a row for every light of the scene: zeros where the lights are points)
            const uint32_t staged_lights = motion ? ctx->image.H.n_lights : n_lights;
            const size_t n_offsets = (size_t)lens->n_samples * staged_lights * 3u;
            if (n_offsets > 0u) {                                          // (soft or motion, and the scene has lights)
                if (rm_status gst = grow_device_buffer(ctx, &g.d_offsets, &g.offsets_bytes, n_offsets * sizeof(double))) return gst;
                g.offsets.assign(n_offsets, 0.);
                if (soft)
                    if (rm_status sst = rm_light_sequence(n_before, lens->n_samples, radii, n_lights, g.offsets.data())) return sst;
                RM_HIP(ctx, hipMemcpyAsync(g.d_offsets, g.offsets.data(), n_offsets * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            }
            const size_t n_shape_offsets = (size_t)lens->n_samples * n_shapes * 3u;
            if (n_shape_offsets > 0u) {                                    // (motion, and the scene has shapes)
                if (rm_status gst = grow_device_buffer(ctx, &g.d_shape_offsets, &g.shape_offsets_bytes, n_shape_offsets * sizeof(double))) return gst;
                g.shape_offsets.resize(n_shape_offsets);
                if (rm_status sst = rm_motion_sequence(n_before, lens->n_samples, motion->velocities, n_shapes, motion->shutter, g.shape_offsets.data()))
                    return sst;
                RM_HIP(ctx, hipMemcpyAsync(g.d_shape_offsets, g.shape_offsets.data(), n_shape_offsets * sizeof(double), hipMemcpyHostToDevice,
                                           ctx->stream));
            }
            auto launch = [&]() {
                if (motion)
                    return launch_motion(ctx, p, lens, g.d_table, n_offsets > 0u ? g.d_offsets : nullptr,
                                         n_shape_offsets > 0u ? g.d_shape_offsets : nullptr, n_before, g.d_sum, g.d_mean, g.d_rgb8, ctx->stream);
                return soft ? launch_soft(ctx, p, lens, g.d_table, n_offsets > 0u ? g.d_offsets : nullptr, n_before, g.d_sum, g.d_mean, g.d_rgb8,
                                          ctx->stream)
                            : launch_accum(ctx, p, lens, g.d_table, n_before, g.d_sum, g.d_mean, g.d_rgb8, ctx->stream);
            };
            if (rm_status lst = timed_launch(ctx, &kernel_ms, launch)) return lst;
            g.key = key;
            g.radii.assign(radii, radii + n_lights);                       // (n_lights == 0: empty, radii may be NULL)
            if (motion) g.velocities.assign(motion->velocities, motion->velocities + n_shapes);
            else g.velocities.clear();
            g.n = n_before + lens->n_samples;
            g.have_key = true;
        }
        total = g.n;
        const auto t0 = std::chrono::steady_clock::now();
        if (host_rgb) RM_HIP(ctx, hipMemcpy(host_rgb, g.d_mean, pixels * 3u * sizeof(double), hipMemcpyDeviceToHost));
        if (host_rgb8) RM_HIP(ctx, hipMemcpy(host_rgb8, g.d_rgb8, pixels * 3u, hipMemcpyDeviceToHost));
        d2h_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    if (n_total) *n_total = total;
    fill_timing(timing, kernel_ms, d2h_ms, t_begin);
    return RM_OK;
}

extern "C" {

rm_status rm_lens_sequence(uint32_t first, uint32_t count, double *table) {
    if ((uint64_t)first + count > RM_PROGRESSIVE_MAX_SAMPLES) {
        char buf[128];
        std::snprintf(buf, sizeof buf, "rm_lens_sequence: first + count = %u + %u is more than %u", first, count, RM_PROGRESSIVE_MAX_SAMPLES);
        return ctx_fail(nullptr, RM_ERR_INVALID_ARG, buf);
    }
    if (count == 0u) return RM_OK;
    if (!table) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_lens_sequence: NULL table");
    for (uint32_t k = 0; k < count; k++) {
        const uint32_t s = first + k;
        const double a = 2. * radical_inverse(s, 5u) - 1.;
        const double b = 2. * radical_inverse(s, 7u) - 1.;
        double *r = table + 4u * (size_t)k;
        r[0] = radical_inverse(s, 2u);
        r[1] = radical_inverse(s, 3u);
        r[2] = a * std::sqrt(1. - b * b / 2.);
        r[3] = b * std::sqrt(1. - a * a / 2.);
    }
    return RM_OK;
}

rm_status rm_accumulate_lens_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const void *device_table, uint32_t n_before,
                                    void *device_sum, void *device_mean, void *device_rgb8, void *hip_stream) {
    return guarded(ctx, "rm_accumulate_lens_device", [&]() {
        return rm_accumulate_lens_device_impl(ctx, params, lens, device_table, n_before, device_sum, device_mean, device_rgb8, hip_stream);
    });
}

rm_status rm_render_progressive(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, int restart, double *host_rgb, uint8_t *host_rgb8,
                                uint32_t *n_total, rm_timing *timing) {
    return guarded(ctx, "rm_render_progressive",
                   [&]() { return rm_render_progressive_impl(ctx, "rm_render_progressive", params, lens, false, nullptr, 0u, restart, host_rgb, host_rgb8, n_total, timing); });
}

}  // extern "C"
