// rm_converge_host.inc -- host side of the converging frames (include/rusty_marcher_amd.h, "converging frames"); included at the
// end of rm_device.hip, behind rm_soft_host.inc whose checks (check_accum_device, check_soft_lights, check_soft_radii) and
// rm_accum_host.inc whose key (rm_progressive_key) it shares, and rm_refine_host.inc whose workspace size.  The kernels are
// rm_converge.hip's; rm_converge_motion_host.inc behind this file adds the moving spheres (the kernel of rm_converge_motion.hip)
// to both entry points' machinery: launch_converge_with and rm_render_converging_impl serve both.
//
// rm_accumulate_converging_device touches no render state and keeps all of its own in the caller's buffers: a memset of the
// list's length, the select launch, the shade launch, all on the caller's stream, nothing waited for.  rm_render_converging is
// that on the context's stream with buffers, a resident prefix of both sequences, a pass total and a key of its own
// (rm_ctx::converging) -- nothing of rm_render_progressive's.  rm_render_converging_motion is the same tick on the same state with
// a third resident prefix, the shape offsets, and the velocities and the shutter in the key.

// What both entry points check of rm_converge (ctx is not NULL); table_rows: what the table holds
static rm_status check_converge(rm_ctx *ctx, const char *who, const rm_lens *lens, const rm_converge *c, uint64_t table_rows) {
    if (!c) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL converge");
    if (std::isnan(c->tolerance)) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": converge.tolerance is NaN");
    const uint64_t most = std::min<uint64_t>(table_rows, RM_PROGRESSIVE_MAX_SAMPLES);
    if (c->max_samples < lens->n_samples || c->max_samples > most) {
        char buf[192];
        std::snprintf(buf, sizeof buf, "%s: converge.max_samples = %u is outside n_samples..min(table_rows, %u) = %u..%llu", who, c->max_samples,
                      RM_PROGRESSIVE_MAX_SAMPLES, lens->n_samples, (unsigned long long)most);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    return RM_OK;
}

// The converging block of a launch; everything was checked, table_rows >= n_samples.  offsets: NULL for the lights where the
// scene image says.
static ConvergeArgs converge_args(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c, const void *table,
                                  uint32_t table_rows, const void *offsets, int fresh, const rm_converge_frame *b) {
    ConvergeArgs a{};
    a.L = lens_args(ctx, p, lens, table, nullptr);
    a.tolerance = c->tolerance;
    a.min_samples = c->min_samples;
    a.max_samples = c->max_samples;
    a.fresh = fresh ? 1u : 0u;
    a.last_first = table_rows - lens->n_samples;
    a.sum = static_cast<double *>(b->sum);
    a.stats = static_cast<double *>(b->stats);
    a.count = static_cast<uint32_t *>(b->count);
    a.ws = static_cast<uint32_t *>(b->workspace);
    a.mean = static_cast<double *>(b->mean);
    a.rgb8 = static_cast<uint8_t *>(b->rgb8);
    a.mask = static_cast<uint8_t *>(b->mask);
    a.offsets = static_cast<const double *>(offsets);
    return a;
}

// The three steps on `stream`: the memset of the list's length and the select launch over `a`, then family `f`'s shade kernel
// over `block` -- the argument block `a` is, or is part of.  rows > 0 and no listed pixel's slice ends behind table_rows.
template <class ARGS>
static rm_status launch_converge_with(rm_ctx *ctx, const shade_family &f, ARGS &block, ConvergeArgs &a, hipStream_t stream) {
    auto select = [&]() -> rm_status {
        const uint32_t total = a.L.rows * a.L.frame_width;
        RM_HIP(ctx, hipMemsetAsync(a.ws, 0, sizeof(uint32_t), stream));
        void *select_args[] = {(void *)&a};
        RM_HIP(ctx, hipLaunchKernel(rm_converge_select_kernel(), dim3((total + RM_CONVERGE_SELECT_LANES - 1u) / RM_CONVERGE_SELECT_LANES),
                                    dim3(RM_CONVERGE_SELECT_LANES), select_args, 0, stream));
        return RM_OK;
    };
    return launch_shading(ctx, f, a.L.max_depth, lens_extent(ctx, a.L), block, stream, select);
}

static rm_status launch_converge(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c, const void *table,
                                 uint32_t table_rows, const void *offsets, int fresh, const rm_converge_frame *b, hipStream_t stream) {
    ConvergeArgs a = converge_args(ctx, p, lens, c, table, table_rows, offsets, fresh, b);
    // the two families: lights where the scene image says, and lights moved by the sample's row of `offsets`
    const shade_family stored{"converging", [](bool bvh, int pow_mode, int stack) { return rm_converge_shade_kernel(bvh, pow_mode, stack, false); }};
    const shade_family moved{"converging", [](bool bvh, int pow_mode, int stack) { return rm_converge_shade_kernel(bvh, pow_mode, stack, true); }};
    return launch_converge_with(ctx, offsets ? moved : stored, a, a, stream);
}

static rm_status rm_accumulate_converging_device_impl(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c,
                                                      const void *device_table, uint32_t table_rows, const void *device_offsets,
                                                      uint32_t n_lights, int fresh, const rm_converge_frame *b, void *hip_stream) {
    const char *who = "rm_accumulate_converging_device";
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
    if (!b) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL buffers");
    if (rm_status cst = check_accum_device(ctx, who, p, lens, device_table, 0u, b->sum, b->mean)) return cst;
    if (device_offsets)
        if (rm_status lst = check_soft_lights(ctx, who, n_lights)) return lst;
    if (rm_status vst = check_converge(ctx, who, lens, c, table_rows)) return vst;
    if (!b->stats) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL stats");
    if (!b->count) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL count");
    if (!b->workspace) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL workspace");
    if (refine_rows(p) == 0u) return RM_OK;
    RM_HIP(ctx, hipSetDevice(ctx->device));
    // (a scene without lights never fetches an offset: the kernel with stored lights)
    return launch_converge(ctx, p, lens, c, device_table, table_rows, ctx->image.H.n_lights > 0u ? device_offsets : nullptr, fresh, b,
                           (hipStream_t)hip_stream);
}

// The converging state of a context (rm_ctx::converging; made on the first call, released by rm_destroy)
struct rm_converging {
    void *d_table = nullptr, *d_offsets = nullptr;   // the resident prefix of rm_lens_sequence and of rm_light_sequence
    void *d_shape_offsets = nullptr;                 // ... and of rm_motion_sequence (rm_render_converging_motion's frames)
    uint32_t table_room = 0, table_rows = 0;         // rows d_table has room for / holds
    uint32_t offsets_room = 0, offsets_rows = 0;     // the same of d_offsets, in rows of offsets_lights x 3 doubles
    uint32_t offsets_lights = 0;
    bool offsets_zero = false;                       // d_offsets holds zeros: a motion tick's point lights (else rm_light_sequence of `radii`)
    uint32_t shape_room = 0, shape_rows = 0;         // the same of d_shape_offsets, in rows of shape_count x 3 doubles
    uint32_t shape_count = 0;
    std::vector<rm_vec3> velocities;                 // beside the key; empty: rm_render_converging's frames
    void *d_sum = nullptr, *d_stats = nullptr, *d_count = nullptr, *d_ws = nullptr, *d_mean = nullptr, *d_rgb8 = nullptr;
    size_t pixels = 0;                               // the six buffers have room for that many
    bool have_key = false;                           // a call has succeeded, and nothing failed half-way since
    rm_progressive_key key;
    std::vector<double> radii;                       // beside the key; empty: point lights
    std::vector<double> staging;                     // the rows a call appends, host side
    uint32_t n = 0;                                  // the pass total N: no pixel's count exceeds it (a bound, reached by the pixels sampled in every pass)
    uint32_t passes = 0, listed = 0;                 // passes launched; pixels the last of them listed
    uint64_t cast = 0;                               // samples cast over the frame's life
    rm_converge last{};                              // what the last pass ran with
    uint32_t last_ns = 0;
};

static void converging_destroy(rm_ctx *ctx, bool device_ok) {
    rm_converging *g = ctx->converging;
    if (!g) return;
    for (void *b : {g->d_table, g->d_offsets, g->d_shape_offsets, g->d_sum, g->d_stats, g->d_count, g->d_ws, g->d_mean, g->d_rgb8})
        if (b && device_ok) (void)hipFree(b);
    delete g;
    ctx->converging = nullptr;
}

// Makes *d hold rows [0, need) of a sequence of `row_doubles` doubles a row: what it holds stays (copied on the device where the
// buffer has to grow), rows [*have, need) are computed by fill(first, count, out) and appended on the context's stream.
template <class FILL>
static rm_status converging_extend(rm_ctx *ctx, rm_converging &g, void **d, uint32_t *room, uint32_t *have, uint32_t need, size_t row_doubles,
                                   FILL fill) {
    if (need <= *have) return RM_OK;
    const size_t row_bytes = row_doubles * sizeof(double);
    if (need > *room) {
        const uint32_t grown = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(need, 2ull * *room), RM_PROGRESSIVE_MAX_SAMPLES);
        void *fresh = nullptr;
        RM_HIP(ctx, hipMalloc(&fresh, (size_t)grown * row_bytes));
        if (*d) {
            hipError_t e = *have > 0u ? hipMemcpyAsync(fresh, *d, (size_t)*have * row_bytes, hipMemcpyDeviceToDevice, ctx->stream) : hipSuccess;
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);     // (the old buffer is freed below)
            if (e != hipSuccess) {
                (void)hipFree(fresh);
                return ctx_fail(ctx, RM_ERR_HIP, std::string("converging: growing a sequence: ") + hipGetErrorString(e));
            }
            RM_HIP(ctx, hipFree(*d));
        }
        *d = fresh;
        *room = grown;
    }
    const uint32_t first = *have, count = need - first;
    g.staging.resize((size_t)count * row_doubles);
    if (rm_status sst = fill(first, count, g.staging.data())) return sst;
    RM_HIP(ctx, hipMemcpyAsync(static_cast<char *>(*d) + (size_t)first * row_bytes, g.staging.data(), (size_t)count * row_bytes,
                               hipMemcpyHostToDevice, ctx->stream));
    RM_HIP(ctx, hipStreamSynchronize(ctx->stream));                        // (staging is reused by the next append)
    *have = need;
    return RM_OK;
}

// rm_converge_motion_host.inc: the launch with both offset tables
static rm_status launch_converge_motion(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c, const void *table,
                                        uint32_t table_rows, const void *offsets, const void *shape_offsets, int fresh,
                                        const rm_converge_frame *b, hipStream_t stream);

// `motion`: rm_render_converging_motion's tick -- the velocities and the shutter (checked here), a resident prefix of
// rm_motion_sequence beside the other two, light offsets for every light of the scene (zeros where there are no radii) and the
// kernel of rm_converge_motion.hip; else NULL and everything as it was before there were moving spheres.
static rm_status rm_render_converging_impl(rm_ctx *ctx, const char *who, const rm_params *p, const rm_lens *lens, const rm_converge *c,
                                           const double *radii, uint32_t n_lights, int restart, double *host_rgb, uint8_t *host_rgb8,
                                           rm_converge_report *report, rm_timing *timing, const rm_motion_tick *motion = nullptr) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
    const auto t_begin = std::chrono::steady_clock::now();
    if (rm_status cst = check_accum(ctx, who, p, lens)) return cst;
    const bool soft = radii != nullptr;
    if (!soft) n_lights = 0u;                                              // point lights: no radii, whatever the count says
    if (soft)
        if (rm_status rst = check_soft_radii(ctx, who, radii, n_lights)) return rst;
    if (motion)
        if (rm_status mst = check_motion_tick(ctx, who, *motion)) return mst;
    if (rm_status vst = check_converge(ctx, who, lens, c, RM_PROGRESSIVE_MAX_SAMPLES)) return vst;
    const uint32_t n_shapes = motion ? motion->n_shapes : 0u;
    const uint32_t rows = refine_rows(p), ns = lens->n_samples;
    double kernel_ms = 0., d2h_ms = 0.;
    rm_converge_report rep{};
    if (rows > 0u) {
        if (!ctx->converging) ctx->converging = new rm_converging();
        rm_converging &g = *ctx->converging;
        const rm_progressive_key key = progressive_key_of(ctx, p, lens, soft, n_lights, motion);
        const bool same = !restart && g.have_key && std::memcmp(&key, &g.key, sizeof key) == 0 && g.radii.size() == n_lights &&
                          (n_lights == 0u || std::memcmp(g.radii.data(), radii, n_lights * sizeof(double)) == 0) &&
                          g.velocities.size() == n_shapes &&
                          (n_shapes == 0u || std::memcmp(g.velocities.data(), motion->velocities, n_shapes * sizeof(rm_vec3)) == 0);
        // (a motion tick's kernel reads a row for every light of the scene: zeros where the lights are points)
        const uint32_t staged_lights = motion ? ctx->image.H.n_lights : n_lights;
        const bool zeros = motion && !soft;
        // ... and a row for every shape, where the scene has a sphere to move
        const uint32_t staged_shapes = motion && ctx->image.H.n_spheres > 0u ? n_shapes : 0u;
        // a finished picture: the pass before this one, with the same rule, listed nothing -- so would this one
        const bool finished = same && g.passes > 0u && g.listed == 0u && g.last_ns == ns && std::memcmp(&g.last, c, sizeof *c) == 0;
        const size_t pixels = (size_t)rows * p->frame_width;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        if (!finished) {
            g.have_key = false;                                            // (until this call is through)
            if (!same) {
                g.n = 0u; g.passes = 0u; g.listed = 0u; g.cast = 0u;
                if (g.offsets_lights != staged_lights || g.offsets_zero != zeros ||
                    (!zeros && (g.radii.size() != n_lights || (n_lights > 0u && std::memcmp(g.radii.data(), radii, n_lights * sizeof(double)) != 0))))
                    g.offsets_rows = 0u;                                   // another sequence (the lens sequence is the same for every frame)
                if (g.offsets_lights != staged_lights) {
                    if (g.d_offsets) RM_HIP(ctx, hipFree(g.d_offsets));
                    g.d_offsets = nullptr;
                    g.offsets_room = 0u;
                    g.offsets_lights = staged_lights;
                }
                g.offsets_zero = zeros;
                g.radii.assign(radii, radii + n_lights);                   // (n_lights == 0: empty, radii is NULL)
                // the shape offsets are a function of the velocities and the shutter: whatever began the frame again, they go
                g.shape_rows = 0u;
                if (g.shape_count != staged_shapes) {
                    if (g.d_shape_offsets) RM_HIP(ctx, hipFree(g.d_shape_offsets));
                    g.d_shape_offsets = nullptr;
                    g.shape_room = 0u;
                    g.shape_count = staged_shapes;
                }
                if (motion) g.velocities.assign(motion->velocities, motion->velocities + n_shapes);
                else g.velocities.clear();
            }
            if (g.pixels < pixels) {
                g.pixels = 0;
                const std::pair<void **, size_t> buffers[] = {
                    {&g.d_sum, pixels * 3u * sizeof(double)}, {&g.d_stats, pixels * 2u * sizeof(double)}, {&g.d_count, pixels * sizeof(uint32_t)},
                    {&g.d_ws, (4u * (1u + pixels) + 255u) & ~(size_t)255u}, {&g.d_mean, pixels * 3u * sizeof(double)}, {&g.d_rgb8, pixels * 3u}};
                for (const auto &b : buffers) {
                    size_t none = 0;                                       // (every one is replaced: they share one size)
                    if (rm_status gst = grow_device_buffer(ctx, b.first, &none, b.second)) return gst;
                }
                g.pixels = pixels;
            }
            // no count exceeds N and no slice ends behind max_samples: rows [0, min(N + ns, max_samples)) serve this pass
            const uint32_t need = (uint32_t)std::max<uint64_t>(std::min<uint64_t>((uint64_t)g.n + ns, c->max_samples), ns);
            if (rm_status est = converging_extend(ctx, g, &g.d_table, &g.table_room, &g.table_rows, need, 4u, rm_lens_sequence)) return est;
            const bool offsets = (soft || motion) && staged_lights > 0u;
            if (offsets) {
                const double *rr = g.radii.data();
                auto fill = [=](uint32_t first, uint32_t count, double *out) -> rm_status {
                    if (!zeros) return rm_light_sequence(first, count, rr, n_lights, out);
                    std::fill(out, out + (size_t)count * staged_lights * 3u, 0.);
                    return RM_OK;
                };
                if (rm_status est = converging_extend(ctx, g, &g.d_offsets, &g.offsets_room, &g.offsets_rows, need, (size_t)staged_lights * 3u, fill))
                    return est;
            }
            const bool shapes = staged_shapes > 0u;
            if (shapes) {
                const rm_vec3 *vv = g.velocities.data();
                const double shutter = motion->shutter;
                auto fill = [=](uint32_t first, uint32_t count, double *out) { return rm_motion_sequence(first, count, vv, n_shapes, shutter, out); };
                if (rm_status est = converging_extend(ctx, g, &g.d_shape_offsets, &g.shape_room, &g.shape_rows, need, (size_t)n_shapes * 3u, fill))
                    return est;
            }
            const rm_converge_frame b{g.d_sum, g.d_stats, g.d_count, g.d_ws, g.d_mean, g.d_rgb8, nullptr};
            // (the kernel is told what is resident -- at least `need` rows of every sequence -- so its clamp guards the buffers' end)
            uint32_t resident = g.table_rows;
            if (offsets) resident = std::min(resident, g.offsets_rows);
            if (shapes) resident = std::min(resident, g.shape_rows);
            auto launch = [&]() {
                if (motion)
                    return launch_converge_motion(ctx, p, lens, c, g.d_table, resident, offsets ? g.d_offsets : nullptr,
                                                  shapes ? g.d_shape_offsets : nullptr, g.n == 0u, &b, ctx->stream);
                return launch_converge(ctx, p, lens, c, g.d_table, resident, offsets ? g.d_offsets : nullptr, g.n == 0u, &b, ctx->stream);
            };
            if (rm_status lst = timed_launch(ctx, &kernel_ms, launch)) return lst;
            uint32_t listed = 0;
            RM_HIP(ctx, hipMemcpy(&listed, g.d_ws, sizeof listed, hipMemcpyDeviceToHost));
            g.key = key;
            g.listed = listed;
            g.passes += 1u;
            g.cast += (uint64_t)listed * ns;
            // N stays a bound on every count whatever n_samples and the cap were from tick to tick: a sampled pixel had c <= N and
            // c + ns <= max_samples, so it holds at most min(N + ns, max_samples); a pass that sampled nothing raised no count
            if (listed > 0u) g.n = std::max<uint32_t>(g.n, (uint32_t)std::min<uint64_t>((uint64_t)g.n + ns, c->max_samples));
            g.last = *c;
            g.last_ns = ns;
            g.have_key = true;
        }
        rep.listed = finished ? 0u : g.listed;
        rep.passes = g.passes;
        rep.max_count = g.n;
        rep.samples_cast = g.cast;
        const auto t0 = std::chrono::steady_clock::now();
        if (host_rgb) RM_HIP(ctx, hipMemcpy(host_rgb, g.d_mean, pixels * 3u * sizeof(double), hipMemcpyDeviceToHost));
        if (host_rgb8) RM_HIP(ctx, hipMemcpy(host_rgb8, g.d_rgb8, pixels * 3u, hipMemcpyDeviceToHost));
        d2h_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    if (report) *report = rep;
    fill_timing(timing, kernel_ms, d2h_ms, t_begin);
    return RM_OK;
}

extern "C" {

rm_status rm_converge_workspace(const rm_params *params, size_t *bytes) {
    if (!params || !bytes) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_converge_workspace: NULL argument");
    if (params->frame_width % RM_PATCH_SIZE != 0)
        return ctx_fail(nullptr, RM_ERR_DIMENSIONS, "rm_converge_workspace: frame width is not a multiple of 32");
    *bytes = refine_workspace_bytes(params);
    return RM_OK;
}

rm_status rm_accumulate_converging_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const rm_converge *converge,
                                          const void *device_table, uint32_t table_rows, const void *device_offsets, uint32_t n_lights,
                                          int fresh, const rm_converge_frame *buffers, void *hip_stream) {
    return guarded(ctx, "rm_accumulate_converging_device", [&]() {
        return rm_accumulate_converging_device_impl(ctx, params, lens, converge, device_table, table_rows, device_offsets, n_lights, fresh,
                                                    buffers, hip_stream);
    });
}

rm_status rm_render_converging(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const rm_converge *converge, const double *radii,
                               uint32_t n_lights, int restart, double *host_rgb, uint8_t *host_rgb8, rm_converge_report *report,
                               rm_timing *timing) {
    return guarded(ctx, "rm_render_converging", [&]() {
        return rm_render_converging_impl(ctx, "rm_render_converging", params, lens, converge, radii, n_lights, restart, host_rgb, host_rgb8, report, timing);
    });
}

}  // extern "C"
