// rm_converge_motion_host.inc -- host side of the converging frames with moving spheres (include/rusty_marcher_amd.h,
// "converging frames with moving spheres") and, behind both launches it can end in, the tick of the converging frames with and
// without them; included at the end of rm_device.hip, behind rm_converge_host.inc whose checks (check_converge,
// check_converge_call), argument block (converge_args) and launches (launch_converge_with, launch_converge) it uses, and
// rm_accum_host.inc whose checks (check_accum, check_offset_tables, check_rules).  The shade kernel is rm_converge_motion.hip's,
// the select kernel rm_converge.hip's.
//
// rm_accumulate_converging_motion_device touches no render state and keeps all of its own in the caller's buffers, as
// rm_accumulate_converging_device does.  rm_render_converging is a pass on the context's stream with buffers, a resident prefix
// of the lens and the light sequence, a pass total and a frame identity of its own (rm_ctx::converging) -- nothing of
// rm_render_progressive's.  rm_render_converging_motion is the same tick on the same state with a third resident prefix, the
// shape offsets, and the velocities and the shutter in the identity: which tables a tick keeps is rm_staging_of's rule.
// rm_render_converging_moving (rm_converge_moving_host.inc, behind this file) is the third: the motion tick with every shape
// free to move.

// The three steps on `stream`; everything was checked, rows > 0.  offsets: NULL where the scene has no lights; shape_offsets:
// NULL where it has no spheres.
static rm_status launch_converge_motion(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c, const void *table,
                                        uint32_t table_rows, const void *offsets, const void *shape_offsets, int fresh,
                                        const rm_converge_frame *b, hipStream_t stream) {
    ConvergeMotionArgs m{};
    m.C = converge_args(ctx, p, lens, c, table, table_rows, offsets, fresh, b);
    m.shape_offsets = static_cast<const double *>(shape_offsets);
    m.pid_map = ctx->d_pid_map;
    m.n_shapes = resident_shape_count(ctx);
    return launch_converge_with(ctx, shade_family{"converging with moving spheres", rm_converge_motion_kernel}, m, m.C, stream);
}

// The moving camera's three steps (rm_camera_host.inc, behind this file): launch_converge_moving's with the camera's rows;
// shape_offsets NULL: no shape moves
static rm_status launch_converge_camera(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c, const void *table,
                                        uint32_t table_rows, const void *offsets, const void *shape_offsets, const void *camera_rows, int fresh,
                                        const rm_converge_frame *b, hipStream_t stream);

// The moving spheres' three steps over the ticks' swept hierarchy where tick_swept_prepare made it ready (rm_swept_host.inc,
// behind this file) -- launch_converge_motion where not
static rm_status launch_converge_motion_tick(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c, const void *table,
                                             uint32_t table_rows, const void *offsets, const void *shape_offsets, int fresh,
                                             const rm_converge_frame *b, hipStream_t stream);

// The diffuse bounce's three steps (rm_bounce_host.inc, behind this file): launch_converge's with the bounce table and the strength
static rm_status launch_converge_bounce(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c, const void *table,
                                        uint32_t table_rows, const void *offsets, const void *bounce, double strength, int fresh,
                                        const rm_converge_frame *b, hipStream_t stream);

// The reprojection's launch into the tick's own buffers, mean and bytes included (rm_reproject_host.inc, behind this file)
static rm_status launch_reproject_tick(rm_ctx *ctx, const rm_params *p, const rm_reproject *r, const rm_view *v, const void *prev_sum,
                                       const void *prev_stats, const void *prev_count, const void *prev_hits, const void *cur_hits, void *out_sum,
                                       void *out_stats, void *out_count, void *carried_total, void *mean, void *rgb8, hipStream_t stream);

// A resident prefix of a sequence: rows [0, rows) of `columns` doubles each (the lens table: 4; an offset table: 3 a light or
// shape; the camera table: 12)
struct rm_resident_prefix {
    void *d = nullptr;
    uint32_t room = 0, rows = 0;             // rows d has room for / holds
    uint32_t columns = 0;
};

// The converging state of a context (rm_ctx::converging; made on the first call, released by rm_destroy)
struct rm_converging {
    rm_resident_prefix table{nullptr, 0u, 0u, 4u}, lights, shapes;   // of rm_lens_sequence, of rm_light_sequence (or zeros) and of rm_motion_sequence
    rm_resident_prefix camera;                       // ... and of rm_camera_sequence (the moving camera's tick)
    rm_resident_prefix bounce{nullptr, 0u, 0u, 2u};  // ... and of rm_bounce_sequence (the diffuse bounce's tick): the same rows for every frame
    bool lights_zero = false;                        // `lights` holds zeros: a motion tick's point lights (else rm_light_sequence of id.radii)
    void *d_sum = nullptr, *d_stats = nullptr, *d_count = nullptr, *d_ws = nullptr, *d_mean = nullptr, *d_rgb8 = nullptr;
    size_t pixels = 0;                               // the six buffers have room for that many
    bool have_key = false;                           // a call has succeeded, and nothing failed half-way since
    rm_frame_identity id;                            // the frame the buffers belong to
    std::vector<double> staging;                     // the rows a call appends, host side
    uint32_t n = 0;                                  // the pass total N: no pixel's count exceeds it (a bound, reached by the pixels sampled in every pass)
    uint32_t passes = 0, listed = 0;                 // passes launched; pixels the last of them listed
    uint64_t cast = 0;                               // samples cast over the frame's life
    rm_converge last{};                              // what the last pass ran with
    uint32_t last_ns = 0;
    // history (rm_converge_history; include/rusty_marcher_amd.h, "temporal reprojection").  Off: nothing below is allocated or
    // looked at.  On: rm_render_converging keeps the hits under the frame's pixels, and a second set of sum, stats and count it
    // reprojects into and then swaps with the first
    bool history = false;
    rm_reproject history_rule{};
    void *d_hits = nullptr, *d_hits_next = nullptr;  // rm_hit a pixel of the frame's view; of the view a reprojection moves to
    size_t hits_bytes = 0, hits_next_bytes = 0;
    bool have_hits = false;                          // d_hits holds the hits of the frame the buffers belong to
    void *d_sum_next = nullptr, *d_stats_next = nullptr, *d_count_next = nullptr, *d_carried_total = nullptr;
    size_t next_pixels = 0;                          // the second set has room for that many
    uint64_t reprojections = 0;                      // rm_history_report's four
    uint32_t last_reprojected = 0, carried = 0, without = 0;
};

// Whether two frames differ in nothing but the view: the camera's position, its basis and whether it is oriented
static bool same_frame_but_view(const rm_frame_identity &a, const rm_frame_identity &b) {
    rm_frame_identity c = a;
    c.key.camera = b.key.camera;
    c.key.basis = b.key.basis;
    c.key.oriented = b.key.oriented;
    return rm_same_frame(c, b);
}

// Turning the history off releases what it alone uses; the report's counters stay
static rm_status converging_drop_history(rm_ctx *ctx, rm_converging &g) {
    for (void **b : {&g.d_hits, &g.d_hits_next, &g.d_sum_next, &g.d_stats_next, &g.d_count_next, &g.d_carried_total}) {
        if (*b) RM_HIP(ctx, hipFree(*b));
        *b = nullptr;
    }
    g.hits_bytes = g.hits_next_bytes = 0;
    g.next_pixels = 0;
    g.have_hits = false;
    return RM_OK;
}

static void converging_destroy(rm_ctx *ctx, bool device_ok) {
    rm_converging *g = ctx->converging;
    if (!g) return;
    for (void *b : {g->table.d, g->lights.d, g->shapes.d, g->camera.d, g->bounce.d, g->d_sum, g->d_stats, g->d_count, g->d_ws, g->d_mean, g->d_rgb8,
                    g->d_hits, g->d_hits_next, g->d_sum_next, g->d_stats_next, g->d_count_next, g->d_carried_total})
        if (b && device_ok) (void)hipFree(b);
    delete g;
    ctx->converging = nullptr;
}

// A prefix whose rows change their length holds nothing, and its buffer goes
static rm_status converging_recolumn(rm_ctx *ctx, rm_resident_prefix &s, uint32_t columns) {
    if (s.columns == columns) return RM_OK;
    if (s.d) RM_HIP(ctx, hipFree(s.d));
    s.d = nullptr;
    s.room = s.rows = 0u;
    s.columns = columns;
    return RM_OK;
}

// Makes the prefix hold rows [0, need): what it holds stays (copied on the device where the buffer has to grow), rows
// [s.rows, need) are computed by fill(first, count, out) and appended on the context's stream.
template <class FILL>
static rm_status converging_extend(rm_ctx *ctx, rm_converging &g, rm_resident_prefix &s, uint32_t need, FILL fill) {
    if (need <= s.rows) return RM_OK;
    const size_t row_bytes = (size_t)s.columns * sizeof(double);
    if (need > s.room) {
        const uint32_t grown = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(need, 2ull * s.room), RM_PROGRESSIVE_MAX_SAMPLES);
        void *fresh = nullptr;
        RM_HIP(ctx, hipMalloc(&fresh, (size_t)grown * row_bytes));
        if (s.d) {
            hipError_t e = s.rows > 0u ? hipMemcpyAsync(fresh, s.d, (size_t)s.rows * row_bytes, hipMemcpyDeviceToDevice, ctx->stream) : hipSuccess;
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);     // (the old buffer is freed below)
            if (e != hipSuccess) {
                (void)hipFree(fresh);
                return ctx_fail(ctx, RM_ERR_HIP, std::string("converging: growing a sequence: ") + hipGetErrorString(e));
            }
            RM_HIP(ctx, hipFree(s.d));
        }
        s.d = fresh;
        s.room = grown;
    }
    const uint32_t first = s.rows, count = need - first;
    g.staging.resize((size_t)count * s.columns);
    if (rm_status sst = fill(first, count, g.staging.data())) return sst;
    RM_HIP(ctx, hipMemcpyAsync(static_cast<char *>(s.d) + (size_t)first * row_bytes, g.staging.data(), (size_t)count * row_bytes,
                               hipMemcpyHostToDevice, ctx->stream));
    RM_HIP(ctx, hipStreamSynchronize(ctx->stream));                        // (staging is reused by the next append)
    s.rows = need;
    return RM_OK;
}

// A launch with launch_converge_motion's arguments: the moving shapes' tick (rm_converge_moving_host.inc) hands the tick below its own
using converge_motion_launch = rm_status (*)(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c, const void *table,
                                             uint32_t table_rows, const void *offsets, const void *shape_offsets, int fresh,
                                             const rm_converge_frame *b, hipStream_t stream);

// The tick of the five calls; `rules` says which (rules.bounce: the diffuse bounce's, rm_bounce_host.inc, which keeps a prefix of
// rm_bounce_sequence as well and launches its own shade kernel; its frames begin again on a camera move, history or not;
// rules.camera: the moving camera's, rm_camera_host.inc, which keeps a prefix of rm_camera_sequence as well and launches its own kernels), and `any_shape`, the moving shapes' launch, tells their tick (a motion tick in
// which a velocity on any shape is obeyed and a shape table is kept whenever the scene holds a shape; key.motion = 2 keeps its
// frames apart from the moving spheres') from the moving spheres': checked here, the prefixes they ask for kept resident, the
// launch by them.
static rm_status rm_render_converging_impl(rm_ctx *ctx, const char *who, const rm_params *p, const rm_lens *lens, const rm_converge *c,
                                           const rm_sampling_rules &rules, int restart, double *host_rgb, uint8_t *host_rgb8,
                                           rm_converge_report *report, rm_timing *timing, converge_motion_launch any_shape = nullptr) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
    ctx->swept_walked = 0u;                                                // (until a launch of this tick walks a swept hierarchy)
    const auto t_begin = std::chrono::steady_clock::now();
    if (rm_status cst = check_accum(ctx, who, p, lens)) return cst;
    if (rm_status rst = check_rules(ctx, who, rules, any_shape != nullptr)) return rst;
    if (rm_status vst = check_converge(ctx, who, lens, c, RM_PROGRESSIVE_MAX_SAMPLES)) return vst;
    const uint32_t rows = refine_rows(p), ns = lens->n_samples;
    const size_t pixels = (size_t)rows * p->frame_width;
    double kernel_ms = 0.;
    rm_converge_report rep{};
    if (rows > 0u) {
        if (!ctx->converging) ctx->converging = new rm_converging();
        rm_converging &g = *ctx->converging;
        rm_frame_identity id = rm_frame_identity_of(*p, *lens, ctx->camera, ctx->basis, ctx->oriented, ctx->upload_copies, rules);
        if (any_shape) id.key.motion = 2u;
        const bool same = !restart && g.have_key && rm_same_frame(g.id, id);
        // history: rm_render_converging's alone.  A frame that differs from the kept one in the view only is carried over
        const bool keeps_hits = g.history && !rules.motion && !rules.camera && !rules.bounce && !any_shape;
        const bool reproject = keeps_hits && !same && !restart && g.have_key && g.passes > 0u && g.have_hits && same_frame_but_view(g.id, id);
        const size_t hit_bytes = (size_t)p->frame_height * p->frame_width * sizeof(rm_hit);
        const rm_staging staged = rm_staging_of(any_shape ? RM_TICK_CONVERGING_MOVING : RM_TICK_CONVERGING, rules, ctx->image.H.n_lights,
                                                ctx->image.H.n_spheres, resident_shape_count(ctx));
        // a finished picture: the pass before this one, with the same rule, listed nothing -- so would this one
        const bool finished = same && g.passes > 0u && g.listed == 0u && g.last_ns == ns && std::memcmp(&g.last, c, sizeof *c) == 0;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        if (finished && keeps_hits && !g.have_hits) {
            // the continuing frame has no hit buffer yet (history was turned on since it began): this tick fills it
            g.have_key = false;
            if (rm_status gst = grow_device_buffer(ctx, &g.d_hits, &g.hits_bytes, hit_bytes)) return gst;
            if (rm_status lst = timed_launch(ctx, &kernel_ms, [&]() { return rm_primary_hits_device_impl(ctx, p, g.d_hits, ctx->stream); })) return lst;
            g.have_hits = true;
            g.have_key = true;
        }
        if (!finished) {
            g.have_key = false;                                            // (until this call is through)
            rm_view previous_view{};
            if (reproject) {
                // the kept sums move to the new view: the pass total is held to max_history as every carried count is
                previous_view.position = g.id.key.camera;
                previous_view.basis = g.id.key.basis;
                g.n = std::min<uint32_t>(g.n, g.history_rule.max_history);
                g.passes = 0u; g.listed = 0u; g.cast = 0u;
                g.id = std::move(id);
            } else if (!same) {
                g.have_hits = false;
                g.n = 0u; g.passes = 0u; g.listed = 0u; g.cast = 0u;
                // the light rows stay where they are the same sequence (the lens sequence is the same for every frame); the shape
                // rows are a function of the velocities and the shutter: whatever began the frame again, they go
                const bool lights_stay = g.lights_zero == staged.light_zeros && (staged.light_zeros || rm_same_radii(g.id, id));
                if (!lights_stay) g.lights.rows = 0u;
                g.shapes.rows = 0u;
                g.camera.rows = 0u;                                        // (a function of the motion, the shutter and the basis)
                if (rm_status rst = converging_recolumn(ctx, g.camera, rules.camera ? 12u : 0u)) return rst;
                if (rm_status rst = converging_recolumn(ctx, g.lights, staged.light_columns * 3u)) return rst;
                if (rm_status rst = converging_recolumn(ctx, g.shapes, staged.shape_columns * 3u)) return rst;
                g.lights_zero = staged.light_zeros;
                g.id = std::move(id);
            }
            if (rm_status gst = grow_frame_buffers(
                    ctx, &g.pixels, pixels,
                    {{&g.d_sum, pixels * 3u * sizeof(double)}, {&g.d_stats, pixels * 2u * sizeof(double)}, {&g.d_count, pixels * sizeof(uint32_t)},
                     {&g.d_ws, (4u * (1u + pixels) + 255u) & ~(size_t)255u}, {&g.d_mean, pixels * 3u * sizeof(double)}, {&g.d_rgb8, pixels * 3u}}))
                return gst;
            // no count exceeds N and no slice ends behind max_samples: rows [0, min(N + ns, max_samples)) serve this pass
            const uint32_t need = (uint32_t)std::max<uint64_t>(std::min<uint64_t>((uint64_t)g.n + ns, c->max_samples), ns);
            if (rm_status est = converging_extend(ctx, g, g.table, need, rm_fill_lens_rows)) return est;
            const bool offsets = staged.light_columns > 0u, shapes = staged.shape_columns > 0u;
            if (offsets)
                if (rm_status est = converging_extend(ctx, g, g.lights, need, [&](uint32_t first, uint32_t count, double *out) {
                        return rm_fill_light_rows(rules, staged, first, count, out);
                    }))
                    return est;
            if (shapes)
                if (rm_status est = converging_extend(ctx, g, g.shapes, need, [&](uint32_t first, uint32_t count, double *out) {
                        return rm_fill_shape_rows(rules, first, count, out);
                    }))
                    return est;
            if (rules.camera) {
                const rm_camera_basis basis = reported_basis(ctx);
                if (rm_status est = converging_extend(ctx, g, g.camera, need, [&](uint32_t first, uint32_t count, double *out) {
                        return host_refusal(ctx, rm_camera_sequence(first, count, rules.camera, &basis, rules.shutter, out));
                    }))
                    return est;
            }
            if (rules.bounce)
                if (rm_status est = converging_extend(ctx, g, g.bounce, need, rm_fill_bounce_rows)) return est;
            const bool fill_hits = keeps_hits && !reproject && !g.have_hits;
            if (fill_hits || reproject)
                if (rm_status gst = grow_device_buffer(ctx, &g.d_hits, &g.hits_bytes, hit_bytes)) return gst;
            if (reproject) {
                if (rm_status gst = grow_device_buffer(ctx, &g.d_hits_next, &g.hits_next_bytes, hit_bytes)) return gst;
                if (rm_status gst = grow_frame_buffers(ctx, &g.next_pixels, pixels,
                                                       {{&g.d_sum_next, pixels * 3u * sizeof(double)}, {&g.d_stats_next, pixels * 2u * sizeof(double)},
                                                        {&g.d_count_next, pixels * sizeof(uint32_t)}}))
                    return gst;
                size_t word = g.d_carried_total ? 256u : 0u;
                if (rm_status gst = grow_device_buffer(ctx, &g.d_carried_total, &word, 256u)) return gst;
                g.have_hits = false;                                       // (until the swap below is through)
            }
            const rm_converge_frame b{reproject ? g.d_sum_next : g.d_sum, reproject ? g.d_stats_next : g.d_stats, reproject ? g.d_count_next : g.d_count,
                                      g.d_ws, g.d_mean, g.d_rgb8, nullptr};
            const int fresh = !reproject && g.n == 0u;
            // (the kernel is told what is resident -- at least `need` rows of every sequence -- so its clamp guards the buffers' end)
            uint32_t resident = g.table.rows;
            if (offsets) resident = std::min(resident, g.lights.rows);
            if (shapes) resident = std::min(resident, g.shapes.rows);
            if (rules.camera) resident = std::min(resident, g.camera.rows);
            if (rules.bounce) resident = std::min(resident, g.bounce.rows);
            auto launch = [&]() -> rm_status {
                if (fill_hits)
                    if (rm_status hst = rm_primary_hits_device_impl(ctx, p, g.d_hits, ctx->stream)) return hst;
                if (reproject) {
                    if (rm_status hst = rm_primary_hits_device_impl(ctx, p, g.d_hits_next, ctx->stream)) return hst;
                    if (rm_status rst = launch_reproject_tick(ctx, p, &g.history_rule, &previous_view, g.d_sum, g.d_stats, g.d_count, g.d_hits,
                                                              g.d_hits_next, g.d_sum_next, g.d_stats_next, g.d_count_next, g.d_carried_total,
                                                              g.d_mean, g.d_rgb8, ctx->stream))
                        return rst;
                }
                if (rules.camera)
                    return launch_converge_camera(ctx, p, lens, c, g.table.d, resident, offsets ? g.lights.d : nullptr, shapes ? g.shapes.d : nullptr,
                                                  g.camera.d, fresh, &b, ctx->stream);
                if (any_shape)
                    return any_shape(ctx, p, lens, c, g.table.d, resident, offsets ? g.lights.d : nullptr, shapes ? g.shapes.d : nullptr,
                                     fresh, &b, ctx->stream);
                if (rules.motion)
                    return launch_converge_motion_tick(ctx, p, lens, c, g.table.d, resident, offsets ? g.lights.d : nullptr,
                                                       shapes ? g.shapes.d : nullptr, fresh, &b, ctx->stream);
                if (rules.bounce)
                    return launch_converge_bounce(ctx, p, lens, c, g.table.d, resident, offsets ? g.lights.d : nullptr, g.bounce.d, rules.strength,
                                                  fresh, &b, ctx->stream);
                return launch_converge(ctx, p, lens, c, g.table.d, resident, offsets ? g.lights.d : nullptr, fresh, &b, ctx->stream);
            };
            if (rm_status lst = timed_launch(ctx, &kernel_ms, launch)) return lst;
            if (fill_hits) g.have_hits = true;
            if (reproject) {
                uint32_t carried = 0;
                RM_HIP(ctx, hipMemcpy(&carried, g.d_carried_total, sizeof carried, hipMemcpyDeviceToHost));
                std::swap(g.d_sum, g.d_sum_next);
                std::swap(g.d_stats, g.d_stats_next);
                std::swap(g.d_count, g.d_count_next);
                std::swap(g.d_hits, g.d_hits_next);
                std::swap(g.hits_bytes, g.hits_next_bytes);
                g.pixels = g.next_pixels = std::min(g.pixels, g.next_pixels);   // (the room of either set, now that they are mixed)
                g.have_hits = true;
                g.reprojections += 1u;
                g.carried = carried;
                g.without = (uint32_t)pixels - carried;
            }
            uint32_t listed = 0;
            RM_HIP(ctx, hipMemcpy(&listed, g.d_ws, sizeof listed, hipMemcpyDeviceToHost));
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
        if (!rules.motion && !rules.camera && !rules.bounce && !any_shape) g.last_reprojected = reproject ? 1u : 0u;   // (rm_render_converging's own)
        rep.listed = finished ? 0u : g.listed;
        rep.passes = g.passes;
        rep.max_count = g.n;
        rep.samples_cast = g.cast;
    }
    const rm_converging *g = rows > 0u ? ctx->converging : nullptr;
    if (rm_status fst = finish_tick(ctx, pixels, g ? g->d_mean : nullptr, g ? g->d_rgb8 : nullptr, host_rgb, host_rgb8, kernel_ms, timing, t_begin))
        return fst;
    if (report) *report = rep;
    return RM_OK;
}

extern "C" {

rm_status rm_accumulate_converging_motion_device(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c,
                                                 const void *device_table, uint32_t table_rows, const void *device_light_offsets,
                                                 uint32_t n_lights, const void *device_shape_offsets, uint32_t n_shapes, int fresh,
                                                 const rm_converge_frame *b, void *hip_stream) {
    const char *who = "rm_accumulate_converging_motion_device";
    return guarded(ctx, who, [&]() -> rm_status {
        if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
        const shape_table shapes{device_shape_offsets, n_shapes};
        auto tables = [&]() { return check_offset_tables(ctx, who, "light offsets", device_light_offsets, n_lights, &shapes); };
        if (rm_status cst = check_converge_call(ctx, who, p, lens, c, device_table, table_rows, b, tables)) return cst;
        if (refine_rows(p) == 0u) return RM_OK;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        return launch_converge_motion(ctx, p, lens, c, device_table, table_rows, n_lights > 0u ? device_light_offsets : nullptr,
                                      ctx->image.H.n_spheres > 0u ? device_shape_offsets : nullptr, fresh, b, (hipStream_t)hip_stream);
    });
}

rm_status rm_render_converging(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const rm_converge *converge, const double *radii,
                               uint32_t n_lights, int restart, double *host_rgb, uint8_t *host_rgb8, rm_converge_report *report,
                               rm_timing *timing) {
    return guarded(ctx, "rm_render_converging", [&]() {
        return rm_render_converging_impl(ctx, "rm_render_converging", params, lens, converge, rules_with_radii(radii, n_lights), restart, host_rgb,
                                         host_rgb8, report, timing);
    });
}

rm_status rm_render_converging_motion(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const rm_converge *converge,
                                      const double *radii, uint32_t n_lights, const rm_vec3 *velocities, uint32_t n_shapes, double shutter,
                                      int restart, double *host_rgb, uint8_t *host_rgb8, rm_converge_report *report, rm_timing *timing) {
    return guarded(ctx, "rm_render_converging_motion", [&]() -> rm_status {
        const tick_swept_scope done{ctx};
        if (rm_status pst = tick_swept_prepare(ctx, "rm_render_converging_motion", velocities, n_shapes, shutter, true)) return pst;
        return rm_render_converging_impl(ctx, "rm_render_converging_motion", params, lens, converge,
                                         rules_with_motion(radii, n_lights, velocities, n_shapes, shutter), restart, host_rgb, host_rgb8, report,
                                         timing);
    });
}

}  // extern "C"
