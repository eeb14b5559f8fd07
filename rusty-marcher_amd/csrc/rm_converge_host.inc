// rm_converge_host.inc -- host side of the converging frames' device call (include/rusty_marcher_amd.h, "converging frames");
// included at the end of rm_device.hip, behind rm_accum_host.inc whose checks (check_accum_device, check_offset_tables) it shares,
// and rm_refine_host.inc whose workspace size.  The kernels are rm_converge.hip's.
//
// Here: the check of rm_converge (check_converge) and of a device call's arguments (check_converge_call), the converging block
// of a launch (converge_args), the three steps of a pass (launch_converge_with) and rm_accumulate_converging_device, which
// touches no render state and keeps all of its own in the caller's buffers: a memset of the list's length, the select launch,
// the shade launch, all on the caller's stream, nothing waited for.  rm_converge_motion_host.inc behind this file adds the
// moving spheres' launch and, behind both launches, the tick rm_render_converging*.

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

// What both device calls check of their arguments (ctx is not NULL), in the order a call with several faults reports them: the
// frame's struct, check_accum_device with its sum and mean, the call's offset tables (`tables`), the rule, the frame's other
// required pointers
template <class TABLES>
static rm_status check_converge_call(rm_ctx *ctx, const char *who, const rm_params *p, const rm_lens *lens, const rm_converge *c,
                                     const void *device_table, uint32_t table_rows, const rm_converge_frame *b, TABLES tables) {
    if (!b) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL buffers");
    if (rm_status cst = check_accum_device(ctx, who, p, lens, device_table, 0u, b->sum, b->mean)) return cst;
    if (rm_status ost = tables()) return ost;
    if (rm_status vst = check_converge(ctx, who, lens, c, table_rows)) return vst;
    if (!b->stats) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL stats");
    if (!b->count) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL count");
    if (!b->workspace) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL workspace");
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

extern "C" {

rm_status rm_converge_workspace(const rm_params *params, size_t *bytes) {
    if (!params || !bytes) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_converge_workspace: NULL argument");
    if (params->frame_width % RM_PATCH_SIZE != 0)
        return ctx_fail(nullptr, RM_ERR_DIMENSIONS, "rm_converge_workspace: frame width is not a multiple of 32");
    *bytes = refine_workspace_bytes(params);
    return RM_OK;
}

rm_status rm_accumulate_converging_device(rm_ctx *ctx, const rm_params *p, const rm_lens *lens, const rm_converge *c, const void *device_table,
                                          uint32_t table_rows, const void *device_offsets, uint32_t n_lights, int fresh,
                                          const rm_converge_frame *b, void *hip_stream) {
    const char *who = "rm_accumulate_converging_device";
    return guarded(ctx, who, [&]() -> rm_status {
        if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
        // (without a table n_lights is not looked at)
        auto tables = [&]() { return device_offsets ? check_offset_tables(ctx, who, "offsets", device_offsets, n_lights) : RM_OK; };
        if (rm_status cst = check_converge_call(ctx, who, p, lens, c, device_table, table_rows, b, tables)) return cst;
        if (refine_rows(p) == 0u) return RM_OK;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        // (a scene without lights never fetches an offset: the kernel with stored lights)
        return launch_converge(ctx, p, lens, c, device_table, table_rows, ctx->image.H.n_lights > 0u ? device_offsets : nullptr, fresh, b,
                               (hipStream_t)hip_stream);
    });
}

}  // extern "C"
