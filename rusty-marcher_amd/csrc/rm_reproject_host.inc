// rm_reproject_host.inc -- host side of the temporal reprojection (include/rusty_marcher_amd.h, "temporal reprojection");
// included at the end of rm_device.hip, behind rm_denoise_host.inc whose check of the params (check_denoise_params) it shares and
// rm_converge_motion_host.inc whose converging state (rm_converging) holds the history's settings, buffers and report.  The
// kernel is rm_reproject.hip's.
//
// rm_reproject_device touches no render state and keeps none of its own: where a total is asked for a memset of that word, then
// one launch on the caller's stream, nothing waited for.  The tick that uses it is rm_render_converging_impl
// (rm_converge_motion_host.inc), which calls launch_reproject below with its own buffers; rm_converge_history and
// rm_converge_history_info, here, turn the history on and off and report what the ticks did with it.

// The ranges of rm_reproject; a NaN fails the comparison of its line
static rm_status check_reproject(rm_ctx *ctx, const char *who, const rm_reproject *r) {
    if (!r) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL reproject");
    char buf[192];
    if (!std::isfinite(r->sigma_z) || !(r->sigma_z > 0.)) {
        std::snprintf(buf, sizeof buf, "%s: reproject.sigma_z = %g is not a finite number > 0", who, r->sigma_z);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    if (!(r->min_normal_dot >= -1. && r->min_normal_dot < 1.)) {
        std::snprintf(buf, sizeof buf, "%s: reproject.min_normal_dot = %g is outside [-1, 1)", who, r->min_normal_dot);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    if (r->max_history < 1u || r->max_history > RM_PROGRESSIVE_MAX_SAMPLES) {
        std::snprintf(buf, sizeof buf, "%s: reproject.max_history = %u is outside 1..%u", who, r->max_history, RM_PROGRESSIVE_MAX_SAMPLES);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    return RM_OK;
}

// A view: a finite position and a basis rm_camera_basis_check accepts
static rm_status check_view(rm_ctx *ctx, const char *who, const rm_view *v) {
    if (!v) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL previous_view");
    if (!finite3(v->position)) {
        char buf[192];
        std::snprintf(buf, sizeof buf, "%s: previous_view.position (%g, %g, %g) is not finite", who, v->position.x, v->position.y, v->position.z);
        return ctx_fail(ctx, RM_ERR_INVALID_ARG, buf);
    }
    if (rm_status st = rm_camera_basis_check(&v->basis))
        return ctx_fail(ctx, st, std::string(who) + ": previous_view.basis: " + rm_get_host_error());
    return RM_OK;
}

// The buffers of a call; carried, carried_total, mean and rgb8 may be NULL (the last two are the tick's alone)
struct reproject_buffers {
    const void *prev_sum, *prev_stats, *prev_count, *prev_hits, *cur_hits;
    void *out_sum, *out_stats, *out_count, *carried, *carried_total, *mean, *rgb8;
};

static rm_status check_reproject_buffers(rm_ctx *ctx, const char *who, const reproject_buffers &b) {
    const struct { const char *name; const void *p; } inputs[] = {
        {"prev_sum", b.prev_sum}, {"prev_stats", b.prev_stats}, {"prev_count", b.prev_count}, {"prev_hits", b.prev_hits}, {"cur_hits", b.cur_hits}};
    const struct { const char *name; const void *p; bool required; } outputs[] = {
        {"out_sum", b.out_sum, true}, {"out_stats", b.out_stats, true}, {"out_count", b.out_count, true},
        {"out_carried", b.carried, false}, {"out_carried_total", b.carried_total, false}};
    for (const auto &i : inputs)
        if (!i.p) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL " + i.name);
    for (const auto &o : outputs)
        if (!o.p && o.required) return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": NULL " + o.name);
    for (const auto &o : outputs)
        for (const auto &i : inputs)
            if (o.p && o.p == i.p)
                return ctx_fail(ctx, RM_ERR_INVALID_ARG, std::string(who) + ": an output would overwrite an input (" + o.name + " == " + i.name + ")");
    return RM_OK;
}

// The launch on `stream`; everything was checked, rows > 0
static rm_status launch_reproject(rm_ctx *ctx, const rm_params *p, const rm_reproject *r, const rm_view *v, const reproject_buffers &b,
                                  hipStream_t stream) {
    ReprojectArgs a{};
    a.frame_width = p->frame_width;
    a.rows = refine_rows(p);
    a.max_history = r->max_history;
    a.width = p->width; a.height = p->height; a.ratio = p->ratio; a.half_fov = p->half_fov;
    a.sigma_z = r->sigma_z; a.min_normal_dot = r->min_normal_dot;
    a.ex = v->position.x; a.ey = v->position.y; a.ez = v->position.z;
    a.rx = v->basis.right.x; a.ry = v->basis.right.y; a.rz = v->basis.right.z;
    a.ux = v->basis.up.x; a.uy = v->basis.up.y; a.uz = v->basis.up.z;
    a.fx = v->basis.forward.x; a.fy = v->basis.forward.y; a.fz = v->basis.forward.z;
    a.prev_sum = static_cast<const double *>(b.prev_sum);
    a.prev_stats = static_cast<const double *>(b.prev_stats);
    a.prev_count = static_cast<const uint32_t *>(b.prev_count);
    a.prev_hits = static_cast<const double *>(b.prev_hits);
    a.cur_hits = static_cast<const double *>(b.cur_hits);
    a.out_sum = static_cast<double *>(b.out_sum);
    a.out_stats = static_cast<double *>(b.out_stats);
    a.out_count = static_cast<uint32_t *>(b.out_count);
    a.carried = static_cast<uint8_t *>(b.carried);
    a.carried_total = static_cast<uint32_t *>(b.carried_total);
    a.mean = static_cast<double *>(b.mean);
    a.rgb8 = static_cast<uint8_t *>(b.rgb8);
    if (a.carried_total) RM_HIP(ctx, hipMemsetAsync(a.carried_total, 0, sizeof(uint32_t), stream));
    void *args[] = {(void *)&a};
    RM_HIP(ctx, hipLaunchKernel(rm_reproject_kernel(), dim3(a.frame_width / RM_REPROJECT_TILE_W, a.rows / RM_REPROJECT_TILE_H),
                                dim3(RM_REPROJECT_TILE_W * RM_REPROJECT_TILE_H), args, 0, stream));
    return RM_OK;
}

// What the tick hands over (declared in rm_converge_motion_host.inc): its own buffers, mean and bytes included
static rm_status launch_reproject_tick(rm_ctx *ctx, const rm_params *p, const rm_reproject *r, const rm_view *v, const void *prev_sum,
                                       const void *prev_stats, const void *prev_count, const void *prev_hits, const void *cur_hits, void *out_sum,
                                       void *out_stats, void *out_count, void *carried_total, void *mean, void *rgb8, hipStream_t stream) {
    const reproject_buffers b{prev_sum, prev_stats, prev_count, prev_hits, cur_hits, out_sum, out_stats, out_count, nullptr, carried_total, mean, rgb8};
    return launch_reproject(ctx, p, r, v, b, stream);
}

extern "C" {

rm_status rm_reproject_device(rm_ctx *ctx, const rm_params *p, const rm_reproject *r, const rm_view *previous_view, const void *prev_sum,
                              const void *prev_stats, const void *prev_count, const void *prev_hits, const void *cur_hits, void *out_sum,
                              void *out_stats, void *out_count, void *out_carried, void *out_carried_total, void *hip_stream) {
    const char *who = "rm_reproject_device";
    return guarded(ctx, who, [&]() -> rm_status {
        if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
        if (rm_status pst = check_denoise_params(ctx, who, p)) return pst;
        if (rm_status rst = check_reproject(ctx, who, r)) return rst;
        if (rm_status vst = check_view(ctx, who, previous_view)) return vst;
        const reproject_buffers b{prev_sum, prev_stats, prev_count, prev_hits, cur_hits, out_sum, out_stats, out_count, out_carried, out_carried_total,
                                  nullptr, nullptr};
        if (rm_status bst = check_reproject_buffers(ctx, who, b)) return bst;
        if (refine_rows(p) == 0u) return RM_OK;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        return launch_reproject(ctx, p, r, previous_view, b, (hipStream_t)hip_stream);
    });
}

rm_status rm_converge_history(rm_ctx *ctx, const rm_reproject *reproject) {
    const char *who = "rm_converge_history";
    return guarded(ctx, who, [&]() -> rm_status {
        if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, std::string(who) + ": NULL ctx");
        if (reproject)
            if (rm_status rst = check_reproject(ctx, who, reproject)) return rst;
        if (!reproject && !ctx->converging) return RM_OK;                 // (off, and nothing was ever on)
        if (!ctx->converging) ctx->converging = new rm_converging();
        rm_converging &g = *ctx->converging;
        if (reproject) {
            g.history = true;
            g.history_rule = *reproject;
            return RM_OK;
        }
        g.history = false;
        RM_HIP(ctx, hipSetDevice(ctx->device));
        return converging_drop_history(ctx, g);
    });
}

rm_status rm_converge_history_info(rm_ctx *ctx, rm_history_report *report) {
    if (!ctx) return ctx_fail(nullptr, RM_ERR_INVALID_ARG, "rm_converge_history_info: NULL ctx");
    if (!report) return ctx_fail(ctx, RM_ERR_INVALID_ARG, "rm_converge_history_info: NULL report");
    rm_history_report rep{};
    if (const rm_converging *g = ctx->converging) {
        rep.reprojections = g->reprojections;
        rep.last_reprojected = g->last_reprojected;
        rep.carried = g->carried;
        rep.without = g->without;
    }
    *report = rep;
    return RM_OK;
}

}  // extern "C"
