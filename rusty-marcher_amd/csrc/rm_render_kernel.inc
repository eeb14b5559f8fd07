// rm_render_kernel.inc -- render_tile and the kernel, once per numeric flavour (no include
// guard; see rm_render_kernel.hpp).
namespace RM_FLAVOR_NS {
using namespace rmdev;

// One 16x4 tile, one wave.  cast_ray's recursion (renderer.rs:254-309) becomes a loop over
// RAY STEPS that all 64 lanes take together: in a step every lane that holds a ray finds its
// closest hit, shades it, and turns into the ray's refracted (else reflected) child; where
// both children exist the reflected one is parked.  Radiance is linear in the children
// (renderer.rs:219,249), so a ray carries the product of the factors above it and adds
// `weight x (background + direct light)` to its pixel's sum -- which is not always the lane's
// own pixel:
//
// Ray-tree parallelism.  A pixel's tree has 1 to 2^(depth-1) rays (demo scene: 1.9 on
// average, 8 at most), so lanes run out of work at different times.  A lane whose tree is
// done takes over the OLDEST parked ray of a lane that still has one (its level-0 slot, which
// lives in LDS in a lane-contiguous column, readable by any lane): one ballot of idle lanes,
// one of donors, ranks by mbcnt, a 64-entry table in LDS to pair them up.  The loop ends
// when no lane holds a ray, i.e. after about (rays of the tile / 64) steps instead of
// (rays of its deepest pixel) steps.  Which lane renders which ray depends on nothing but the
// tile's own rays, so the image is reproducible bit for bit; the ORDER in which a pixel's
// terms are summed differs from the recursion's (allowed: it feeds no decision).
//
// Parked rays: each lane has a stack of its own -- level 0 in LDS (written only when the
// stack is empty, so it always holds the shallowest parked ray of the lane's current tree),
// deeper levels in scratch.  A lane works depth-first on ONE tree at a time, so its parked
// rays have distinct depths: at most max_depth - 1 of them (STACK = 4 / 8 / 16 / 32).
// Returns whether the tile has to be rendered again by the exact code -- nothing of it has been stored then (RM_CHECKED, the
// range-free numerics of rm_trace.inc: some lane met an operand outside their range); never, otherwise.
// SIG: the scene signature the body is compiled for (rm_kernel_args.hpp RM_SCENE_SIGNATURES; 0: any scene).  Under a signature the
// body below is the same text over a copy of the scene view whose counts are the signature's constants: the walks' loops over
// them unroll, their remainder loops, the tie keys behind list_ordered and the hierarchy alternatives go.  The values are
// assigned, not assumed -- the host's verdict (rm_plan.cpp rm_scene_signature) makes them the image's own.
template <int STACK, int POW, bool BVH, bool CULL, bool EDGES, bool PREFETCHED, int SIG = 0>
__device__ __forceinline__ bool render_tile(const SceneView &sc_any, const KernelArgs &a, uint32_t tx0, uint32_t ty0,
                                            uint32_t tyf, uint32_t ty8, double bp_x, double bp_y, double *wl,
                                            double *__restrict__ frame_in, unsigned long long *stats, bool have_mask,
                                            unsigned long long first_mask, const char *kargs_of_kernel) {
    SceneView sc_sig;
    if constexpr (SIG != 0) {
        constexpr SceneSignature K = RM_SCENE_SIGNATURES[SIG - 1];
        sc_sig = sc_any;
        sc_sig.H.n_spheres = K.n_spheres; sc_sig.H.n_polygons = K.n_polygons; sc_sig.H.n_triangles = K.n_triangles;
        sc_sig.H.n_lights = K.n_lights; sc_sig.H.list_ordered = K.list_ordered;
        sc_sig.H.off_bvh_spheres = 0u; sc_sig.H.off_bvh_triangles = 0u;
    }
    const SceneView &sc = SIG != 0 ? sc_sig : sc_any;
    const uint32_t lane = threadIdx.x & 63u;
    const V3 bg = mk(own_sgpr(a.bg_x), own_sgpr(a.bg_y), own_sgpr(a.bg_z));
    const uint32_t max_depth = own_sgpr(a.max_depth);
#if RM_CHECKED
    bool sus = false;                                         // per lane: an operand outside the checked sequences' range
#endif

    // the wave's LDS block (rm_render_kernel.hpp): level 0 of the ray stacks, the pixel sums
    // (which the store phase reads as they lie: [pixel][channel] is the tile's row-major
    // order), the pairing table of the hand-over
    double *const lds0 = wl + lane;                            // field f of this lane's level 0 at lds0[64 * f]
    uint32_t *const l0_depth = reinterpret_cast<uint32_t *>(wl + RM_WAVE_L0_DEPTH_WORDS);
    double *const sum = wl + RM_WAVE_SUM_WORDS;
    uint32_t *const pair = reinterpret_cast<uint32_t *>(wl + RM_WAVE_PAIR_WORDS);

    // backproject, renderer.rs:128-135 (no pixel-centre offset).  Exact divisions in both
    // flavours: x / width must be the reference's value -- on the image's centre column and
    // row it is exactly 0.5, the ray component exactly 0, and symmetric scenes then sit
    // exactly on polygon edges (x * (1/width) lost that and flipped 117 edge pixels of an
    // icosphere, profiles/r01_notes_fast_flavour.txt).
    // (The two unnormalised components depend on the column and on the row only: the host
    // tabulates them once per frame geometry with these very operations, rm_device.hip
    // backproject_tables -- two loads instead of two divisions and six multiplies per pixel.)
    // (PREFETCHED: fetched by the caller -- in the kernels with the feedback they travel while the tile's flag does)
#if RM_KERNEL_ORIENTED
    // The oriented camera: the same two table values along the view's own right and up, plus its forward -- per component two
    // products and two sums in this order (the strict flavour rounds each once; the fast one may contract).  The nine words are
    // kernel arguments: scalar registers, one scalar operand to a vector instruction.
    const double bx = PREFETCHED ? bp_x : a.bp_x[tx0 + (lane % TILE_W)], by = PREFETCHED ? bp_y : a.bp_y[ty0 + (lane / TILE_W)];
    V3 dir = RM_NORMALIZED(mk((bx * a.cam_rx + by * a.cam_ux) + a.cam_fx, (bx * a.cam_ry + by * a.cam_uy) + a.cam_fy, (bx * a.cam_rz + by * a.cam_uz) + a.cam_fz), true);
#else
    V3 dir = RM_NORMALIZED(PREFETCHED ? mk(bp_x, bp_y, -1.) : mk(a.bp_x[tx0 + (lane % TILE_W)], a.bp_y[ty0 + (lane / TILE_W)], -1.), true);
#endif
    V3 orig = mk(a.cam_x, a.cam_y, a.cam_z);
    double weight = 1.;
    uint32_t depth = 1;                                       // renderer.rs:83
    uint32_t pix = lane;                                      // the pixel (of this tile) the lane's ray belongs to
    bool on = true;                                           // the lane holds a ray
    // A lane sums its OWN pixel's terms in registers; the terms of rays taken over from other
    // lanes go to the pixels' sums in LDS by float atomics (zeroed when the first ray changes
    // hands: most tiles never get there) and are added in at the end.
    V3 acc = mk(0., 0., 0.);
    bool handed = false;                                      // wave-uniform: a ray has changed hands in this tile

    StackEntry deep[STACK > 1 ? STACK - 1 : 1];
    uint32_t n_deep = 0;
    bool l0_full = false;
#ifdef RM_EXP_STAMPS
    uint32_t st_steps = 0, st_rays = 0, st_taken = 0;
#endif
    __builtin_amdgcn_wave_barrier();
#if defined(RM_EXP_STAMPS) && defined(RM_EXP_STARTUP)
    // (the first ray step waits for the primary directions: the value is asked for before the time is)
    if (dir.x == 12345.678) sc.cnt[2] = 1u;
    sc.cnt[1] |= (((uint32_t)__builtin_amdgcn_s_memrealtime() - sc.cnt[3]) & 0xFFFFu) << 16;           // the first ray step begins
#endif

    // Kernels without the bundle cull branch per lane (where<> in rm_trace.inc): the step is
    // entered by the lanes that hold a ray, the shading by those that hit, and so on; kernels
    // with it enter every block on a wave vote and predicate inside.  One source for both:
    // under a per-lane branch the predicate is the constant `true` and folds away.
    constexpr bool DIV = !CULL;
    // The hand-over of parked rays is compiled into the kernels with the cull only.  Measured
    // (profiles/r02_handover.txt): on the demo scene the rays of a tile are so alike that 98.9 %
    // of the lanes hold a ray in every step anyway and 0.3 % of the rays change hands, while
    // its bookkeeping costs the few-primitive kernel 5 % (89.2 against 84.6 us at 1080p).
    // (Culling only the tile's primary bundle in that kernel -- 40 % of its tiles see nothing but
    // sky -- was measured too: 85.9 against 83.9 us; a cull step costs what it saves there.)
    constexpr bool HANDOVER = CULL;
    // Children that leave a glass-like polygon / triangle into an empty half-space (rm_image.cpp rm_build_empty_sides; the
    // launch plan says whether the image's flags hold for this camera) are not walked: per-lane kernels only -- the others
    // form one fused term per step, and the sum would round differently.
    // (one word, two bits -- RM_DEAD_DROP, RM_DEAD_EARLY_FATES: no second argument is live through the tile)
    const uint32_t dead_word = DIV ? own_sgpr(a.dead_children) : 0u;     // wave-uniform
    const bool dead_children = (dead_word & RM_DEAD_DROP) != 0u, early_fates = (dead_word & RM_DEAD_EARLY_FATES) != 0u;
    uint32_t step = 0;
    for (;; step++) {                                          // one ray step; the loop itself is wave-uniform
        // Critical-path scheduling: a launch ends with its deepest tiles (8 steps where the mean
        // is 2), so a wave that is past its first steps outranks the waves it shares the SIMD with.
        if (step == 1u) __builtin_amdgcn_s_setprio(1);
        else if (step == 2u) __builtin_amdgcn_s_setprio(2);
        else if (step == 3u) __builtin_amdgcn_s_setprio(3);
#ifdef RM_EXP_STAMPS
        st_steps++; st_rays += (uint32_t)__popcll(__ballot(on));
#endif
        bool next = false;                                     // the lane goes on with a child of its ray
        if (where<DIV>(on)) {
            Hit h;
            // (the primary rays of a classified tile test the primitives of its mask only: rm_classify.hip)
            const unsigned long long t_ch = RM_PHASE_T();
            const bool got = closest_hit<BVH, CULL, EDGES>(sc, orig, dir, on, h, have_mask & (step == 0u), first_mask) & on;
            RM_PHASE_ADD(sc, 0, t_ch);
            // what this step adds to the ray's pixel: weight x (background + direct light) on a
            // hit (renderer.rs:272-275), weight x background where a secondary ray leaves the
            // scene (:302-303), nothing where a primary ray does (:305), + the children beyond
            // the cap.  Lanes without a ray add zero.
            // (Per-lane kernels add each term where it arises, under the branch that is there
            // anyway; the others form one predicated term per step.)
            V3 L = bg;
            const double w_add = (on & (got | (depth > 1u))) ? weight : 0.;
            double w_cap = 0.;
            if (DIV && !got && depth > 1u) acc = acc + scaled(bg, weight);
            if (where<DIV>(got)) {
                const Surface s = surface_at<DIV>(sc, orig, dir, h, got RM_SUS_ARG);
                const unsigned long long t_sd = RM_PHASE_T();
                L = pick(got, bg + shade_direct<POW, BVH, CULL, EDGES>(sc, neg(dir), s, got, h.pid RM_SUS_ARG), bg);
                RM_PHASE_ADD(sc, 3, t_sd);
                if (DIV) acc = acc + scaled(L, weight);
                const bool glass = got & (s.mat[8] != 0.);     // is_glass_like, renderer.rs:277
                if (where<DIV>(glass)) {
                    const double reflection = s.mat[6], ri = s.mat[7], inv_ri = s.mat[9];   // (1 / ri: the upload's division, rm_image.cpp put_material)
                    V3 ro, rd, to, td;
                    double dn_r, dn_t;                          // rd . normal, td . normal: the dots the children's origins were offset by
                    const bool has_r = glass & reflect_child<DIV>(dir, s, ri, inv_ri, ro, rd, dn_r);   // renderer.rs:195-222
                    bool has_t = false, fated_dead = false;     // renderer.rs:225-252
                    if (!DIV) has_t = glass & refract_child(dir, s, ri, inv_ri, glass, to, td, dn_t RM_SUS_ARG);
                    const double wr = weight * reflection, wt = weight * (1. - reflection);
                    // a child beyond the cap returns the background (renderer.rs:262-264)
                    const bool capped = depth + 1u > max_depth;
                    if (DIV) {
                        // Early child fates: the refracted ray is formed only where it is walked or its computed dot decides.
                        // Not beyond the cap (only `has_t` counts there); not where it leaves into a flagged side for certain --
                        // d . normal is -+sqrt(cos_theta_2): with the flip it points to the normal's side, else to the other one,
                        // and away from the critical angle the computed dot has that sign (DESIGN.md section 4).
                        const RefractFate f = refract_fate(dir, s, ri, inv_ri);
                        has_t = glass & f.has;
                        bool ray = glass;
                        if (early_fates) {
                            const uint32_t sides = (uint32_t)s.mat[8];
                            fated_dead = dead_children & has_t & !capped & (f.cos_theta_2 >= RM_FATE_COS2_MIN) & (f.r <= RM_FATE_R_MAX) &
                                         ((sides & (f.flip ? 2u : 4u)) != 0u);
                            ray = has_t & !capped & !fated_dead;
                        }
                        // (the ray goes where the lane's ray lives: `to` and `td` beside `orig` and `dir`, through the parking
                        // below, were ten vector registers spilt in the ray-step loop)
                        dn_t = 0.;
                        if (ray) {
                            refract_ray(dir, s, f, glass, to, td, dn_t RM_SUS_ARG);
                            orig = to;
                            dir = td;
                        }
                    }
                    w_cap = ((capped & has_r) ? wr : 0.) + ((capped & has_t) ? wt : 0.);
                    if (DIV && capped) acc = acc + scaled(bg, w_cap);
                    bool live_r = has_r & !capped, live_t = has_t & !capped;
                    if (DIV && dead_children) {
                        // A child starts on the side of the surface its direction points to (optics.rs:41-45, :82-86): where
                        // the glass word (1 + 2 x empty(+) + 4 x empty(-)) says that side of the plane holds nothing, its step
                        // would find no hit -- the plane's own test rejects it on the sign of the dot its origin was offset by -- and add
                        // weight x background: added here, in its place (a term of its own: 0. + w is not always w), and the
                        // ray is dropped.  d . normal == 0 leaves it alive.  The order of the pixel's terms stays what it was:
                        // the refracted child is walked first, and the reflected one is dropped only where it would be next.
                        const uint32_t sides = (uint32_t)s.mat[8];
                        // (a child whose fate was decided early has no ray and dn_t == 0: the two never overlap)
                        const bool dead_t = fated_dead | (live_t & (((dn_t > 0.) & ((sides & 2u) != 0u)) | ((dn_t < 0.) & ((sides & 4u) != 0u))));
                        if (dead_t) acc = acc + scaled(bg, wt);
                        live_t = live_t & !dead_t;
                        if (live_r & !live_t) {
                            const bool dead_r = ((dn_r > 0.) & ((sides & 2u) != 0u)) | ((dn_r < 0.) & ((sides & 4u) != 0u));
                            if (dead_r) acc = acc + scaled(bg, wr);
                            live_r = live_r & !dead_r;
                        }
                    }
                    // both children: park the reflected sibling (the stores are per-lane branches)
                    const bool park = live_r & live_t, park_l0 = park & (n_deep == 0u) & !l0_full;
                    if (park_l0) {
                        lds0[0] = ro.x; lds0[64] = ro.y; lds0[128] = ro.z;
                        lds0[192] = rd.x; lds0[256] = rd.y; lds0[320] = rd.z;
                        lds0[384] = wr;
                        l0_depth[lane] = depth + 1u;
                    }
                    if (park & !park_l0) {
                        StackEntry &e = deep[n_deep];
                        e.ox = ro.x; e.oy = ro.y; e.oz = ro.z;
                        e.dx = rd.x; e.dy = rd.y; e.dz = rd.z;
                        e.w = wr; e.depth = depth + 1u;
                    }
                    n_deep += (park & !park_l0) ? 1u : 0u;
                    l0_full = l0_full | park_l0;
                    // walk into the refracted child, else the reflected one (lanes whose ray ends
                    // here get values nobody reads: they take a parked ray or fall idle below)
                    next = live_r | live_t;
                    orig = pick(live_t, DIV ? orig : to, ro);
                    dir = pick(live_t, DIV ? dir : td, rd);
                    weight = live_t ? wt : wr;
                    depth += 1u;
                }
            }
            const V3 term = mk(__builtin_fma(bg.x, w_cap, L.x * w_add), __builtin_fma(bg.y, w_cap, L.y * w_add),
                               __builtin_fma(bg.z, w_cap, L.z * w_add));
            if (DIV) {
                // (added above)
            } else if (!HANDOVER || pix == lane) {
                acc = acc + term;
            } else {                                           // a ray taken over: several lanes may work on one pixel
                __hip_atomic_fetch_add(&sum[pix * 3 + 0], term.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                __hip_atomic_fetch_add(&sum[pix * 3 + 1], term.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                __hip_atomic_fetch_add(&sum[pix * 3 + 2], term.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            }
            // a lane whose ray ended takes a parked ray of its own: deepest first, level 0 last
            const bool pop_deep = on & !next & (n_deep > 0u);
            if (where<DIV>(pop_deep)) {
                n_deep -= pop_deep ? 1u : 0u;
                const StackEntry &e = deep[pop_deep ? n_deep : 0u];
                orig = pick(pop_deep, mk(e.ox, e.oy, e.oz), orig);
                dir = pick(pop_deep, mk(e.dx, e.dy, e.dz), dir);
                weight = pop_deep ? e.w : weight;
                depth = pop_deep ? e.depth : depth;
            }
            const bool pop_l0 = on & !next & !pop_deep & l0_full;
            if (where<DIV>(pop_l0)) {
                orig = pick(pop_l0, mk(lds0[0], lds0[64], lds0[128]), orig);
                dir = pick(pop_l0, mk(lds0[192], lds0[256], lds0[320]), dir);
                weight = pop_l0 ? lds0[384] : weight;
                depth = pop_l0 ? l0_depth[lane] : depth;
                l0_full = l0_full & !pop_l0;
            }
            next = next | pop_deep | pop_l0;
        }
        on = on & next;

        // hand-over: the k-th idle lane takes the level-0 ray of the k-th lane that has one
        if (!HANDOVER) {                                       // every lane walks its own pixel's tree, and leaves
            if (!on) break;                                    // the loop when it is done (a per-lane exit)
            continue;
        }
        const unsigned long long idle = __ballot(!on), donors = __ballot(l0_full);
        if (idle == ~0ull) break;                              // no lane holds a ray (an idle lane has nothing parked either)
        if (idle != 0ull && donors != 0ull) {
            const uint32_t n_pairs = min((uint32_t)__popcll(idle), (uint32_t)__popcll(donors));
            const uint32_t my_idle = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
            const uint32_t my_donor = __builtin_amdgcn_mbcnt_hi((uint32_t)(donors >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)donors, 0u));
            const bool give = l0_full & (my_donor < n_pairs), take = !on & (my_idle < n_pairs);
            if (!handed) {
                sum[lane * 3 + 0] = 0.; sum[lane * 3 + 1] = 0.; sum[lane * 3 + 2] = 0.;
                handed = true;
            }
            if (give) pair[my_donor] = lane | (pix << 8);
            __builtin_amdgcn_wave_barrier();
            if (take) {
                const uint32_t from = pair[my_idle];
                const double *src = wl + (from & 63u);
                orig = mk(src[0], src[64], src[128]);
                dir = mk(src[192], src[256], src[320]);
                weight = src[384];
                depth = l0_depth[from & 63u];
                pix = from >> 8;
                on = true;
            }
            l0_full = l0_full & !give;
            __builtin_amdgcn_wave_barrier();
#ifdef RM_EXP_STAMPS
            st_taken += n_pairs;
#endif
        }
    }
    __builtin_amdgcn_wave_barrier();
#if RM_CHECKED
    if (__any(sus)) return true;                               // (wave-uniform; nothing of the tile has left the wave)
#endif
    if (handed) acc = acc + mk(sum[lane * 3 + 0], sum[lane * 3 + 1], sum[lane * 3 + 2]);
    sum[lane * 3 + 0] = acc.x;
    sum[lane * 3 + 1] = acc.y;
    sum[lane * 3 + 2] = acc.z;
    __builtin_amdgcn_wave_barrier();
#if defined(RM_EXP_STAMPS) && defined(RM_EXP_STARTUP)
    sc.cnt[2] = (uint32_t)__builtin_amdgcn_s_memrealtime() - sc.cnt[3];                                 // the last ray step is over
#endif

    // ---- store the tile: the sums lie in LDS as [pixel][channel], the tile's row-major order,
    // so each of its rows leaves as contiguous 16-byte pieces (16x4 tile: 384 B = three whole
    // lines; frame.buffer[y][x], renderer.rs:103)
    // (what the stores need of the kernel's arguments is read afresh from the argument segment: asked of `a` it would sit in
    // scalar registers -- spilt ones -- through every ray step of the tile)
#ifdef RM_NO_REREAD
    const uint32_t frame_width = a.frame_width;
    uint8_t *const frame8 = a.frame8;
    double *__restrict__ frame = frame_in;
#else
    const char *kargs = reread_kernargs(kargs_of_kernel);
    const KernelArgs &b = *reinterpret_cast<const KernelArgs *>(kargs + sizeof(const double *));
    const uint32_t frame_width = b.frame_width;
    uint8_t *const frame8 = b.frame8;
    double *__restrict__ frame = *reinterpret_cast<double *const *>(kargs + sizeof(const double *) + sizeof(KernelArgs));
    (void)frame_in;
#endif
    const double2 *sum2 = reinterpret_cast<const double2 *>(sum);
    constexpr uint32_t PIECES = TILE_W * 3u / 2u;             // 16-byte pieces per tile row
    for (uint32_t q = lane; q < 96u; q += 64u) {
        const uint32_t row = q / PIECES, piece = q % PIECES;
        double2 *dst = reinterpret_cast<double2 *>(frame + ((size_t)(tyf + row) * frame_width + tx0) * 3u);
        dst[piece] = sum2[row * PIECES + piece];
    }

    // ---- optional display bytes: to_vec / quantize (framebuffer.rs:40-55, :80-82) fused
    // into the epilogue, `(255. * f.max(0.).min(1.)) as u8` per channel, 3 B/pixel
    if (frame8) {                                               // wave-uniform
        const double vx = acc.x, vy = acc.y, vz = acc.z;
        uint8_t *slab8 = reinterpret_cast<uint8_t *>(wl);      // the level-0 columns are free now
        slab8[lane * 3 + 0] = (uint8_t)(255. * __builtin_fmin(__builtin_fmax(vx, 0.), 1.));
        slab8[lane * 3 + 1] = (uint8_t)(255. * __builtin_fmin(__builtin_fmax(vy, 0.), 1.));
        slab8[lane * 3 + 2] = (uint8_t)(255. * __builtin_fmin(__builtin_fmax(vz, 0.), 1.));
        __builtin_amdgcn_wave_barrier();
        constexpr uint32_t P8 = TILE_W * 3u / 8u;              // 8-byte pieces per tile row
        if (lane < 24u) {
            const uint32_t row = lane / P8, piece = lane % P8;
            unsigned long long *dst = reinterpret_cast<unsigned long long *>(
                frame8 + ((size_t)(ty8 + row) * frame_width + tx0) * 3u);
            dst[piece] = reinterpret_cast<const unsigned long long *>(wl)[row * P8 + piece];
        }
    }
    __builtin_amdgcn_wave_barrier();
#ifdef RM_EXP_STAMPS
    if (stats) *stats = (unsigned long long)st_steps | ((unsigned long long)st_rays << 16) | ((unsigned long long)st_taken << 40);
#else
    (void)stats;
#endif
    return false;
}

// The tile by the body for signature `sig` (wave-uniform; 0, or a number beyond the table: the body for any scene): one
// comparison a compiled-in signature, N counting down from the table's length.
template <int N, int STACK, int POW, bool BVH, bool CULL, bool EDGES, bool PREFETCHED>
__device__ __forceinline__ bool render_tile_of(uint32_t sig, const SceneView &sc, const KernelArgs &a, uint32_t tx0, uint32_t ty0,
                                               uint32_t tyf, uint32_t ty8, double bp_x, double bp_y, double *wl,
                                               double *__restrict__ frame_in, unsigned long long *stats, bool have_mask,
                                               unsigned long long first_mask, const char *kargs_of_kernel) {
    if constexpr (N > 0) {
        if (sig != (uint32_t)N)
            return render_tile_of<N - 1, STACK, POW, BVH, CULL, EDGES, PREFETCHED>(sig, sc, a, tx0, ty0, tyf, ty8, bp_x, bp_y, wl, frame_in, stats, have_mask, first_mask, kargs_of_kernel);
    }
    return render_tile<STACK, POW, BVH, CULL, EDGES, PREFETCHED, N>(sc, a, tx0, ty0, tyf, ty8, bp_x, bp_y, wl, frame_in, stats, have_mask, first_mask, kargs_of_kernel);
}
#undef RM_SUS_PARAM
#undef RM_SUS_ARG
#undef RM_NORMALIZED
#undef RM_SQRT_DISCRIMINANT
#if RM_CHECKED
#undef RM_CHECKED_X_MIN
#undef RM_CHECKED_X_MAX
#endif

#if !RM_CHECKED   // (the checked copy is the tile body alone: the kernels are the strict namespace's)

// What a patch is sorted by: its LONGEST tile.  A launch ends with the tiles that were started late and run long; sorted by
// the sum of its tiles' times a patch of a few 30-us tiles among cheap ones went out in the middle of the launch, and the
// launch drained for 15 us (list scheduling over the measured tile times: 73.5 us by the sum, 66.8 by the longest tile,
// 66.4 with every tile sorted on its own).
#ifndef RM_PATCH_COST_OP
#define RM_PATCH_COST_OP atomicMax
#endif

// The place `k` of the dispatch order (KernelArgs::ord_flat): one word, written by one of the launch's classifying workgroups
// (rm_classify.inc order_places) -- the launch's first, all dispatched before any wave that asks -- which
// says itself when it is there (it carries the launch's tag).  A wave that runs out of patience (RM_ORD_PATIENCE polls) asks for
// the order of last resort instead (see the launch's decision word, rm_kernel_args.hpp): correct, only slower.  ~0: gave up even so,
// which cannot happen -- the frame is void and the host is told (err_word).  The wait is bounded in POLLS, not in time: where several processes share the card its scheduler
// takes a queue's waves off the chip for milliseconds at a time, the clock runs on, and a wave that comes back must not find
// its patience spent on a wait during which nobody of its launch ran (found by two ranks on one GPU).  2^16 polls of ~1.5 us: a
// tenth of a second of waiting in earnest.  `sky`: nothing can be hit in the patch.
#ifndef RM_ORD_POLLS
#define RM_ORD_POLLS 65536u
#endif
__device__ __forceinline__ uint32_t order_entry(const KernelArgs &a, uint32_t k, bool &sky, bool &last_resort) {
    const uint32_t n_dyn = (a.n_tiles >> 4) - (a.n_static >> 4);
    uint32_t entry = 0u;
    bool gave_up = k >= a.ord_cap || k >= n_dyn;                      // (beyond the places there are: cannot happen)
    last_resort = false;
    if (a.ord_read != a.ord_flat) {
        // the previous launch's order: that launch is over -- an entry that is not there never will be (it fell back on the order
        // of last resort, every wave of it: so does every wave of this one, which all see the same memory)
        // (a plain load of a uniform address: a scalar load, and the sixteen waves of a patch ask for the same word)
        if (!gave_up) entry = a.ord_read[k];
        last_resort = (entry >> RM_ORD_TAG_SHIFT) != a.ord_read_tag;
    } else {
        for (uint32_t polls = 0u; !gave_up; polls++) {
            entry = uniform_u32(__hip_atomic_load(a.ord_flat + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if ((entry >> RM_ORD_TAG_SHIFT) == a.ord_tag) break;
            if ((polls & 63u) == 63u) {
                // out of patience: the order of last resort, if the launch has not decided yet (one word, compare and swap: the
                // classifying workgroups write places only once it carries the launch's tag -- either every wave gets an entry,
                // or none does)
                uint32_t go = uniform_u32(__hip_atomic_load(a.ord_cnt + RM_ORD_GO, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                if (go == 0u && polls >= RM_ORD_PATIENCE) {
                    uint32_t expected = 0u;
                    if ((threadIdx.x & 63u) == 0u)
                        (void)__hip_atomic_compare_exchange_strong(a.ord_cnt + RM_ORD_GO, &expected, a.ord_tag | RM_ORD_FALLBACK_BIT, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    go = uniform_u32(__hip_atomic_load(a.ord_cnt + RM_ORD_GO, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                }
                if (go == (a.ord_tag | RM_ORD_FALLBACK_BIT)) { last_resort = true; break; }
                if (polls >= RM_ORD_POLLS) { gave_up = true; break; }  // (decided, and still no entry: cannot happen)
            }
            __builtin_amdgcn_s_sleep(8);
        }
    }
    uint32_t patch = entry & (RM_ORD_SKY_BIT - 1u);
    sky = (entry & RM_ORD_SKY_BIT) != 0u;
    if (last_resort && !gave_up) {                                    // the place k of the index the launch came with
        patch = lists_ok(a) ? a.dyn_inv[k] : n_dyn - 1u - k;
        sky = false;
    }
    if (gave_up || patch >= (a.n_tiles >> 4)) {
        if ((threadIdx.x & 63u) == 0u && a.err_word) __hip_atomic_store(a.err_word, ((unsigned long long)a.launch_seq << 32) | 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return ~0u;
    }
    return patch;
}

// A patch of the sky tail that is not sky after all (the hint was stale): its wave renders the sixteen tiles itself, one
// after the other -- correct, and slow.  A function of its own, not inlined, that takes nothing but the patch: code that no
// wave of a settled render loop runs must not shape the registers of the others (the kernel's arguments it reads where
// they lie, in the kernel's argument segment: scene pointer, KernelArgs, frame pointer).
// (... and the exact twin of the kernels whose tile body has the checked numerics: `n` = 1, the tile a wave has to render again,
// or renders in the first place where the launch is exact only; `staged`: the wave's LDS block holds the scene already)
template <int STACK, int POW, bool STAGED, bool BVH, bool CULL, bool EDGES>
__device__ __attribute__((noinline)) void render_patch_alone(const char *kargs_of_kernel, uint32_t tile0, uint32_t n = 16u, bool staged = false) {
    // (the pointer arrives in vector registers; it is the same for every lane and points into the constant address
    // space: said so, the argument block is read with scalar loads as in the kernel)
    const unsigned long long kv = (unsigned long long)kargs_of_kernel;
    const unsigned long long ku = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(kv >> 32)) << 32) |
                                  (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)kv);
    const char *kargs = (const char *)reinterpret_cast<const __attribute__((address_space(4))) char *>(ku);
    const double *__restrict__ scene_blob = *reinterpret_cast<const double *const *>(kargs);
    const KernelArgs &a = *reinterpret_cast<const KernelArgs *>(kargs + sizeof(const double *));
    double *__restrict__ frame = *reinterpret_cast<double *const *>(kargs + sizeof(const double *) + sizeof(KernelArgs));
    for (uint32_t t = 0; t < n; t++) {
        const uint32_t tile = tile0 + t;
        uint32_t tx0, ty0, tyf, ty8;
        tile_origin(a, tile, tx0, ty0, tyf, ty8);
        unsigned long long first_mask = ~0ull;
        bool have_mask = false;
        if (a.tile_mask && a.mask_tag) {                            // (the word as it is: whoever calls has waited for it)
            const unsigned long long w = uniform_u64(__hip_atomic_load(const_cast<unsigned long long *>(a.tile_mask) + tile, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if ((uint32_t)(w >> 56) == a.mask_tag) { first_mask = w & 0x00FFFFFFFFFFFFFFull; have_mask = true; }
        }
        if (STAGED && !staged) stage_scene(scene_blob, a.H);
        double *wl = rm_lds + (STAGED ? a.H.total_words : 0u);
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        SceneView sc;
        if (STAGED) sc.S = rm_lds; else sc.S = scene_blob;
        sc.G = scene_blob;
        sc.cull_bounds = scene_blob + a.H.off_bounds;
        sc.cull_planar = scene_blob + a.H.off_planar;
        sc.bstack = reinterpret_cast<uint32_t *>(wl + RM_WAVE_BVH_STACK_WORDS);
        sc.cull_cos = a.cull_cos;
        sc.H = a.H;
#ifdef RM_EXP_STAMPS
        uint32_t cull_counts[4] = {0u, 0u, 0u, 0u};
        sc.cnt = cull_counts;
#endif
        (void)render_tile<STACK, POW, BVH, CULL, EDGES, false>(sc, a, tx0, ty0, tyf, ty8, 0., 0., wl, frame, nullptr, have_mask & (a.mask_exact != 0u), first_mask, kargs_of_kernel);
        if (a.patch_cost && (threadIdx.x & 63u) == 0u) {
            const unsigned long long dt = __builtin_amdgcn_s_memrealtime() - t0;
            RM_PATCH_COST_OP(a.patch_cost + (tile >> 4), dt < 0x00FFFFFFull ? (uint32_t)dt : 0x00FFFFFFu);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// A wave of the sky tail: the `t`-th of the tail_patches places at the end of the order.  Its place lies in the last bucket
// (what the host's hint said it would): the primary-miss value (renderer.rs:305) over the whole patch, 24 KB.  It does not (the
// hint was a guess and the view shows less sky than the frames it came from; such places are the tail's FIRST, the buckets
// being laid end to end): the sixteen waves t * 16 .. behind the grid's end render it while t < ov_cap; beyond that this wave
// does, tile by tile -- correct, and slow.
template <int STACK, int POW, bool STAGED, bool BVH, bool CULL, bool EDGES>
__device__ __attribute__((noinline)) void sky_tail_patch(const char *kargs_of_kernel, uint32_t t) {
    const unsigned long long kv = (unsigned long long)kargs_of_kernel;
    const unsigned long long ku = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(kv >> 32)) << 32) |
                                  (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)kv);
    const char *kargs = (const char *)reinterpret_cast<const __attribute__((address_space(4))) char *>(ku);
    const KernelArgs &a = *reinterpret_cast<const KernelArgs *>(kargs + sizeof(const double *));
    double *__restrict__ frame = *reinterpret_cast<double *const *>(kargs + sizeof(const double *) + sizeof(KernelArgs));
    const uint32_t n_dyn = (a.n_tiles >> 4) - (a.n_static >> 4);
    bool sky, last_resort;
    const uint32_t patch = order_entry(a, n_dyn - a.tail_patches + t, sky, last_resort);
    if (patch == ~0u) return;                                       // (the frame is void: the host is told)
    const uint32_t tile0 = patch * 16u, lane = threadIdx.x & 63u;
    if (last_resort && a.tile_mask && a.mask_tag) {
        // (no order to say what the patch is: its sixteen words of this launch's classification do, if they come)
        unsigned long long *word = const_cast<unsigned long long *>(a.tile_mask) + tile0 + (lane & 15u);
        for (uint32_t polls = 0u; polls < 64u; polls++) {
            const unsigned long long w = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__all((uint32_t)(w >> 56) == a.mask_tag)) { sky = !__any((w & 0x00FFFFFFFFFFFFFFull) != 0ull); break; }
            __builtin_amdgcn_s_sleep(8);
        }
    }
    if (!sky) {
        if (t < a.ov_cap && !last_resort) return;                   // sixteen waves at the grid's end have it
        render_patch_alone<STACK, POW, STAGED, BVH, CULL, EDGES>(kargs, tile0);
        return;
    }
    constexpr uint32_t PIECES = TILE_W * 3u / 2u, P8 = TILE_W * 3u / 8u;
    for (uint32_t i = 0; i < 16u; i++) {
        uint32_t tx0, ty0, tyf, ty8;
        tile_origin(a, tile0 + i, tx0, ty0, tyf, ty8);
        for (uint32_t q = lane; q < 96u; q += 64u) {
            double2 *dst = reinterpret_cast<double2 *>(frame + ((size_t)(tyf + q / PIECES) * a.frame_width + tx0) * 3u);
            dst[q % PIECES] = double2{0., 0.};
        }
        if (a.frame8 && lane < 24u) {
            unsigned long long *dst = reinterpret_cast<unsigned long long *>(a.frame8 + ((size_t)(ty8 + lane / P8) * a.frame_width + tx0) * 3u);
            dst[lane % P8] = 0ull;
        }
    }
}

// The wave `id` (counted from the first render wave) of a launch with a dispatch order, behind the first round: the tile it
// renders, or ~0 -- a wave of the sky tail (which has done its work here), a wave behind the grid's end with nothing handed
// on to it, or a wait given up (the frame is void, the host is told).
// (inlined: measured against a function of its own, demo 1080p 77.1 / 74.0 against 80.4 / 80.5 us, Cornell 55.2 against 57.1)
#ifndef RM_ORDERED_TILE_INLINE
#define RM_ORDERED_TILE_INLINE __forceinline__
#endif
template <int STACK, int POW, bool STAGED, bool BVH, bool CULL, bool EDGES>
__device__ RM_ORDERED_TILE_INLINE uint32_t ordered_tile(const char *kargs_of_kernel, uint32_t id_v) {
    const unsigned long long kv = (unsigned long long)kargs_of_kernel;
    const unsigned long long ku = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(kv >> 32)) << 32) |
                                  (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)kv);
    const char *kargs = (const char *)reinterpret_cast<const __attribute__((address_space(4))) char *>(ku);
    const KernelArgs &a = *reinterpret_cast<const KernelArgs *>(kargs + sizeof(const double *));
    const uint32_t id = (uint32_t)__builtin_amdgcn_readfirstlane((int)id_v);
    const uint32_t n_dyn = (a.n_tiles >> 4) - (a.n_static >> 4), behind = 16u * (n_dyn - a.tail_patches);
    uint32_t m = id - a.n_static, k, sub;
    bool handed = false;
    if (m >= behind + a.tail_patches) {                             // behind the grid's end: sixteen waves per place a guessed tail may have to hand on
        m -= behind + a.tail_patches;
        if (m >= 16u * a.ov_cap) {                                  // ... and behind those, the workgroups that write the places of the order the next launch dispatches by
            order_places(a, m - 16u * a.ov_cap, nullptr, false, true);
            return ~0u;
        }
        k = n_dyn - a.tail_patches + (m >> 4);
        sub = m & 15u;
        handed = true;
    } else {
        if (a.tail_patches) {
            // Sky tail: the last tail_patches places of the order get ONE wave each instead of sixteen.  Behind the first round
            // those waves are dealt out evenly among the others (a burst of them -- 24 MB of stores in a few microseconds -- holds
            // up every load of the waves that compute): position m is the tail's when floor(m q / 2^32) steps there, q = ceil(tail
            // 2^32 / positions) from the host (0: the tail is all there is; 1: the tail behind every tile wave -- frames that are
            // mostly sky, whose few tiles with something to hit must not wait for a slot behind waves that only store)
            const uint32_t before = a.tail_q == 1u ? (m >= behind ? m - behind : 0u) : a.tail_q ? __umulhi(m, a.tail_q) : min(m, a.tail_patches);
            const bool mine = a.tail_q == 1u ? m >= behind : a.tail_q ? __umulhi(m + 1u, a.tail_q) > before : m < a.tail_patches;
            if (mine) {
                sky_tail_patch<STACK, POW, STAGED, BVH, CULL, EDGES>(kargs_of_kernel, before);
                return ~0u;
            }
            m -= before;
        }
        k = m >> 4;
        sub = 15u - (m & 15u);
    }
    bool sky, last_resort;
    const uint32_t patch = order_entry(a, k, sky, last_resort);
    // (a place a guessed tail did not have to hand on: its own wave has stored the sky's zeros -- or, with the order of last
    // resort, rendered whatever the patch holds by itself)
    if (patch == ~0u || (handed && (sky || last_resort))) return ~0u;
    return patch * 16u + sub;
}

// A classifying workgroup (rm_classify.inc): `id` of the launch's first cls_blocks.  Four patches at a time -- sixteen lanes to a
// patch -- bottom-up like the first round; with a dispatch order, their slots in it, and (once every classifying workgroup has
// arrived) their places.  Returns the diagnostic build's phase stamps.
// (inlined: as a function of its own it is given 150 vector registers -- the classification's doubles -- and a kernel's budget
// is the largest of its functions': three waves to a SIMD instead of four; a function's budget cannot be set, a kernel's can)
#ifndef RM_CLASSIFY_WG_INLINE
#define RM_CLASSIFY_WG_INLINE __forceinline__
#endif
template <bool ORDER, bool STAGED>
__device__ RM_CLASSIFY_WG_INLINE unsigned long long classify_workgroup(const char *kargs_of_kernel, uint32_t id_v, unsigned long long t_start) {
    const unsigned long long kv = (unsigned long long)kargs_of_kernel;
    const unsigned long long ku = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(kv >> 32)) << 32) |
                                  (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)kv);
    const char *kargs = (const char *)reinterpret_cast<const __attribute__((address_space(4))) char *>(ku);
    const double *__restrict__ scene_blob = *reinterpret_cast<const double *const *>(kargs);
    const KernelArgs &a = *reinterpret_cast<const KernelArgs *>(kargs + sizeof(const double *));
    const uint32_t id = (uint32_t)__builtin_amdgcn_readfirstlane((int)id_v);
    unsigned long long stats = 0ull;
    (void)t_start;
    const uint32_t n_patches = a.n_tiles >> 4;
    const bool bottom_up = a.order_mul == a.n_tiles - 1u && a.order_add == a.n_tiles - 1u && a.n_tiles > 1u;
    const bool ordering = ORDER && a.ord_cnt;
    // (where the launch dispatches by the order it lays out itself, every wave behind the first round waits for the slowest of these)
    if (ordering && a.ord_read == a.ord_flat) __builtin_amdgcn_s_setprio(3);
    // What a lane's chain of tests waits for is memory: every primitive's bounds and edges are a load away, one after the other
    // (the Cornell box: eight tests in a row, 14 us -- the tests themselves are a tenth of that).  Where the scene fits the
    // workgroup's block (it renders nothing: the block is free) the tests read the copy every render wave makes anyway.
    // What the first patches' tests and their slots wait for, asked for before anything else is waited for: the table values at the
    // patches' and tiles' corners, the patches' words in the index, the previous frame's cost table (a workgroup's first
    // microseconds were four round trips one after the other -- arguments, scene copy, the patch's corners, the tile's -- each over
    // a microsecond at a launch's start).
    const uint32_t iters = ordering ? a.cls_iters : 1u;
    auto patch_of = [&](uint32_t it, bool &valid) {
        const uint32_t q = (it * a.cls_blocks + id) * 4u + ((threadIdx.x & 63u) >> 4);
        valid = q < n_patches;
        return !valid ? 0u : bottom_up ? n_patches - 1u - q : q;     // (every patch once, whatever the tile order)
    };
    bool valid;
    uint32_t patch = patch_of(0u, valid);
    ClsAsked cls_asked = classify_ask(a, patch, valid);
    OrdAsked ord_asked{0u, 0u, 0u};
    if (ordering) ord_asked = order_ask(a, patch, valid);
    // (cost by content: the table of the previous frame, lane p the primitive p's mean tile time; ~0: a primitive no sampled tile
    // of that frame reached)
    uint32_t ct_sum = 0u, ct_num = 0u;
    if (ordering && a.key_mode == RM_KEY_CONTENT) { ct_sum = a.ctab[threadIdx.x & 63u]; ct_num = a.ctab[64u + (threadIdx.x & 63u)]; }
    // (scenes too long for a copy: only what the tests read, packed -- where the host found room for it, cls_lds_words)
#ifndef RM_CLASSIFY_FROM_MEMORY
    ClsView blob;
    OrdRec *rec;
    if (STAGED) {
        stage_scene(scene_blob, a.H);
        blob = cls_view_of_blob(rm_lds, a.H);
        rec = reinterpret_cast<OrdRec *>(rm_lds + a.H.total_words);
    } else if (a.cls_lds_words) {                                    // wave-uniform
        blob = cls_stage(scene_blob, a.H, rm_lds);
        rec = reinterpret_cast<OrdRec *>(rm_lds + a.cls_lds_words);
    } else {
        blob = cls_view_of_blob(scene_blob, a.H);
        rec = reinterpret_cast<OrdRec *>(rm_lds);
    }
#else
    const ClsView blob = cls_view_of_blob(scene_blob, a.H);
    OrdRec *rec = reinterpret_cast<OrdRec *>(rm_lds);
#endif
    const uint32_t prim_cost = !(ordering && a.key_mode == RM_KEY_CONTENT) ? 0u : ct_num ? (ct_sum / ct_num) << 6 : ~0u;
    if (ordering && id == 0u) {                                      // (what the next launch counts into: nobody of this one looks at it)
        if (a.ord_cnt_next) for (uint32_t i = threadIdx.x & 63u; i < RM_ORD_CNT_WORDS; i += 64u) a.ord_cnt_next[i] = 0u;
        if (a.ctab_zero) for (uint32_t i = threadIdx.x & 63u; i < RM_CTAB_WORDS; i += 64u) a.ctab_zero[i] = 0u;
    }
    for (uint32_t it = 0; it < iters; it++) {                        // wave-uniform
        // (the next turn's values travel while this turn's patches are classified)
        bool valid_next = false;
        uint32_t patch_next = 0u;
        ClsAsked cls_next = cls_asked;
        OrdAsked ord_next = ord_asked;
        if (it + 1u < iters) {
            patch_next = patch_of(it + 1u, valid_next);
            cls_next = classify_ask(a, patch_next, valid_next);
            ord_next = order_ask(a, patch_next, valid_next);
        }
        unsigned long long sig, own;
        (void)classify_patches<true>(blob, a, patch, valid, cls_asked, const_cast<unsigned long long *>(a.tile_mask), a.cls_prims, a.mask_tag, sig, own);
#ifdef RM_EXP_STAMPS
        if (it + 1u == iters) stats = (__builtin_amdgcn_s_memrealtime() - t_start) & 0xFFFFFull;            // classified
#endif
        if (ordering) order_slot(a, id, patch, valid, sig, a.mask_exact ? own : ~0ull, prim_cost, ord_asked, rec + it * 4u, a.ord_rec ? a.ord_rec + (size_t)(it * a.cls_blocks + id) * 12u : nullptr);
        patch = patch_next; valid = valid_next; cls_asked = cls_next; ord_asked = ord_next;
    }
    if (ordering) {
        __builtin_amdgcn_wave_barrier();
#ifdef RM_EXP_STAMPS
        stats |= ((__builtin_amdgcn_s_memrealtime() - t_start) & 0xFFFFFull) << 20;                          // its patches have their slots
#endif
        // (a launch that dispatches by its predecessor's order: the places are written at the grid's end, nobody waits here)
        order_places(a, id, rec, true, a.ord_rec == nullptr);
    }
    return stats;
}

// ---- the kernel ------------------------------------------------------------------
// ORDER: the dispatch order from the launch's own classification and the sky tail (KernelArgs::ord_*) compiled in; launches that
// cannot use them run the kernel without (what every wave carries for them costs such a launch 2-3 %).
// One workgroup = one wave = one tile (WAVES = TPW = 1 is the only geometry instantiated: the
// waves of a workgroup share nothing but the LDS scene copy, and slots freed by a workgroup of
// several waves are handed on only when a whole workgroup fits).  The hardware dispatcher
// balances the load across workgroups.
// Register budget: with the integer specular power the kernel is held to 128 VGPRs (4 waves
// per SIMD).  The generic pow flavour needs ~168 (its constants, see specular_pow) and is left alone.
// The kernels with the cull's edge test get 170 (3 waves per SIMD): at 128 they spill 19 values around
// the cull step -- the Cornell frame then WROTE 82.4 MB per launch for the 54.7 MB of its frames -- and
// with the tiles classified the fourth wave buys nothing (Cornell 43.0 / 43.6 us, WRITE_SIZE 57.0 MB).
// STAGED = false: scenes too large for an LDS copy -- the per-lane gathers read the blob
// in global memory as well (the uniform walk always does).
template <int STACK, int POW, int WAVES, int TPW, bool STAGED = true, bool BVH = false, bool CULL = false, bool EDGES = false, bool ORDER = false, bool FEEDBACK = false>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(POW == POW_INTEGER ? (EDGES ? RM_EDGES_WAVES : RM_MIN_WAVES) : 1, 8))) void rm_render_static(const double *__restrict__ scene_blob, KernelArgs a,
                                                              double *__restrict__ frame) {
    static_assert(WAVES == 1 && TPW == 1, "one tile per wave, one wave per workgroup");
#ifdef RM_EXP_STAMPS   // diagnostic build: wave start / end times, hardware slot, ray-step counts, to a buffer of their own
    const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
    unsigned long long tile_stats = 0;
    uint32_t cull_counts[4] = {0u, 0u, 0u, 0u};
    uint32_t st_tile = ~0u;                                         // the tile rendered (~0: a wave that renders none)
    unsigned long long st_mask = ~0ull;                             // its classification word (~0: none)
    auto stamp = [&]() {
        if ((threadIdx.x & 63u) == 0 && a.debug_stamps) {
            unsigned long long *o = a.debug_stamps + 4ull * blockIdx.x;
            o[0] = t_start; o[1] = tile_stats; o[2] = __builtin_amdgcn_s_memrealtime();
            // (behind the grid's four-word records: tile and mask, two words per wave -> <file>.ext)
            unsigned long long *x = a.debug_stamps + 4ull * gridDim.x + 2ull * blockIdx.x;
#if defined(RM_EXP_WALKSTATS) || defined(RM_EXP_PHASES) || defined(RM_EXP_STARTUP)
            o[3] = (unsigned long long)cull_counts[0] | ((unsigned long long)cull_counts[1] << 32);
            x[0] = st_tile; x[1] = (unsigned long long)cull_counts[2] | ((unsigned long long)cull_counts[3] << 32);
#else
            o[3] = (unsigned long long)cull_counts[0] | ((unsigned long long)cull_counts[1] << 16) |
                   ((unsigned long long)cull_counts[2] << 40) | ((unsigned long long)cull_counts[3] << 52);
            x[0] = st_tile; x[1] = st_mask;
#endif
        }
    };
#else
    auto stamp = []() {};
#endif
    // (compiled into the kernels that can use it only: its few live scalars cost the others 4 %)
    const bool feedback = FEEDBACK && a.fb_flag != nullptr;        // wave-uniform
    if (feedback && blockIdx.x == 0u) {
        // The launch's first wave: clears the counter and histogram of the frame after next, and
        // turns the previous frame's histogram into this frame's threshold -- the lower edge of the
        // bucket from which on at most fb_target tiles lie (lane b: bucket b; one scan from the
        // top).  A wave that reads the threshold before it is written sees the previous frame's:
        // it is a hint either way.
        const uint32_t b = threadIdx.x;
        a.fb_zero[b] = 0u;                                          // hist[64] | count
        if (b == 0u) a.fb_zero[RM_FB_BUCKETS] = 0u;
        if (a.fb_target != 0u) {
            uint32_t above = a.fb_hist[b] * RM_FB_SAMPLE;           // tiles in buckets >= b
            for (uint32_t off = 1u; off < 64u; off <<= 1) {
                const uint32_t o = (uint32_t)__shfl_down((int)above, off, 64);
                above += (b + off < 64u) ? o : 0u;
            }
            const unsigned long long fits = __ballot(above <= a.fb_target);
            const uint32_t first = (uint32_t)__builtin_ctzll(fits | (1ull << 63));
            const uint32_t total = (uint32_t)__shfl((int)above, 0, 64);
            if (b == 0u) *a.fb_threshold = total == 0u ? a.fb_long_ticks : max(fb_edge(first), 200u);   // (never below 2 us)
        }
    }

    // ---- which tile.  Feedback (rm_device.hip): ids below fb_cap take the previous frame's long
    // tiles, the others the tiles in dispatch order -- less those the list holds.  A tile is on
    // the list exactly where its flag is set (the same wave of the same frame wrote both).
    uint32_t id = blockIdx.x;
    // The head of the launch classifies (rm_classify.inc): workgroups are dispatched in id order, so these
    // are running before the first render wave starts, four patches each, bottom-up like the first round.
    if (a.cls_blocks) {                                             // wave-uniform
        if (id < a.cls_blocks) {
#ifdef RM_EXP_STAMPS
            tile_stats = classify_workgroup<ORDER, STAGED>((const char *)__builtin_amdgcn_kernarg_segment_ptr(), id, t_start);
#else
            (void)classify_workgroup<ORDER, STAGED>((const char *)__builtin_amdgcn_kernarg_segment_ptr(), id, 0ull);
#endif
            stamp();
            return;
        }
        id -= a.cls_blocks;
    }
    // A wave's first microseconds are a chain of loads -- its place (known after 1.07 us on the demo frame), its tile's word (+0.76),
    // the scene copy (+0.72), the primary directions (+0.35; +0.78 / +1.29 in the kernels without a copy: Cornell / 256 spheres) --
    // of which the last two need not wait for the first.  -DRM_EARLY_LOADS asks for them here and where the tile is known:
    // measured (profiles/r04_ab_notes.txt 8) 68.6 against 68.95, 32.9 against 33.2 and 1,152 against 1,143 us -- the chain is
    // hidden behind the SIMD's other three waves already, and what is held meanwhile costs the demo kernel 14 vector spills.
#ifdef RM_EARLY_LOADS
    constexpr bool EARLY = ORDER;
#else
    constexpr bool EARLY = false;
#endif
    SceneAsked scene_asked;
    if (STAGED && EARLY) scene_asked = stage_scene_ask(scene_blob, a.H);
    uint32_t tile = 0u;
    bool late = id >= a.first_round;                                // behind the launch's first round: the tile's classification is there, or about to be
    bool listed_tile = false;
    if (ORDER && a.ord_cnt && id >= a.n_static) {                   // wave-uniform: a place in the order, or in the sky tail
        // (a function of its own, not inlined: what it needs must not shape the registers of the tile that follows)
        // (its answer comes back in a vector register: said to be the same in every lane, which it is)
        tile = uniform_u32(ordered_tile<STACK, POW, STAGED, BVH, CULL, EDGES>((const char *)__builtin_amdgcn_kernarg_segment_ptr(), id));
        if (tile == ~0u) { stamp(); return; }
        late = true;
    } else if (feedback && id < a.fb_cap) {
        if (id >= min(a.fb_count[0], a.fb_cap)) { stamp(); return; }
        tile = a.fb_list[id];
        if (tile >= a.n_tiles) { stamp(); return; }                // (cannot happen: the list is per launch geometry)
        listed_tile = true;
    } else {
        if (feedback) id -= a.fb_cap;
        if (id >= a.n_tiles) { stamp(); return; }                   // wave-uniform
        // (the first round of a launch with an order: the first places of the previous launch's, where there was one)
        // (both words asked for at once: whether there is a list, and the entry)
        if (ORDER && a.ord_cnt && a.static_list && a.lists_done) {
            const uint32_t done = *a.lists_done, cand = a.static_list[id >> 4];
            tile = done == a.lists_tag ? cand * 16u + (15u - (id & 15u)) : tile_of_id(a, id);
        } else {
            tile = tile_of_id(a, id);
        }
    }
#if defined(RM_EXP_STAMPS) && defined(RM_EXP_STARTUP)   // (where a wave's first microseconds go: ticks since its start, sixteen bits each)
    cull_counts[3] = (uint32_t)t_start;
    cull_counts[0] = ((uint32_t)__builtin_amdgcn_s_memrealtime() - cull_counts[3]) & 0xFFFFu;          // the tile is known
#endif
    // What the tile's first instructions wait for is requested up front, all at once: the flag, the
    // backproject values of the lane's column and row, the threshold -- and, below, the scene copy.
    const uint32_t flagged = (feedback && !listed_tile) ? a.fb_flag[tile] : 0u;
    uint32_t tx0, ty0, tyf, ty8;
    tile_origin(a, tile, tx0, ty0, tyf, ty8);
    // (only where there is a flag to wait for: ahead of the scene copy of the small-scene kernels
    // these loads were measured at +0.8 % on the 1080p demo frame and +1.6 % at 8K)
    double bp_x = 0., bp_y = 0.;
    if (FEEDBACK || EARLY) { bp_x = a.bp_x[tx0 + ((threadIdx.x & 63u) % TILE_W)]; bp_y = a.bp_y[ty0 + ((threadIdx.x & 63u) / TILE_W)]; }
    // (the threshold is read here, not where it is used: at the end of the tile the wave would
    // wait for it with its slot taken and nothing else to do)
    uint32_t fb_thr = a.fb_long_ticks;
    if (feedback && a.fb_target != 0u) {
        fb_thr = __hip_atomic_load(a.fb_threshold, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        fb_thr = fb_thr ? fb_thr : a.fb_long_ticks;
    }
    if (flagged) { stamp(); return; }                               // the list holds this tile

    // Classified tiles (rm_classify.hip): a mask of zero says no primary ray of the tile can hit anything --
    // the wave stores the primary-miss value and leaves: no scene copy, no ray, no walk.
    bool have_mask = a.tile_mask != nullptr && a.mask_exact != 0u;           // wave-uniform
    unsigned long long first_mask = ~0ull;
    if (a.tile_mask && a.mask_tag) {
        // classified at the head of this launch: the tile's word is there once it carries the launch's tag.  The
        // waves of the launch's first round do not wait for it (their tiles are walked unclassified: the bottom
        // rows, nothing of which is sky in the reference's scenes), later ones find it written; a wave that
        // does not within 20 us goes on without -- a mask only ever spares work.
        have_mask = false;
        if (late || a.mask_tag_prev) {                              // (the first round: what is resident at once, 256 CUs x 4 SIMDs x 4 waves, 3 in the edge-test kernels)
            unsigned long long *word = const_cast<unsigned long long *>(a.tile_mask) + tile;
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
            if (a.mask_tag_prev) {                                  // (the word of a launch that is over, or this launch's: a scalar load will do)
                const unsigned long long w = a.tile_mask[tile];
                if ((uint32_t)(w >> 56) == a.mask_tag || (uint32_t)(w >> 56) == a.mask_tag_prev) { first_mask = w & 0x00FFFFFFFFFFFFFFull; have_mask = true; }
            }
            while (!have_mask) {
                // (every lane reads the one word: said so, the mask is a scalar and the walk over its primitives a scalar loop with
                // scalar record loads, like the plain walk -- as a vector value it made that walk a per-lane loop with vector loads)
                const unsigned long long w = uniform_u64(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                if ((uint32_t)(w >> 56) == a.mask_tag || (a.mask_tag_prev && (uint32_t)(w >> 56) == a.mask_tag_prev)) { first_mask = w & 0x00FFFFFFFFFFFFFFull; have_mask = true; break; }
                if (__builtin_amdgcn_s_memrealtime() - t0 > 2000ull) break;          // 100 MHz ticks
                __builtin_amdgcn_s_sleep(4);
            }
        }
    } else if (a.tile_mask) {
        first_mask = uniform_u64(a.tile_mask[tile]);
    }
    if (a.tile_mask) {
        if (first_mask == 0ull && !listed_tile) {                  // (a tile the feedback list holds goes the long way: its wave owns the tile's flag)
            const uint32_t lane = threadIdx.x & 63u;
            constexpr uint32_t PIECES = TILE_W * 3u / 2u, P8 = TILE_W * 3u / 8u;
            for (uint32_t q = lane; q < 96u; q += 64u) {
                double2 *dst = reinterpret_cast<double2 *>(frame + ((size_t)(tyf + q / PIECES) * a.frame_width + tx0) * 3u);
                dst[q % PIECES] = double2{0., 0.};
            }
            if (a.frame8 && lane < 24u) {
                unsigned long long *dst = reinterpret_cast<unsigned long long *>(a.frame8 + ((size_t)(ty8 + lane / P8) * a.frame_width + tx0) * 3u);
                dst[lane % P8] = 0ull;
            }
            if (feedback && (threadIdx.x & 63u) == 0u) a.fb_next_flag[tile] = 0;
            stamp();
            return;
        }
    }

#ifdef RM_EXP_STAMPS
    st_tile = tile; st_mask = have_mask ? first_mask : ~0ull;
#endif
    // (a scene of more than 64 primitives: the word only says whether there is anything to hit -- not what the walk may leave out)
    have_mask = have_mask & (a.mask_exact != 0u);
#if defined(RM_EXP_STAMPS) && defined(RM_EXP_STARTUP)
    cull_counts[0] |= (((uint32_t)__builtin_amdgcn_s_memrealtime() - cull_counts[3]) & 0xFFFFu) << 16;  // its classification word is there
#endif
    if (STAGED) { if (EARLY) stage_scene_put(scene_asked, a.H); else stage_scene(scene_blob, a.H); }
#if defined(RM_EXP_STAMPS) && defined(RM_EXP_STARTUP)
    cull_counts[1] = ((uint32_t)__builtin_amdgcn_s_memrealtime() - cull_counts[3]) & 0xFFFFu;          // the scene copy is made
#endif
    // (scenes too long for a copy, kernels with the bundle cull: its two arrays alone, where the launch has room -- every cull
    // step of the tile then reads LDS instead of waiting for memory)
    const uint32_t cull_words = (!STAGED && CULL) ? a.cull_lds_words : 0u;                               // wave-uniform
    if (!STAGED && CULL && cull_words) { cull_stage(scene_blob, a.H, rm_lds); __syncthreads(); }
    double *wl = rm_lds + (STAGED ? a.H.total_words : cull_words);
    // (patch order: the wave's start time waits in its LDS block, not in a register that would be live through the tile)
    if (ORDER && (threadIdx.x & 63u) == 0u) reinterpret_cast<uint32_t *>(wl + RM_WAVE_T0_WORDS)[0] = (uint32_t)__builtin_amdgcn_s_memrealtime();
    // The strict plain-walk kernels render the tile with the checked numerics (RM_CHECKED_NS: this source's device functions
    // compiled once more, rm_render_kernel.hpp) and keep this namespace's tile body, behind render_patch_alone, as the exact
    // twin: a launch that is exact only (KernelArgs::exact_only) enters it at once, a tile some lane of which met an operand
    // outside the checked range is rendered again by it -- and only then stored.
#ifdef RM_CHECKED_NS
    constexpr bool CHECKED = STAGED && !BVH && !CULL;
    namespace tile_ns = RM_CHECKED_NS;
#else
    constexpr bool CHECKED = false;
    namespace tile_ns = RM_FLAVOR_NS;
#endif
    const unsigned long long fb_t0 = feedback ? __builtin_amdgcn_s_memrealtime() : 0ull;
    bool exact = CHECKED && a.exact_only != 0u;                     // wave-uniform
    if (!exact) {
        tile_ns::SceneView sc;
        if (STAGED) sc.S = rm_lds; else sc.S = scene_blob;
        sc.G = scene_blob;
        sc.cull_bounds = cull_words ? rm_lds : scene_blob + a.H.off_bounds;
        sc.cull_planar = cull_words ? rm_lds + 4u * (a.H.n_spheres + a.H.n_polygons + a.H.n_triangles) : scene_blob + a.H.off_planar;
        sc.bstack = reinterpret_cast<uint32_t *>(wl + RM_WAVE_BVH_STACK_WORDS);
        sc.cull_cos = own_sgpr(a.cull_cos);
#ifdef RM_EXP_STAMPS
        sc.cnt = cull_counts;
#endif
        // every header field in a scalar register of its own: the kernel arguments arrive as
        // 16-dword tuples, and a tuple is spilled and reloaded whole (16 lane reads to get at
        // the background colour, four times per ray)
        sc.H.n_spheres = own_sgpr(a.H.n_spheres);         sc.H.n_polygons = own_sgpr(a.H.n_polygons);
        sc.H.n_triangles = own_sgpr(a.H.n_triangles);     sc.H.n_lights = own_sgpr(a.H.n_lights);
        sc.H.off_spheres = own_sgpr(a.H.off_spheres);     sc.H.off_polygons = own_sgpr(a.H.off_polygons);
        sc.H.off_pverts = own_sgpr(a.H.off_pverts);       sc.H.off_triangles = own_sgpr(a.H.off_triangles);
        sc.H.off_materials = own_sgpr(a.H.off_materials); sc.H.off_lights = own_sgpr(a.H.off_lights);
        sc.H.off_keys = own_sgpr(a.H.off_keys);           sc.H.total_words = a.H.total_words;
        sc.H.list_ordered = own_sgpr(a.H.list_ordered);   sc.H.off_bvh_spheres = own_sgpr(a.H.off_bvh_spheres);
        sc.H.off_bvh_triangles = own_sgpr(a.H.off_bvh_triangles); sc.H.off_bounds = own_sgpr(a.H.off_bounds);
        sc.H.off_planar = own_sgpr(a.H.off_planar);       sc.H.off_groups = own_sgpr(a.H.off_groups);
        sc.H.off_occ = own_sgpr(a.H.off_occ);
        sc.H.shadow_rho = own_sgpr(a.H.shadow_rho);

#if defined(RM_EXP_STAMPS) && defined(RM_EXP_PHASES)
        cull_counts[2] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - t_start);
#endif
#ifdef RM_EXP_STAMPS
        unsigned long long *const stats_to = &tile_stats;
#else
        unsigned long long *const stats_to = nullptr;
#endif
        if constexpr (rm_scene_sig_kernel(STAGED, BVH, CULL)) {
            // The resident scene's signature (the plan's verdict, bits of a word the tile reads anyway: asked for here, used
            // here, live nowhere else): the body compiled for its counts, or the body for any scene -- wave-uniform, once a tile.
            const uint32_t sig = (a.dead_children >> RM_SCENE_SIG_SHIFT) & RM_SCENE_SIG_MASK;
            exact = tile_ns::render_tile_of<RM_SCENE_SIG_COUNT, STACK, POW, BVH, CULL, EDGES, FEEDBACK || EARLY>(sig, sc, a, tx0, ty0, tyf, ty8, bp_x, bp_y, wl, frame, stats_to, have_mask, first_mask, (const char *)__builtin_amdgcn_kernarg_segment_ptr());
        } else {
            exact = tile_ns::render_tile<STACK, POW, BVH, CULL, EDGES, FEEDBACK || EARLY>(sc, a, tx0, ty0, tyf, ty8, bp_x, bp_y, wl, frame, stats_to, have_mask, first_mask, (const char *)__builtin_amdgcn_kernarg_segment_ptr());
        }
        if (CHECKED && exact) {                                          // (counted: tests and profiles ask how many, rm_device.hip rmi_redone_tiles)
            const KernelArgs &b = *reinterpret_cast<const KernelArgs *>(reread_kernargs((const char *)__builtin_amdgcn_kernarg_segment_ptr()) + sizeof(const double *));
            if (b.redo_count && (threadIdx.x & 63u) == 0u) atomicAdd(b.redo_count, 1u);
        }
    }
    if constexpr (CHECKED) if (exact) render_patch_alone<STACK, POW, STAGED, BVH, CULL, EDGES>((const char *)__builtin_amdgcn_kernarg_segment_ptr(), tile, 1u, true);
    if (ORDER) {
        // (the kernel's arguments read afresh from its argument segment: asked of `a` they would be kept in scalar registers
        // -- spilt ones -- through the whole tile for these few lines)
#ifdef RM_NO_REREAD
        const KernelArgs &b = a;
#else
        const KernelArgs &b = *reinterpret_cast<const KernelArgs *>(reread_kernargs((const char *)__builtin_amdgcn_kernarg_segment_ptr()) + sizeof(const double *));
#endif
        if (b.patch_cost) {                                          // what the tile took (100 MHz ticks) ...
            const uint32_t dt = min(uniform_u32((uint32_t)__builtin_amdgcn_s_memrealtime() - reinterpret_cast<const uint32_t *>(wl + RM_WAVE_T0_WORDS)[0]), 0x00FFFFFFu);
            // ... to its patch's counter: the longest tile of a patch is what the patch is sorted by while the view stands
            if ((threadIdx.x & 63u) == 0u) RM_PATCH_COST_OP(b.patch_cost + (tile >> 4), dt);
            // ... and, one tile in sixteen, to the primitives its primary rays could reach (lane b: primitive b): cost by content,
            // what the next launch sorts by when the view has moved (the tile's word is there by now, whoever waited for it)
            if ((tile & 15u) == 0u && b.ctab_cur && b.tile_mask && b.mask_tag && b.mask_exact) {
                const unsigned long long w = uniform_u64(__hip_atomic_load(const_cast<unsigned long long *>(b.tile_mask) + tile, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                if ((uint32_t)(w >> 56) == b.mask_tag && ((w >> (threadIdx.x & 63u)) & 1ull) && (threadIdx.x & 63u) < 56u) {
                    atomicAdd(b.ctab_cur + (threadIdx.x & 63u), dt >> 6);
                    atomicAdd(b.ctab_cur + 64u + (threadIdx.x & 63u), 1u);
                }
            }
        }
    }
#ifdef RM_EXP_STAMPS
    // (the tile's word as the classification left it -- the first round's waves did not wait for it, it is there by now)
    if (a.tile_mask) st_mask = __hip_atomic_load(const_cast<unsigned long long *>(a.tile_mask) + tile, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 0x00FFFFFFFFFFFFFFull;
#endif
    if (feedback) {
        const unsigned long long fb_dt = __builtin_amdgcn_s_memrealtime() - fb_t0;
        const uint32_t ticks = fb_dt < 0x7FFFFFFFull ? (uint32_t)fb_dt : 0x7FFFFFFFu;
        const bool is_long = ticks >= fb_thr;
        if ((threadIdx.x & 63u) == 0u) {
            if (a.fb_target != 0u && tile % RM_FB_SAMPLE == 0u) atomicAdd(a.fb_next_hist + fb_bucket(ticks), 1u);
            bool listed = false;
            // (the threshold keeps the long tiles to about fb_target: few waves meet at the counter.
            // Reading the counter first, to leave a full list alone, was measured: 1,247 -> 1,342 us)
            if (is_long) {
                const uint32_t slot = atomicAdd(a.fb_next_count, 1u);
                if (slot < a.fb_cap) { a.fb_next_list[slot] = tile; listed = true; }
            }
            a.fb_next_flag[tile] = listed ? 1 : 0;
        }
    }
    stamp();
}

#endif   // !RM_CHECKED

}  // namespace RM_FLAVOR_NS
