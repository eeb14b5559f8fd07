// rm_classify.inc -- the tile classification (see rm_classify.hip for what it is for), once per numeric
// flavour like rm_trace.inc (no include guard): the launch of its own (rm_classify.hip) and the head of the
// render launches (rm_render_kernel.inc) both run classify_patches().
namespace RM_FLAVOR_NS {
using namespace rmdev;

// Two steps, coarse to fine, sixteen lanes to a 32x32 patch (a wave takes four patches):
//   1. the PATCH: the cone around its 1,024 primary rays against every primitive -- lane s of the group
//      takes the primitives s, s + 16, ... -- and the lanes combine what they kept;
//   2. its sixteen TILES, lane s the s-th: the tile's own cone against the primitives the patch kept.
// Most patches keep nothing or one or two primitives, so step 2 is short; a lane's chain of tests is what
// the launch lasts (495 waves at 1080p cannot fill the chip, only get done sooner).
__device__ __forceinline__ V3 unit(V3 a) {
    // (1/sqrt from the hardware estimate and two Newton steps: relative error ~1e-16 against margins of 1e-9)
    const double x = dot(a, a);
    double y = __builtin_amdgcn_rsq(x);
    const double h = 0.5 * x;
    y = y * (1.5 - h * y * y);
    y = y * (1.5 - h * y * y);
    return scaled(a, y);
}

// The cone around the rays whose unnormalised directions fill the rectangle [bx0, bx1] x [by0, by1] x {-1}; the
// lanes of a group that shares the rectangle each take a corner (`sub`).  A cone is convex: it holds the rectangle when it
// holds its corners.  The margins are far beyond the rounding of the kernel's own normalisation of the same
// table values.  False: the cone tests do not hold for it (half-angle towards 90 degrees -- a frame of a few
// tiles -- or a camera / table value that is not a number): everything is kept.
#if RM_KERNEL_ORIENTED
// (oriented camera: the rectangle's points go through the view's linear map, (bx right + by up) + forward, as the render's rays
// do: the rectangle becomes a parallelogram in world space, still convex, its corners still its extreme points)
__device__ __forceinline__ V3 cls_dir(const KernelArgs &a, double bx, double by) {
    return mk((bx * a.cam_rx + by * a.cam_ux) + a.cam_fx, (bx * a.cam_ry + by * a.cam_uy) + a.cam_fy, (bx * a.cam_rz + by * a.cam_uz) + a.cam_fz);
}
#else
__device__ __forceinline__ V3 cls_dir(const KernelArgs &, double bx, double by) { return mk(bx, by, -1.); }
#endif
template <bool SHARED>
__device__ __forceinline__ bool cone_of(Bundle &b, const KernelArgs &a, double bx0, double bx1, double by0, double by1, uint32_t sub) {
    const V3 u = unit(cls_dir(a, 0.5 * (bx0 + bx1), 0.5 * (by0 + by1)));
    double cm;
    if (SHARED) {                                                  // the lanes of a group share the rectangle: a corner each
        cm = dot(unit(cls_dir(a, (sub & 1u) ? bx1 : bx0, (sub & 2u) ? by1 : by0)), u);
        cm = __builtin_fmin(cm, __shfl_xor(cm, 1, 64));
        cm = __builtin_fmin(cm, __shfl_xor(cm, 2, 64));
    } else {
        cm = __builtin_fmin(__builtin_fmin(dot(unit(cls_dir(a, bx0, by0)), u), dot(unit(cls_dir(a, bx1, by0)), u)),
                            __builtin_fmin(dot(unit(cls_dir(a, bx0, by1)), u), dot(unit(cls_dir(a, bx1, by1)), u)));
    }
    cm -= 1e-9;
    b.ax = a.cam_x; b.ay = a.cam_y; b.az = a.cam_z;
    b.ux = u.x; b.uy = u.y; b.uz = u.z;
    b.cos2 = cm * cm;
    // (single-precision roots, rounded towards the wider cone, as bundle_cone does)
    b.sin_t = (double)__builtin_sqrtf((float)__builtin_fmax((1. - cm) * (1. + cm), 0.)) * (1. + 1e-6) + 1e-7;
    b.chord = (double)__builtin_sqrtf((float)__builtin_fmax(2. * (1. - cm), 0.)) * (1. + 1e-6) + 1e-7;
    b.rho = 0.;                                                   // every primary ray starts AT the camera
    b.two_sided = false;
    b.narrow = true;
    return cm > 0.5;
}

// What the tests read of the scene: every primitive's bounding sphere, the planar primitives' lifted vertices, and the first six
// words of their records (normal, plane point) -- in the scene blob where it lies (global memory, or the LDS copy of the staged
// kernels), or packed into the classifying workgroup's LDS block (cls_stage below: a lane's tests are a chain of loads, two round
// trips a primitive, and at a launch's start a round trip is over a microsecond).
struct ClsView { const double *bounds, *planar, *poly, *tri; uint32_t poly_stride, tri_stride; };
__device__ __forceinline__ ClsView cls_view_of_blob(const double *blob, const rm_dev_header &H) {
    return ClsView{blob + H.off_bounds, blob + H.off_planar, blob + H.off_polygons, blob + H.off_triangles, RM_POLYGON_WORDS, RM_TRIANGLE_WORDS};
}
// (the layout cls_stage fills and rm_device.hip sizes: 4 n | 16 n_planar | 6 n_polygons | 6 n_triangles words)
__device__ __forceinline__ uint32_t cls_stage_words(const rm_dev_header &H) {
    return 4u * (H.n_spheres + H.n_polygons + H.n_triangles) + 22u * (H.n_polygons + H.n_triangles);
}
__device__ __forceinline__ ClsView cls_stage(const double *__restrict__ blob, const rm_dev_header &H, double *lds) {
    const uint32_t lane = threadIdx.x & 63u, n = H.n_spheres + H.n_polygons + H.n_triangles, npl = H.n_polygons + H.n_triangles;
    double *bounds = lds, *planar = bounds + 4u * n, *poly = planar + 16u * npl, *tri = poly + 6u * H.n_polygons;
    cull_stage(blob, H, lds);                                       // (the bundle cull's two arrays, as the render waves pack them)
    for (uint32_t i = lane; i < 3u * H.n_polygons; i += 64u)
        reinterpret_cast<double2 *>(poly)[i] = reinterpret_cast<const double2 *>(blob + H.off_polygons + RM_POLYGON_WORDS * (i / 3u))[i % 3u];
    for (uint32_t i = lane; i < 3u * H.n_triangles; i += 64u)
        reinterpret_cast<double2 *>(tri)[i] = reinterpret_cast<const double2 *>(blob + H.off_triangles + RM_TRIANGLE_WORDS * (i / 3u))[i % 3u];
    __syncthreads();
    return ClsView{bounds, planar, poly, tri, 6u, 6u};
}

// One primitive against a cone of primary rays: true = keep.
template <bool EDGES>
__device__ __forceinline__ bool keeps(const ClsView &v, const KernelArgs &a, const Bundle &b, uint32_t pid, bool in) {
    const uint32_t ns = a.H.n_spheres, np = a.H.n_polygons;
    const double2 *bp = reinterpret_cast<const double2 *>(v.bounds) + 2u * (in ? pid : 0u);
    const SphereCull sph = cull_sphere(bp, b);
    bool out = sph.out;
    const bool planar = in & (pid >= ns);
    if (EDGES && __any(planar)) {
        const double2 *pp = reinterpret_cast<const double2 *>(v.planar) + 8u * (planar ? pid - ns : 0u);
        out = out | cull_edges(pp, b, sph, planar & !out);
        // The plane itself: a hit needs dist = num / dotprod >= 0 (polygon.rs:71-76, triangle.rs:62-67), num =
        // (plane point - origin) . normal the same for every primary ray, dotprod = dir . normal within
        // chord |normal| of axis . normal.  Signs that differ for the whole cone: no ray of it hits (what bounds
        // a primitive whose lifted hull no sphere holds -- a wall along z).
        // (a primitive that is not planar reads the bounds' first words: in bounds, never used)
        const double *recw = !planar ? v.bounds : pid < ns + np ? v.poly + v.poly_stride * (pid - ns) : v.tri + v.tri_stride * (pid - ns - np);
        const double2 *rec = reinterpret_cast<const double2 *>(recw);
        const double2 r0 = rec[0], r1 = rec[1], r2 = rec[2];      // nx ny | nz px | py pz
        const double nn = (double)__builtin_sqrtf((float)(r0.x * r0.x + r0.y * r0.y + r1.x * r1.x)) * (1. + 1e-6);   // >= |normal|
        const double num = (r1.y - b.ax) * r0.x + (r2.x - b.ay) * r0.y + (r2.y - b.az) * r1.x;
        const double un = b.ux * r0.x + b.uy * r0.y + b.uz * r1.x, spread = (b.chord + 1e-7) * nn;
        const double tiny = 1e-9 * nn * (__builtin_fabs(r1.y - b.ax) + __builtin_fabs(r2.x - b.ay) + __builtin_fabs(r2.y - b.az)) + 1e-290;
        const bool away = ((num > tiny) & (un + spread < 0.)) | ((num < -tiny) & (un - spread > 0.));
        out = out | (planar & away);
    }
    return in & !out;
}

// Two primitives against one cone, side by side (-DRM_CLASSIFY_TWO_CHAINS): a lane's tests are one long chain of dependent
// double-precision operations (a test of a triangle: ~150 of them) -- two chains in one stretch of code fill the gaps of each
// other.  The same tests as keeps(), primitive for primitive.  Measured: the Cornell box classified after p50 7.2 / max 15.2 us
// either way -- what a classifying workgroup waits for is memory, not its own arithmetic -- and the kernels held to 128 registers
// spill 29 of them for it.  Compiled out.
template <bool EDGES>
__device__ __forceinline__ void keeps2(const ClsView &v, const KernelArgs &a, const Bundle &b, uint32_t pid_a, bool in_a, uint32_t pid_b, bool in_b,
                                       bool &keep_a, bool &keep_b) {
    const uint32_t ns = a.H.n_spheres, np = a.H.n_polygons;
    const double2 *bounds = reinterpret_cast<const double2 *>(v.bounds);
    const SphereCull sph_a = cull_sphere(bounds + 2u * (in_a ? pid_a : 0u), b), sph_b = cull_sphere(bounds + 2u * (in_b ? pid_b : 0u), b);
    bool out_a = sph_a.out, out_b = sph_b.out;
    const bool planar_a = in_a & (pid_a >= ns), planar_b = in_b & (pid_b >= ns);
    if (EDGES && __any(planar_a | planar_b)) {
        const double2 *planar = reinterpret_cast<const double2 *>(v.planar);
        EdgeCull ea = cull_edges_begin(planar + 8u * (planar_a ? pid_a - ns : 0u), b, sph_a, planar_a & !out_a);
        EdgeCull eb = cull_edges_begin(planar + 8u * (planar_b ? pid_b - ns : 0u), b, sph_b, planar_b & !out_b);
        if (__any((ea.nv == 4u) | (eb.nv == 4u))) { cull_edges_fourth(ea, b); cull_edges_fourth(eb, b); }
        out_a = out_a | cull_edges_end(ea, b, planar_a & !out_a);
        out_b = out_b | cull_edges_end(eb, b, planar_b & !out_b);
        // (the plane itself: see keeps())
        auto away = [&](uint32_t pid, bool planar_p) {
            const double *recw = !planar_p ? v.bounds : pid < ns + np ? v.poly + v.poly_stride * (pid - ns) : v.tri + v.tri_stride * (pid - ns - np);
            const double2 *rec = reinterpret_cast<const double2 *>(recw);
            const double2 r0 = rec[0], r1 = rec[1], r2 = rec[2];      // nx ny | nz px | py pz
            const double nn = (double)__builtin_sqrtf((float)(r0.x * r0.x + r0.y * r0.y + r1.x * r1.x)) * (1. + 1e-6);   // >= |normal|
            const double num = (r1.y - b.ax) * r0.x + (r2.x - b.ay) * r0.y + (r2.y - b.az) * r1.x;
            const double un = b.ux * r0.x + b.uy * r0.y + b.uz * r1.x, spread = (b.chord + 1e-7) * nn;
            const double tiny = 1e-9 * nn * (__builtin_fabs(r1.y - b.ax) + __builtin_fabs(r2.x - b.ay) + __builtin_fabs(r2.y - b.az)) + 1e-290;
            return planar_p & (((num > tiny) & (un + spread < 0.)) | ((num < -tiny) & (un - spread > 0.)));
        };
        const bool away_a = away(pid_a, planar_a), away_b = away(pid_b, planar_b);
        out_a = out_a | away_a;
        out_b = out_b | away_b;
    }
    keep_a = in_a & !out_a;
    keep_b = in_b & !out_b;
}

// A wave's four patches: lanes 16 g .. 16 g + 15 take `patch` (the same for the sixteen), lane s of them the
// patch's tile s.  `tag` != 0: the word written is (tag << 56) | mask -- scenes of up to 56 primitives; a
// reader in the same launch knows the tile's word by its tag (rm_render_kernel.inc).
// `sig`: what the patch's tiles can reach between them (the lane group's sixteen masks or-ed; 0: the sky); `own`: the lane's tile's mask.
// The unnormalised direction components at the corners of the lane's patch and of its tile (the host's tables): eight loads that
// depend on nothing but the patch -- asked for ahead of whatever else the workgroup waits for first (its copy of the scene).
struct ClsAsked { double px0, px1, py0, py1, tx0, tx1, ty0, ty1; };
__device__ __forceinline__ ClsAsked classify_ask(const KernelArgs &a, uint32_t patch, bool valid) {
    const uint32_t tile = (valid ? patch : 0u) * 16u + (threadIdx.x & 15u);
    uint32_t tx0, ty0, tyf, ty8;
    tile_origin(a, tile, tx0, ty0, tyf, ty8);
    const uint32_t px0 = tx0 & ~31u, py0 = ty0 & ~31u;            // the patch's corner
    return ClsAsked{a.bp_x[px0], a.bp_x[px0 + 31u], a.bp_y[py0], a.bp_y[py0 + 31u],
                    a.bp_x[tx0], a.bp_x[tx0 + TILE_W - 1u], a.bp_y[ty0], a.bp_y[ty0 + TILE_H - 1u]};
}
template <bool EDGES>
__device__ __forceinline__ bool classify_patches(const ClsView &scene_blob, const KernelArgs &a, uint32_t patch, bool valid, const ClsAsked &asked,
                                                 unsigned long long *__restrict__ tile_mask, uint32_t n, uint32_t tag, unsigned long long &sig, unsigned long long &own) {
    const uint32_t lane = threadIdx.x & 63u, sub = lane & 15u;
    const uint32_t tile = (valid ? patch : 0u) * 16u + sub;       // lane s: tile s of the patch

    // ---- 1. the patch
    Bundle b;
    const bool patch_usable = cone_of<true>(b, a, asked.px0, asked.px1, asked.py0, asked.py1, sub);
    unsigned long long pm = 0ull;
#ifdef RM_CLASSIFY_TWO_CHAINS
    for (uint32_t base = 0; base < n; base += 32u) {               // wave-uniform trip count; two primitives a lane and turn
        const uint32_t pid_a = base + sub, pid_b = base + 16u + sub;
        const bool in_a = pid_a < n, in_b = pid_b < n;
        bool keep_a, keep_b;
        keeps2<EDGES>(scene_blob, a, b, pid_a, in_a, pid_b, in_b, keep_a, keep_b);
        pm |= (in_a & (keep_a | !patch_usable)) ? (1ull << (pid_a & 63u)) : 0ull;
        pm |= (in_b & (keep_b | !patch_usable)) ? (1ull << (pid_b & 63u)) : 0ull;
    }
#else
    for (uint32_t base = 0; base < n; base += 16u) {               // wave-uniform trip count
        const uint32_t pid = base + sub;
        const bool in = pid < n;
        const bool keep = in & (keeps<EDGES>(scene_blob, a, b, pid, in) | !patch_usable);
        pm |= keep ? (1ull << (pid & 63u)) : 0ull;
    }
#endif
    auto group_or = [](unsigned long long v) {                     // over the sixteen lanes of a group
        for (uint32_t off = 1u; off < 16u; off <<= 1) {
            const uint32_t lo = (uint32_t)v | (uint32_t)__shfl_xor((int)(uint32_t)v, (int)off, 64);
            const uint32_t hi = (uint32_t)(v >> 32) | (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), (int)off, 64);
            v = ((unsigned long long)hi << 32) | lo;
        }
        return v;
    };
    pm = group_or(pm);                                             // the group's lanes combine what they kept

    // ---- 2. its tiles, against what the patch kept (scenes of more than 64 primitives stop at the patch:
    // a mask cannot name them, it only says whether there is anything)
    // (a tagged word has 56 bits for primitives: with more than that it, too, only says whether there is anything --
    // found by the fuzz with the order forced on: 64 primitives, the last eight cut off by the tag, their tiles taken for sky)
    unsigned long long mask = 0ull;
    if (n > (tag ? 56u : 64u)) {
        mask = pm != 0ull ? ~0ull : 0ull;
    } else if (__any(pm != 0ull)) {
        const bool tile_usable = cone_of<false>(b, a, asked.tx0, asked.tx1, asked.ty0, asked.ty1, sub);
        unsigned long long m = pm;
#ifdef RM_CLASSIFY_TWO_CHAINS
        while (__any(m != 0ull)) {                                 // two of what the patch kept a turn
            const bool in_a = m != 0ull;
            const uint32_t pid_a = in_a ? (uint32_t)__builtin_ctzll(m) : 0u;
            m &= m - 1ull;
            const bool in_b = m != 0ull;
            const uint32_t pid_b = in_b ? (uint32_t)__builtin_ctzll(m) : 0u;
            m &= m - 1ull;
            bool keep_a, keep_b;
            keeps2<EDGES>(scene_blob, a, b, pid_a, in_a, pid_b, in_b, keep_a, keep_b);
            mask |= (in_a & (keep_a | !tile_usable)) ? (1ull << pid_a) : 0ull;
            mask |= (in_b & (keep_b | !tile_usable)) ? (1ull << pid_b) : 0ull;
        }
#else
        while (__any(m != 0ull)) {
            const bool in = m != 0ull;
            const uint32_t pid = in ? (uint32_t)__builtin_ctzll(m) : 0u;
            m &= m - 1ull;
            const bool keep = in & (keeps<EDGES>(scene_blob, a, b, pid, in) | !tile_usable);
            mask |= keep ? (1ull << pid) : 0ull;
        }
#endif
    }
    if (valid) {
        if (tag) __hip_atomic_store(tile_mask + tile, ((unsigned long long)tag << 56) | (mask & 0x00FFFFFFFFFFFFFFull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else tile_mask[tile] = mask;
    }
    own = valid ? mask : 0ull;
    sig = group_or(own);
    return sig != 0ull;                                          // (the lane's patch: some tile of it has something to hit)
}

// ---- the dispatch order, built while the launch's first round renders (KernelArgs::ord_*) ------------------------
// Which of the fifteen buckets of patches with something to hit: 0 goes first.  Costs are tile times in 100 MHz ticks,
// two buckets per octave from 5 us up (5 7 10 14 20 29 41 58 82 116 ... us): absolute, so a launch needs nothing from
// its predecessors to read them.  List scheduling of measured tile times (profiles/sim_keys.py) finds eight buckets as
// good as a full sort to within a microsecond.
__device__ __forceinline__ uint32_t cost_bucket(uint32_t ticks) {
    if (ticks < 512u) return RM_ORD_SKY - 1u;
    const uint32_t e = 31u - (uint32_t)__builtin_clz(ticks);         // ticks in [2^e, 2^(e+1)), e >= 9
    const uint32_t b = 2u * (e - 9u) + ((ticks >> (e - 1u)) & 1u);
    return RM_ORD_SKY - 1u - min(b, RM_ORD_SKY - 1u);
}

// ---- a classifying workgroup of a launch with a dispatch order (KernelArgs::ord_*) ----------------------------------
// What it keeps of a lane group's patch between the two halves of its work (LDS, one record per group and iteration).
struct OrdRec { uint32_t patch, bucket_slot, index; };                // counter (bucket x RM_ORD_SUBS + sub) << 24 | slot; dyn_index's word (bit 31: first round)

// First half, per group of four patches: each patch's bucket, and its slot in it -- ONE atomic per bucket present among
// the wave's (up to four) patches: 64 lanes, or 495 waves, adding to one word take their turns (measured: 20 us).
// `own`: the lane's tile's mask (cost by content: a tile is as dear as the dearest primitive it can reach, a patch as its
// dearest tile); `prim_cost`: lane p holds primitive p's cost.
// What order_slot reads of the launch's memory for a patch, asked for BEFORE the patch is classified (three loads, two of them one
// after the other, were 2-3 us between a workgroup's classification and its slots -- and every wave behind the first round waits
// for the slowest workgroup): whether there is a list, the patch's word in it, its time in the previous frame.
struct OrdAsked { uint32_t done, index, cost; };
__device__ __forceinline__ OrdAsked order_ask(const KernelArgs &a, uint32_t patch, bool valid) {
    OrdAsked q;
    q.done = (a.static_list && a.lists_done) ? *a.lists_done : 0u;
    q.index = a.dyn_index ? a.dyn_index[valid ? patch : 0u] : 0u;
    q.cost = (a.key_mode == RM_KEY_COST && a.cost_prev) ? a.cost_prev[valid ? patch : 0u] : 0u;
    return q;
}
__device__ __forceinline__ void order_slot(const KernelArgs &a, uint32_t id, uint32_t patch, bool valid, unsigned long long sig, unsigned long long own, uint32_t prim_cost, const OrdAsked &asked, OrdRec *rec, uint32_t *grec) {
    const uint32_t lane = threadIdx.x & 63u, n_patches = a.n_tiles >> 4, n_dyn = n_patches - (a.n_static >> 4);
    uint32_t c = 0u;
    if (a.key_mode == RM_KEY_CONTENT) {                              // wave-uniform
        unsigned long long m = (valid && own != ~0ull) ? own : 0ull;
        bool unseen = false;
        while (__any(m != 0ull)) {
            const bool in = m != 0ull;
            const uint32_t pid = in ? (uint32_t)__builtin_ctzll(m) : 0u;
            const uint32_t v = (uint32_t)__shfl((int)prim_cost, (int)pid, 64);   // (lane pid holds primitive pid's: classify_workgroup)
            m &= m - 1ull;
            unseen = unseen | (in & (v == ~0u));
            c = max(c, (in && v != ~0u) ? v : 0u);
        }
        c = unseen ? 0x00FFFFFFu : c;                                 // a primitive the previous frame did not see: first, to be on the safe side
        for (uint32_t off = 1u; off < 16u; off <<= 1) c = max(c, (uint32_t)__shfl_xor((int)c, (int)off, 64));
    } else if (a.key_mode == RM_KEY_COST) {
        c = asked.cost;
    }
    const bool leader = (lane & 15u) == 0u;
    // (the patches of the first round have their places already: bit 31 of their word; without a list, the bottom rows)
    const bool have_lists = a.static_list && a.lists_done && uniform_u32(asked.done) == a.lists_tag;      // (lists_ok, the word asked for ahead)
    const uint32_t index = !valid ? RM_ORD_STATIC_BIT : have_lists ? asked.index : patch < n_dyn ? 0u : RM_ORD_STATIC_BIT | (n_patches - 1u - patch);
    const bool placed = valid & leader & !(index & RM_ORD_STATIC_BIT), first_round = valid & leader & ((index & RM_ORD_STATIC_BIT) != 0u);
    // RM_KEY_PLACE: bands of the bottom-up order every launch had before there was anything to go by
    const uint32_t bucket = sig == 0ull ? RM_ORD_SKY
                          : a.key_mode == RM_KEY_PLACE ? (uint32_t)(((unsigned long long)(n_patches - 1u - patch) * (RM_ORD_SKY)) / n_patches)
                                                       : cost_bucket(c);
    // (the patches of this launch's first round are counted too, by bucket, in counters of their own: the NEXT launch's first
    // round is the dearest of all patches, whichever round they were in here)
    // One atomic per bucket and kind present among the wave's four patches, all of them in flight at once (they used to go one
    // after the other, a round trip each -- up to eight before a workgroup could say it had arrived): the first of the group
    // leaders with a given counter adds for all of them, the others take their share of what comes back.
    // (the counter: the bucket's, of the workgroup's number)
    const uint32_t counter = bucket * RM_ORD_SUBS + (id & (RM_ORD_SUBS - 1u));
    const uint32_t key = (placed | first_round) ? ((first_round ? RM_ORD_COUNTERS : 0u) | counter) : 0xFFFFu;
    uint32_t before = 0u, total = 0u, first_of = lane >> 4;
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++) {
        const bool same = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)(16u * i)) == key;
        total += same ? 1u : 0u;
        before += (same & (i < (lane >> 4))) ? 1u : 0u;
        first_of = (same & (i < first_of)) ? i : first_of;
    }
    uint32_t base = 0u;
    if (key != 0xFFFFu && before == 0u)
        base = __hip_atomic_fetch_add(a.ord_cnt + ((key & RM_ORD_COUNTERS) ? RM_ORD_FIRST : 0u) + (key & (RM_ORD_COUNTERS - 1u)) * RM_ORD_LINE, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t slot = (uint32_t)__shfl((int)base, (int)(16u * first_of), 64) + before;
    if (leader) {
        rec[lane >> 4].patch = valid ? patch : ~0u;
        rec[lane >> 4].bucket_slot = (counter << 24) | slot;
        rec[lane >> 4].index = index;
        if (grec) {
            // (for the workgroup at the grid's end that writes the places -- on another XCD, behind another L2, as likely as not:
            // what one workgroup of a launch leaves for another goes by agent-scope atomics; plain stores stay in their XCD's L2
            // until the launch is over -- found by the order's own check: every such workgroup read the records of the launch before)
            __hip_atomic_store(grec + (lane >> 4) * 3u + 0u, valid ? patch : ~0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(grec + (lane >> 4) * 3u + 1u, (counter << 24) | slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(grec + (lane >> 4) * 3u + 2u, index, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // (the counter the next launch's waves time this patch into)
        if (valid && a.cost_zero) a.cost_zero[patch] = 0u;
    }
}

// Second half, once its patches have their slots: the workgroup says it has arrived, waits for the others -- they are the
// launch's first workgroups, at most 1,024, all resident whatever the kernel's occupancy: nobody is waited for who is not
// running -- reads the sixteen totals and writes its patches' places into the order.  The wait is bounded in polls (2^16 of
// ~1 us); a workgroup that gives it up writes nothing: the waves behind the first round give up in turn, the frame is void
// and the host is told.  The places also make the NEXT launch's first round (the first n_static / 16 of them) and tell every
// patch its word for it; the first workgroup leaves the host its hint and clears what the next launch counts into.
// `arrived`: the workgroup has said so itself (a classifying workgroup; false: a workgroup at the grid's end, which only waits).
// `rec` NULL: the records are read from memory (ord_rec), where the classifying workgroup `id` left them.
__device__ __forceinline__ void order_places(const KernelArgs &a, uint32_t id, const OrdRec *rec, bool arrive, bool wait) {
    const uint32_t lane = threadIdx.x & 63u, n_patches = a.n_tiles >> 4, ns16 = a.n_static >> 4, n_dyn = n_patches - ns16;
    const uint32_t n_groups = (a.cls_blocks + 31u) >> 5;
    // (the slots' atomics have returned -- their results are in the records -- before this one leaves.)  The last of its 32 to
    // arrive tells the launch, the last of those says go: a word in a line of its own that everybody else only reads.
    // The decision word: the last to arrive turns it from 0 into the launch's tag -- unless a render wave that ran out of patience
    // (a card shared with another process, say, whose waves hold the slots these workgroups need) has turned it into "the
    // order of last resort": then nobody writes places, and every wave takes its patch from the index the launch came with.
    uint32_t go = 0u;
    // (test hook 2: the workgroups of a launch that dispatches by its own order never say they have arrived)
    if (arrive && lane == 0u && !(a.test_stall == 2u && a.ord_read == a.ord_flat)) {
        const uint32_t g = id >> 5, of = min(32u, a.cls_blocks - 32u * g);
        if (__hip_atomic_fetch_add(a.ord_cnt + RM_ORD_ARRIVE + g * RM_ORD_LINE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == of)
            if (__hip_atomic_fetch_add(a.ord_cnt + RM_ORD_GROUPS, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == n_groups) {
                uint32_t expected = 0u;
                go = __hip_atomic_compare_exchange_strong(a.ord_cnt + RM_ORD_GO, &expected, a.ord_tag, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? a.ord_tag : expected;
                // (decided: the places will be written, every one -- and with them the next launch's first round and index)
                if (go == a.ord_tag && a.lists_done_next && a.static_next) *a.lists_done_next = a.ord_tag;
            }
    }
    if (!wait) return;                                                // (the places are somebody else's to write, later)
    go = uniform_u32(go);
    for (uint32_t polls = 0u; go == 0u; polls++) {
        go = uniform_u32(__hip_atomic_load(a.ord_cnt + RM_ORD_GO, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (go != 0u) break;
        if (polls >= 65536u) return;                                  // (cannot happen)
        __builtin_amdgcn_s_sleep(16);
    }
    if (go != a.ord_tag) return;                                      // (the order of last resort: nothing to write)
    if (a.test_stall == 1u) return;                                   // (test hook 1: an order that is never laid out)
    // (both sets of totals asked for before either is summed: one round trip, not two)
    static_assert(RM_ORD_COUNTERS == 64u, "a lane a counter");
    const uint32_t cnt = __hip_atomic_load(a.ord_cnt + lane * RM_ORD_LINE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t cnt1 = __hip_atomic_load(a.ord_cnt + RM_ORD_FIRST + lane * RM_ORD_LINE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t incl = cnt;                                              // inclusive prefix over the sixteen buckets
    for (uint32_t off = 1u; off < RM_ORD_COUNTERS; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)incl, (int)off, 64);
        incl += lane >= off ? o : 0u;
    }
    const uint32_t excl = incl - cnt;
    const bool next = a.static_next && a.dyn_index_next && a.dyn_inv_next;
    // The next launch's first round: the dearest ns16 of ALL patches -- bucket by bucket, within a bucket this launch's first
    // round first -- and the others' places in its index: a patch's rank among all, less the first round.  (The sky, the last
    // bucket, gets into a first round only where there is not enough else.)
    uint32_t both = cnt + cnt1;                                       // inclusive prefix over both kinds
    for (uint32_t off = 1u; off < RM_ORD_COUNTERS; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)both, (int)off, 64);
        both += lane >= off ? o : 0u;
    }
    const uint32_t before_first = both - cnt - cnt1, before_ordered = before_first + cnt1;   // lane b: where bucket b's first-round / ordered patches start among all
    const uint32_t n_lit = (uint32_t)__builtin_amdgcn_readlane((int)incl, (int)(RM_ORD_SKY * RM_ORD_SUBS - 1u));
    for (uint32_t it = 0; it < a.cls_iters; it++) {                   // wave-uniform
        OrdRec r;
        if (rec) {
            r = rec[it * 4u + (lane >> 4)];
        } else {
            uint32_t *g = a.ord_rec + ((size_t)(it * a.cls_blocks + id) * 4u + (lane >> 4)) * 3u;
            r.patch = __hip_atomic_load(g + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            r.bucket_slot = __hip_atomic_load(g + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            r.index = __hip_atomic_load(g + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const uint32_t counter = (r.bucket_slot >> 24) & (RM_ORD_COUNTERS - 1u), bucket = counter / RM_ORD_SUBS, slot = r.bucket_slot & 0xFFFFFFu;
        const bool ordered = !(r.index & RM_ORD_STATIC_BIT);
        const uint32_t pos = (uint32_t)__shfl((int)excl, (int)counter, 64) + slot;
        // (both asked of the bucket's lane, the choice made here: the lane asked knows nothing of this lane's patch)
        const uint32_t start_o = (uint32_t)__shfl((int)before_ordered, (int)counter, 64), start_f = (uint32_t)__shfl((int)before_first, (int)counter, 64);
        const uint32_t among_all = (ordered ? start_o : start_f) + slot;
        if ((lane & 15u) == 0u && r.patch != ~0u) {
            if (ordered && pos < a.ord_cap)
                __hip_atomic_store(a.ord_flat + pos, (a.ord_tag << RM_ORD_TAG_SHIFT) | (bucket == RM_ORD_SKY ? RM_ORD_SKY_BIT : 0u) | r.patch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (next) {
                if (among_all < ns16) a.static_next[among_all] = r.patch;
                else a.dyn_inv_next[among_all - ns16] = r.patch;
                a.dyn_index_next[r.patch] = among_all < ns16 ? RM_ORD_STATIC_BIT | among_all : among_all - ns16;
            }
        }
    }
    if (id == 0u && a.ord_hint && lane == 0u) __hip_atomic_store(a.ord_hint, ((unsigned long long)a.launch_seq << 32) | n_lit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace RM_FLAVOR_NS
