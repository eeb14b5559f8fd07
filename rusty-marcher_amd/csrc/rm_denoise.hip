// rm_denoise.hip -- the variance-guided edge-avoiding filter of the converging frames (include/rusty_marcher_amd.h,
// "variance-guided filter"): the spatial filter of SVGF, an a-trous wavelet filter of up to five iterations steered by the
// per-pixel variance the converging frames keep and, where the caller has them, by the hits under the pixels.
//
// Launches of a call, all on the caller's stream, nothing in between goes through the host:
//
//   prepare     one lane per pixel of [0, rows).  Forms C0 = S / n and V0 = m2 / (n (n - 1)) by the header's rule and stores
//               them as (r, g, b, V), 32 B a pixel, into the first plane of the workspace.  Where hits are given it repacks the
//               72-byte rm_hit into the guide's 64 B -- normal, id, point, t, the id being the shape with the hit flag folded in
//               -- so that a tap never touches the record again.  With iterations == 0 it writes the outputs itself.
//   iteration   one per step 1 << i.  A workgroup owns a tile of 32 x 8 pixels, one lane a pixel; the lane forms the 3x3
//               prefilter of V about its pixel, then folds its 25 taps in the header's order and stores (r, g, b, V) into the
//               other plane -- the last iteration into out, variance and the display bytes.
//
// Two paths fetch an iteration's taps and share every line of arithmetic (center_of, fold_tap, finish), so they write the same
// bytes:
//   path 0      every tap is gathered from global memory: 4 B of the count, 32 B of the plane, 64 B of the guide.
//   path 1      the workgroup first stages its tile with a halo of 2 step in LDS, as arrays of one word an entry (steps 1
//               and 2: 432 and 640 entries of 88 B, 38 and 55 KiB, so two workgroups a compute unit stay resident at step 2).
// Which path a step takes is the host's choice (rm_denoise_host.inc), made by measurement (profiles/denoise_figures.txt):
// path 1 for steps 1 and 2, where it takes about 0.6 of the gather's time; the gather beyond.
//
// Nothing read from a count, a hit or a pixel's value forms an address: a tap's address is the lane's own pixel plus a
// constant, held to the frame by comparisons of coordinates alone.  So NaN, infinity or counts from elsewhere give unspecified
// pixels, never a fault.  Rows from `rows` on are neither read nor written: the grid ends there and a tap beyond is skipped.
//
// Arithmetic: + - * / and comparisons of doubles, each rounded once; the unit is compiled with contraction off like every
// other, so there is no fused multiply-add and the bytes are those of tests/denoise_reference.py.
#include <hip/hip_runtime.h>

#include "rm_denoise.hpp"

using namespace rmdev;

namespace rmdenoise {

#define RM_ID_MISS (1ull << 32)              // the guide's id: the shape, or this for a miss
#define RM_ID_EMPTY (1ull << 33)             // path 1 folds count == 0 into the id it keeps in LDS

__device__ __forceinline__ uint8_t display_byte(double v) { return (uint8_t)(255. * __builtin_fmin(__builtin_fmax(v, 0.), 1.)); }

// What a launch leaves for its pixel: the plane, or -- the last one -- the outputs
__device__ __forceinline__ void store_pixel(const DenoiseArgs &a, uint32_t pix, double r, double g, double b, double v) {
    if (!a.last) {
        double2 *d = reinterpret_cast<double2 *>(a.dst + (size_t)pix * RM_DENOISE_PLANE_WORDS);
        d[0] = make_double2(r, g);
        d[1] = make_double2(b, v);
        return;
    }
    a.out[(size_t)pix * 3u] = r;
    a.out[(size_t)pix * 3u + 1u] = g;
    a.out[(size_t)pix * 3u + 2u] = b;
    if (a.variance) a.variance[pix] = v;
    if (a.rgb8) {
        a.rgb8[(size_t)pix * 3u] = display_byte(r);
        a.rgb8[(size_t)pix * 3u + 1u] = display_byte(g);
        a.rgb8[(size_t)pix * 3u + 2u] = display_byte(b);
    }
}

__global__ __launch_bounds__(RM_DENOISE_PREPARE_LANES) void rm_denoise_prepare(DenoiseArgs a) {
    const uint32_t total = a.rows * a.frame_width;                       // (below 2^31: the host checked)
    const uint32_t pix = blockIdx.x * (uint32_t)RM_DENOISE_PREPARE_LANES + threadIdx.x;
    if (pix >= total) return;
    const uint32_t n = a.count[pix];
    const double nd = (double)n;
    double r = 0., g = 0., b = 0.;
    if (n > 0u) {
        r = a.sum[(size_t)pix * 3u] / nd;
        g = a.sum[(size_t)pix * 3u + 1u] / nd;
        b = a.sum[(size_t)pix * 3u + 2u] / nd;
    }
    double v = a.fallback_variance;
    if (n >= 2u) {
        const double Y = a.stats[(size_t)pix * 2u], Q = a.stats[(size_t)pix * 2u + 1u];
        double m2 = Q - (Y * Y) / nd;
        if (m2 < 0.) m2 = 0.;
        v = m2 / (nd * (nd - 1.));
    }
    store_pixel(a, pix, r, g, b, v);
    if (a.hits && !a.last) {
        const double *h = a.hits + (size_t)pix * 9u;                     // rm_hit: t, point, normal, (shape, element), (hit, pad)
        const unsigned long long se = (unsigned long long)__double_as_longlong(h[7]), hp = (unsigned long long)__double_as_longlong(h[8]);
        const unsigned long long id = (uint32_t)hp != 0u ? (se & 0xffffffffull) : RM_ID_MISS;
        double2 *q = reinterpret_cast<double2 *>(a.guide + (size_t)pix * RM_DENOISE_GUIDE_WORDS);
        q[0] = make_double2(h[4], h[5]);
        q[1] = make_double2(h[6], __longlong_as_double((long long)id));
        q[2] = make_double2(h[1], h[2]);
        q[3] = make_double2(h[3], h[0]);
    }
}

// A tap as fold_tap takes it
struct Tap {
    double r, g, b, v;
    double nx, ny, nz, px, py, pz;
    unsigned long long id;
};

// What a lane knows of its own pixel before the taps
struct Center {
    double r, g, b, v, y, den;
    double nx, ny, nz, px, py, pz, dz;
    unsigned long long id;
    bool have;                                                           // count[p] != 0
};

struct Sums {
    double sw = 0., sr = 0., sg = 0., sb = 0., sv = 0.;
};

// den and, guided, dz of the centre: `c` holds the pixel's values, g the prefiltered variance, t the hit's parameter
template <bool GUIDED>
__device__ __forceinline__ void center_of(const DenoiseArgs &a, Center &c, double g, double t) {
    c.y = (c.r + c.g) + c.b;
    c.den = (a.sigma_l * a.sigma_l) * g + a.epsilon;
    if constexpr (GUIDED) {
        const double sz = a.sigma_z * (1. + t);
        c.dz = sz * sz;
    }
}

// One tap that is in bounds and has samples; hh = h(dx) h(dy)
template <bool GUIDED>
__device__ __forceinline__ void fold_tap(const DenoiseArgs &a, const Center &c, const Tap &q, double hh, Sums &s) {
    const double yq = (q.r + q.g) + q.b;
    const double d = c.y - yq;
    const double wl = c.have ? c.den / (c.den + d * d) : 1.;
    double w = hh * wl;
    if constexpr (GUIDED) {
        const bool miss_p = (c.id & RM_ID_MISS) != 0ull, miss_q = (q.id & RM_ID_MISS) != 0ull;
        if (miss_p != miss_q) return;                                    // exactly one missed
        if (!miss_p) {
            if ((uint32_t)c.id != (uint32_t)q.id) return;                // another shape
            const double dot = (c.nx * q.nx + c.ny * q.ny) + c.nz * q.nz;
            if (!(dot > 0.)) return;
            double wn = dot;
            for (uint32_t k = 0; k < a.squarings; k++) wn = wn * wn;
            const double e = (c.nx * (q.px - c.px) + c.ny * (q.py - c.py)) + c.nz * (q.pz - c.pz);
            const double wz = c.dz / (c.dz + e * e);
            w = w * wn * wz;
        }
    }
    s.sw += w;
    s.sr += w * q.r;
    s.sg += w * q.g;
    s.sb += w * q.b;
    s.sv += (w * w) * q.v;
}

__device__ __forceinline__ void finish(const DenoiseArgs &a, uint32_t pix, const Center &c, const Sums &s) {
    if (s.sw > 0.) store_pixel(a, pix, s.sr / s.sw, s.sg / s.sw, s.sb / s.sw, s.sv / (s.sw * s.sw));
    else store_pixel(a, pix, c.r, c.g, c.b, c.v);
}

__device__ __forceinline__ double h5(int d) { return d == 0 ? 3. / 8. : (d == 1 || d == -1) ? 1. / 4. : 1. / 16.; }
__device__ __forceinline__ double k3(int d) { return d == 0 ? 1. / 2. : 1. / 4.; }

// The plane's and the guide's words of pixel `pix` from global memory
template <bool GUIDED>
__device__ __forceinline__ void global_tap(const DenoiseArgs &a, uint32_t pix, Tap &q) {
    const double2 *s = reinterpret_cast<const double2 *>(a.src + (size_t)pix * RM_DENOISE_PLANE_WORDS);
    const double2 s0 = s[0], s1 = s[1];
    q.r = s0.x; q.g = s0.y; q.b = s1.x; q.v = s1.y;
    if constexpr (GUIDED) {
        const double2 *u = reinterpret_cast<const double2 *>(a.guide + (size_t)pix * RM_DENOISE_GUIDE_WORDS);
        const double2 u0 = u[0], u1 = u[1], u2 = u[2], u3 = u[3];
        q.nx = u0.x; q.ny = u0.y; q.nz = u1.x;
        q.id = (unsigned long long)__double_as_longlong(u1.y);
        q.px = u2.x; q.py = u2.y; q.pz = u3.x;
    }
}

// path 0: every tap from global memory
template <bool GUIDED>
__global__ __launch_bounds__(RM_DENOISE_TILE_W * RM_DENOISE_TILE_H) void rm_denoise_gather_t(DenoiseArgs a) {
    const int W = (int)a.frame_width, R = (int)a.rows, S = (int)a.step;
    const int x = (int)(blockIdx.x * RM_DENOISE_TILE_W + threadIdx.x % RM_DENOISE_TILE_W);
    const int y = (int)(blockIdx.y * RM_DENOISE_TILE_H + threadIdx.x / RM_DENOISE_TILE_W);
    if (x >= W || y >= R) return;                                        // (never: the tiles cover the frame exactly)
    const uint32_t pix = (uint32_t)y * a.frame_width + (uint32_t)x;
    double gv = 0., gk = 0.;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= R) continue;
            const double k = k3(dx) * k3(dy);
            gv += k * a.src[(size_t)((uint32_t)qy * a.frame_width + (uint32_t)qx) * RM_DENOISE_PLANE_WORDS + 3u];
            gk += k;
        }
    Center c;
    Tap self;
    global_tap<GUIDED>(a, pix, self);
    c.r = self.r; c.g = self.g; c.b = self.b; c.v = self.v;
    c.have = a.count[pix] != 0u;
    double t = 0.;
    if constexpr (GUIDED) {
        c.nx = self.nx; c.ny = self.ny; c.nz = self.nz; c.px = self.px; c.py = self.py; c.pz = self.pz; c.id = self.id;
        t = a.guide[(size_t)pix * RM_DENOISE_GUIDE_WORDS + 7u];
    }
    center_of<GUIDED>(a, c, gv / gk, t);
    Sums s;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++)
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + S * dx, qy = y + S * dy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= R) continue;
            const uint32_t q = (uint32_t)qy * a.frame_width + (uint32_t)qx;
            if (a.count[q] == 0u) continue;
            Tap tap;
            global_tap<GUIDED>(a, q, tap);
            fold_tap<GUIDED>(a, c, tap, h5(dx) * h5(dy), s);
        }
    finish(a, pix, c, s);
}

// path 1: the tile and its halo staged in LDS, one array a word; STEP is 1 or 2
template <bool GUIDED, int STEP>
__global__ __launch_bounds__(RM_DENOISE_TILE_W * RM_DENOISE_TILE_H) void rm_denoise_tiled_t(DenoiseArgs a) {
    constexpr int HALO = 2 * STEP, TW = RM_DENOISE_TILE_W + 2 * HALO, TH = RM_DENOISE_TILE_H + 2 * HALO, ENTRIES = TW * TH;
    constexpr int WORDS = GUIDED ? 10 : 4;                               // r g b V, then normal and point
    __shared__ double words[WORDS][ENTRIES];
    __shared__ unsigned long long ids[ENTRIES];
    const int W = (int)a.frame_width, R = (int)a.rows;
    const int x0 = (int)(blockIdx.x * RM_DENOISE_TILE_W) - HALO, y0 = (int)(blockIdx.y * RM_DENOISE_TILE_H) - HALO;
    for (int e = (int)threadIdx.x; e < ENTRIES; e += RM_DENOISE_TILE_W * RM_DENOISE_TILE_H) {
        const int qx = x0 + e % TW, qy = y0 + e / TW;
        if (qx < 0 || qx >= W || qy < 0 || qy >= R) continue;            // (never read: the taps test the same coordinates)
        const uint32_t q = (uint32_t)qy * a.frame_width + (uint32_t)qx;
        Tap tap;
        tap.id = 0ull;
        global_tap<GUIDED>(a, q, tap);
        words[0][e] = tap.r; words[1][e] = tap.g; words[2][e] = tap.b; words[3][e] = tap.v;
        if constexpr (GUIDED) {
            words[4][e] = tap.nx; words[5][e] = tap.ny; words[6][e] = tap.nz;
            words[7][e] = tap.px; words[8][e] = tap.py; words[9][e] = tap.pz;
        }
        ids[e] = tap.id | (a.count[q] == 0u ? RM_ID_EMPTY : 0ull);
    }
    __syncthreads();
    const int lx = (int)(threadIdx.x % RM_DENOISE_TILE_W) + HALO, ly = (int)(threadIdx.x / RM_DENOISE_TILE_W) + HALO;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= W || y >= R) return;                                        // (never: the tiles cover the frame exactly)
    const uint32_t pix = (uint32_t)y * a.frame_width + (uint32_t)x;
    const auto local_tap = [&](int e, Tap &q) {
        q.r = words[0][e]; q.g = words[1][e]; q.b = words[2][e]; q.v = words[3][e];
        if constexpr (GUIDED) {
            q.nx = words[4][e]; q.ny = words[5][e]; q.nz = words[6][e];
            q.px = words[7][e]; q.py = words[8][e]; q.pz = words[9][e];
        }
        q.id = ids[e];
    };
    double gv = 0., gk = 0.;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= R) continue;
            const double k = k3(dx) * k3(dy);
            gv += k * words[3][(ly + dy) * TW + lx + dx];
            gk += k;
        }
    Center c;
    Tap self;
    local_tap(ly * TW + lx, self);
    c.r = self.r; c.g = self.g; c.b = self.b; c.v = self.v;
    c.have = (self.id & RM_ID_EMPTY) == 0ull;
    double t = 0.;
    if constexpr (GUIDED) {
        c.nx = self.nx; c.ny = self.ny; c.nz = self.nz; c.px = self.px; c.py = self.py; c.pz = self.pz; c.id = self.id;
        t = a.guide[(size_t)pix * RM_DENOISE_GUIDE_WORDS + 7u];
    }
    center_of<GUIDED>(a, c, gv / gk, t);
    Sums s;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++)
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + STEP * dx, qy = y + STEP * dy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= R) continue;
            Tap tap;
            local_tap((ly + STEP * dy) * TW + lx + STEP * dx, tap);
            if ((tap.id & RM_ID_EMPTY) != 0ull) continue;
            fold_tap<GUIDED>(a, c, tap, h5(dx) * h5(dy), s);
        }
    finish(a, pix, c, s);
}

}  // namespace rmdenoise

using namespace rmdenoise;

const void *rm_denoise_prepare_kernel() { return (const void *)rm_denoise_prepare; }

const void *rm_denoise_iteration_kernel(bool guided, int path, uint32_t step) {
    if (path == 0) return guided ? (const void *)rm_denoise_gather_t<true> : (const void *)rm_denoise_gather_t<false>;
    if (path != 1) return nullptr;
    if (step == 1u) return guided ? (const void *)rm_denoise_tiled_t<true, 1> : (const void *)rm_denoise_tiled_t<false, 1>;
    if (step == 2u) return guided ? (const void *)rm_denoise_tiled_t<true, 2> : (const void *)rm_denoise_tiled_t<false, 2>;
    return nullptr;
}
