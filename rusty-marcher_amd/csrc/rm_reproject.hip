// rm_reproject.hip -- temporal reprojection of the converging frames (include/rusty_marcher_amd.h, "temporal reprojection"):
// the other half of SVGF.  The sums a converging frame held for one view are carried to another view of the same scene: every
// pixel of the new view finds the point under it in the previous view's picture, takes the four samples around that position
// that lie on the same surface, and begins its own frame with their mean and the smallest of their counts.
//
// One launch, on the caller's stream: a workgroup owns a tile of 32 x 8 pixels, one lane a pixel.  The lane reads its own hit
// (72 B), projects the point into the previous view by the header's rule, and gathers its four taps straight from the previous
// frame's buffers: 4 B of the count, 64 B of the hit record, 24 B of the sum, 16 B of the stats a tap.
//
// Why the taps are gathered and nothing is repacked first.  A tap's address follows the motion, but motion is smooth: the 64
// lanes of a wave are two rows of 32 neighbouring pixels, their sample positions are neighbours in the previous view wherever
// the view shows one surface, and the four taps of a lane are the taps of its neighbours one pixel on.  So a wave's 256 taps
// land on about 2 x 33 x 2 distinct pixels, each fetched from HBM once and served from cache thereafter, and the launch moves
// about what a plain copy of the two frames moves: 108 B a pixel in, 72 B of the new hit, 44 B out.  A pack launch in front
// (one 128-byte record a pixel) would add a write and a read of 128 B a pixel to that, more than the gather itself reads, and
// needs a workspace rm_reproject_device's contract has no room for (the call keeps no state).  It was not built;
// profiles/reproject_figures.txt has the gather against its HBM floor.  Nothing is staged in LDS either: a tile's footprint in
// the previous view is known only once every lane has projected, its size is unbounded under a step towards the scene, and the
// cache already serves the overlap.
//
// Data forms addresses here -- that is a gather along motion -- but none is formed before the range check in doubles: the
// sample position is held to (-1, W) x (-1, rows) by comparisons a NaN fails, only then converted, and every tap is held to
// [0, W) x [0, rows) once more as integers.  So NaN, infinity or a hit buffer from elsewhere give pixels without history or
// unspecified values, never a fault.  Counts and shape ids are only compared and converted.  Rows from `rows` on are neither
// read nor written: the grid ends there and a tap beyond is skipped.
//
// Arithmetic: + - * /, floor and comparisons of doubles, each rounded once; the unit is compiled with contraction off like
// every other, so there is no fused multiply-add and the bytes are those of tests/reproject_reference.py.
#include <hip/hip_runtime.h>

#include "rm_reproject.hpp"

using namespace rmdev;

namespace rmreproject {

__device__ __forceinline__ uint8_t display_byte(double v) { return (uint8_t)(255. * __builtin_fmin(__builtin_fmax(v, 0.), 1.)); }

// What the lane found for its pixel
struct Carry {
    double sw = 0., sr = 0., sg = 0., sb = 0., s1 = 0., s2 = 0.;
    uint32_t nmin = 0xffffffffu;
};

// The four taps about (sx, sy), which passed the range check; P, N, dz: the current hit's point, normal and gate
__device__ __forceinline__ void fold_taps(const ReprojectArgs &a, double sx, double sy, uint32_t shape, double px, double py, double pz, double nx,
                                          double ny, double nz, double dz, Carry &c) {
    const int W = (int)a.frame_width, R = (int)a.rows;
    const double fx0 = __builtin_floor(sx), fy0 = __builtin_floor(sy);
    const double fx = sx - fx0, fy = sy - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;                              // in [-1, W) and [-1, rows): the caller's check
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const double wb = (i ? fx : 1. - fx) * (j ? fy : 1. - fy);
            if (!(wb > 0.)) continue;
            const int qx = x0 + i, qy = y0 + j;
            if (qx < 0 || qx >= W || qy < 0 || qy >= R) continue;
            const uint32_t q = (uint32_t)qy * a.frame_width + (uint32_t)qx;
            const uint32_t n = a.prev_count[q];
            if (n == 0u) continue;
            const double *h = a.prev_hits + (size_t)q * 9u;              // rm_hit: t, point, normal, (shape, element), (hit, pad)
            const unsigned long long se = (unsigned long long)__double_as_longlong(h[7]), hp = (unsigned long long)__double_as_longlong(h[8]);
            if ((uint32_t)hp == 0u) continue;
            if ((uint32_t)se != shape) continue;
            const double qnx = h[4], qny = h[5], qnz = h[6];
            const double d = (nx * qnx + ny * qny) + nz * qnz;
            if (!(d > a.min_normal_dot)) continue;
            const double e = (nx * (h[1] - px) + ny * (h[2] - py)) + nz * (h[3] - pz);
            if (!(e * e <= dz)) continue;
            const double nq = (double)n;
            const double *s = a.prev_sum + (size_t)q * 3u;
            const double *st = a.prev_stats + (size_t)q * 2u;
            c.sw += wb;
            c.sr += wb * (s[0] / nq);
            c.sg += wb * (s[1] / nq);
            c.sb += wb * (s[2] / nq);
            c.s1 += wb * (st[0] / nq);
            c.s2 += wb * (st[1] / nq);
            c.nmin = min(c.nmin, n);
        }
}

__global__ __launch_bounds__(RM_REPROJECT_TILE_W * RM_REPROJECT_TILE_H) void rm_reproject_gather(ReprojectArgs a) {
    const uint32_t x = blockIdx.x * RM_REPROJECT_TILE_W + threadIdx.x % RM_REPROJECT_TILE_W;
    const uint32_t y = blockIdx.y * RM_REPROJECT_TILE_H + threadIdx.x / RM_REPROJECT_TILE_W;
    const bool in = x < a.frame_width && y < a.rows;                     // (always: the tiles cover the frame exactly; no early return: the wave votes below)
    bool carried = false;
    if (in) {
        const uint32_t pix = y * a.frame_width + x;
        Carry c;
        const double *h = a.cur_hits + (size_t)pix * 9u;
        const unsigned long long se = (unsigned long long)__double_as_longlong(h[7]), hp = (unsigned long long)__double_as_longlong(h[8]);
        if ((uint32_t)hp != 0u) {
            const double t = h[0], px = h[1], py = h[2], pz = h[3], nx = h[4], ny = h[5], nz = h[6];
            const double vx = px - a.ex, vy = py - a.ey, vz = pz - a.ez;
            const double zf = (vx * a.fx + vy * a.fy) + vz * a.fz;
            const double xr = (vx * a.rx + vy * a.ry) + vz * a.rz;
            const double yu = (vx * a.ux + vy * a.uy) + vz * a.uz;
            if (zf > 0.) {
                const double sx = (((xr / zf) / a.ratio) / a.half_fov / 2. + 0.5) * a.width;
                const double sy = (((yu / zf) / a.half_fov) / -2. + 0.5) * a.height;
                // the range check, in doubles, before any conversion to an integer; a NaN fails every comparison
                if (sx > -1. && sx < (double)a.frame_width && sy > -1. && sy < (double)a.rows) {
                    const double sz = a.sigma_z * (1. + t);
                    fold_taps(a, sx, sy, (uint32_t)se, px, py, pz, nx, ny, nz, sz * sz, c);
                }
            }
        }
        double r = 0., g = 0., b = 0., s1 = 0., s2 = 0.;
        uint32_t n = 0u;
        double mr = 0., mg = 0., mb = 0.;
        if (c.sw > 0.) {
            n = min(c.nmin, a.max_history);
            const double nd = (double)n;
            r = (c.sr / c.sw) * nd; g = (c.sg / c.sw) * nd; b = (c.sb / c.sw) * nd;
            s1 = (c.s1 / c.sw) * nd; s2 = (c.s2 / c.sw) * nd;
            mr = r / nd; mg = g / nd; mb = b / nd;
            carried = true;
        }
        a.out_sum[(size_t)pix * 3u] = r;
        a.out_sum[(size_t)pix * 3u + 1u] = g;
        a.out_sum[(size_t)pix * 3u + 2u] = b;
        a.out_stats[(size_t)pix * 2u] = s1;
        a.out_stats[(size_t)pix * 2u + 1u] = s2;
        a.out_count[pix] = n;
        if (a.carried) a.carried[pix] = carried ? 1 : 0;
        if (a.mean) {
            a.mean[(size_t)pix * 3u] = mr;
            a.mean[(size_t)pix * 3u + 1u] = mg;
            a.mean[(size_t)pix * 3u + 2u] = mb;
        }
        if (a.rgb8) {
            a.rgb8[(size_t)pix * 3u] = display_byte(mr);
            a.rgb8[(size_t)pix * 3u + 1u] = display_byte(mg);
            a.rgb8[(size_t)pix * 3u + 2u] = display_byte(mb);
        }
    }
    if (!a.carried_total) return;                                        // launch-uniform
    const unsigned long long m = __ballot(carried);
    if (m != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(a.carried_total, (uint32_t)__popcll(m));   // one atomic add a wave
}

}  // namespace rmreproject

using namespace rmreproject;

const void *rm_reproject_kernel() { return (const void *)rm_reproject_gather; }
