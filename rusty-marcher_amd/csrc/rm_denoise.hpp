// rm_denoise.hpp -- what the host side (rm_denoise_host.inc) needs to know about the kernels of the variance-guided filter
// (rm_denoise.hip): their argument block, the workspace's layout and the functions that hand out a kernel.  No device code.
#ifndef RM_DENOISE_HPP
#define RM_DENOISE_HPP

#include <stddef.h>
#include <stdint.h>

#define RM_DENOISE_PREPARE_LANES 256
// An iteration's workgroup: a tile of RM_DENOISE_TILE_W x RM_DENOISE_TILE_H pixels, one lane a pixel.  The frame's width and
// its rows are multiples of 32, so the tiles cover [0, rows) x [0, frame_width) exactly and no lane is without a pixel.
#define RM_DENOISE_TILE_W 32
#define RM_DENOISE_TILE_H 8
#define RM_DENOISE_MAX_ITERATIONS 5u
#define RM_DENOISE_MAX_SQUARINGS 8u

// The workspace, for P = rows x frame_width pixels: two planes of (r, g, b, V), 4 doubles a pixel, the iterations go back and
// forth between; behind them the guide, 8 words a pixel: normal, the shape id with the hit flag folded in (a uint64_t: the
// shape, or all ones for a miss), point, t.  256 B are added so that the size is never 0.
#define RM_DENOISE_PLANE_WORDS 4u
#define RM_DENOISE_GUIDE_WORDS 8u
static inline size_t rm_denoise_workspace_bytes(size_t pixels) {
    return (pixels * (2u * RM_DENOISE_PLANE_WORDS + RM_DENOISE_GUIDE_WORDS) * sizeof(double) + 255u) / 256u * 256u + 256u;
}

namespace rmdev {

struct DenoiseArgs {
    uint32_t frame_width, rows;              // the pixels of [0, rows) x [0, frame_width), fewer than 2^31
    uint32_t step;                           // the iteration's: 1 << i
    uint32_t squarings;                      // rm_denoise.normal_squarings
    uint32_t last;                           // != 0: this launch writes out, variance and rgb8 (the prepare launch: iterations == 0)
    uint32_t _pad;
    double sigma_l, sigma_z, epsilon, fallback_variance;
    const double *sum;                       // [frame_height][frame_width][3]     (the prepare launch reads these four)
    const double *stats;                     // [frame_height][frame_width][2]
    const uint32_t *count;                   // [frame_height][frame_width]        (... and every iteration this one)
    const double *hits;                      // [frame_height][frame_width] rm_hit, 9 words each, or NULL: no guide
    const double *src;                       // the plane an iteration reads
    double *dst;                             // the plane a launch writes where it is not the last
    double *guide;                           // the guide's words; written by the prepare launch, read by the iterations
    double *out;                             // [frame_height][frame_width][3]
    double *variance;                        // [frame_height][frame_width], or NULL
    uint8_t *rgb8;                           // [frame_height][frame_width][3] bytes, or NULL
};

}  // namespace rmdev

// The prepare kernel (RM_DENOISE_PREPARE_LANES lanes a workgroup, one lane a pixel; argument: DenoiseArgs): C0 and V0 into dst
// -- into the outputs where `last` -- and, where hits is given, the guide's words.
const void *rm_denoise_prepare_kernel();
// An iteration (a workgroup a tile, grid frame_width / TILE_W x rows / TILE_H; argument: DenoiseArgs), with the guide and without.
// path 0: every tap is gathered from global memory; path 1: the workgroup stages its tile and a halo of two taps in LDS first
// (steps 1 and 2 only; NULL for a step it does not serve).
const void *rm_denoise_iteration_kernel(bool guided, int path, uint32_t step);

#endif
