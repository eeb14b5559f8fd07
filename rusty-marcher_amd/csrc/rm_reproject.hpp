// rm_reproject.hpp -- what the host side (rm_reproject_host.inc) needs to know about the kernel of the temporal reprojection
// (rm_reproject.hip): its argument block and the function that hands it out.  No device code.
#ifndef RM_REPROJECT_HPP
#define RM_REPROJECT_HPP

#include <stddef.h>
#include <stdint.h>

// A workgroup: a tile of RM_REPROJECT_TILE_W x RM_REPROJECT_TILE_H pixels, one lane a pixel, the filter's tiles.  The frame's
// width and its rows are multiples of 32, so the tiles cover [0, rows) x [0, frame_width) exactly and no lane is without a pixel.
#define RM_REPROJECT_TILE_W 32
#define RM_REPROJECT_TILE_H 8

namespace rmdev {

struct ReprojectArgs {
    uint32_t frame_width, rows;              // the pixels of [0, rows) x [0, frame_width), fewer than 2^31
    uint32_t max_history;                    // rm_reproject.max_history
    uint32_t _pad;
    double width, height, ratio, half_fov;   // rm_params': the sample position's four
    double sigma_z, min_normal_dot;
    double ex, ey, ez;                       // the previous view: position, right, up, forward
    double rx, ry, rz, ux, uy, uz, fx, fy, fz;
    const double *prev_sum;                  // [frame_height][frame_width][3]
    const double *prev_stats;                // [frame_height][frame_width][2]
    const uint32_t *prev_count;              // [frame_height][frame_width]
    const double *prev_hits;                 // [frame_height][frame_width] rm_hit, 9 words each: the previous view's
    const double *cur_hits;                  // ... and the view's the new frame is sampled from
    double *out_sum, *out_stats;
    uint32_t *out_count;
    uint8_t *carried;                        // [frame_height][frame_width] bytes, or NULL
    uint32_t *carried_total;                 // one word the host zeroed on the stream, or NULL
    double *mean;                            // [frame_height][frame_width][3], or NULL: out_sum / n' (0 without history) -- the tick's
    uint8_t *rgb8;                           // ... and its display bytes, or NULL
};

}  // namespace rmdev

// The kernel (a workgroup a tile, grid frame_width / TILE_W x rows / TILE_H; argument: ReprojectArgs)
const void *rm_reproject_kernel();

#endif
