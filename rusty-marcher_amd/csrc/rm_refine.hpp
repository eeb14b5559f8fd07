// rm_refine.hpp -- what the host side (rm_refine_host.inc) needs to know about the kernels of the adaptive anti-aliasing
// (rm_refine.hip): their argument block and the functions that hand out a kernel.  No device code.
#ifndef RM_REFINE_HPP
#define RM_REFINE_HPP

#include <stdint.h>

#include "rm_internal.h"

namespace rmdev {

struct RefineArgs {
    rm_dev_header H;                         // the resident scene's, with off_occ = 0 (as the radiance kernels')
    uint32_t frame_width, rows;              // the pixels a render writes: [0, frame_width) x [0, rows)
    uint32_t n, max_depth;                   // n x n samples a refined pixel
    uint32_t oriented, _pad;
    double threshold;                        // a pixel is refined iff its contrast is > threshold
    double bg_x, bg_y, bg_z;
    double width, height, half_fov, ratio;   // the params' Renderer
    double cam_x, cam_y, cam_z;              // the context's camera
    double cam_rx, cam_ry, cam_rz, cam_ux, cam_uy, cam_uz, cam_fx, cam_fy, cam_fz;   // ... and its basis (read where oriented)
    double *frame;                           // [frame_height][frame_width][3], refined in place
    uint32_t *ws;                            // the workspace: the count, then the listed pixels y * frame_width + x
    uint8_t *mask;                           // optional: [frame_height][frame_width] bytes
};

}  // namespace rmdev

// Lanes a workgroup of the mark kernel (one lane per pixel).
#define RM_REFINE_MARK_LANES 256

// The mark kernel (arguments: RefineArgs): contrast, mask, compaction into the workspace.
const void *rm_refine_mark_kernel();
// The shade-and-resolve kernel (64 lanes a workgroup, arguments: scene blob, RefineArgs), instantiated as the radiance
// kernel is (rm_radiance.hpp): bvh, pow_mode, stack 4 or 32.  NULL: no such instantiation.
const void *rm_refine_shade_kernel(bool bvh, int pow_mode, int stack);

#endif
