// rm_lens.hpp -- what the host side (rm_lens_host.inc) needs to know about the kernel of the thin-lens camera (rm_lens.hip):
// its argument block and the function that hands out a kernel.  No device code.
#ifndef RM_LENS_HPP
#define RM_LENS_HPP

#include <stdint.h>

#include "rm_internal.h"

namespace rmdev {

struct LensArgs {
    rm_dev_header H;                         // the resident scene's, with off_occ = 0 (as the radiance kernels')
    uint32_t frame_width, rows;              // the pixels a lens frame writes: [0, frame_width) x [0, rows)
    uint32_t n_samples, max_depth;           // rays a pixel, 1..64
    uint32_t oriented, _pad;
    double aperture, focus;                  // lens radius; distance of the plane in focus along forward
    double bg_x, bg_y, bg_z;
    double width, height, half_fov, ratio;   // the params' Renderer
    double cam_x, cam_y, cam_z;              // the context's camera
    // ... and its basis: the fixed view's where the context is not oriented (the lens point takes right and up either way;
    // sample_direction reads the three where oriented)
    double cam_rx, cam_ry, cam_rz, cam_ux, cam_uy, cam_uz, cam_fx, cam_fy, cam_fz;
    const double *table;                     // n_samples rows (dx, dy, u, v)
    double *frame;                           // [frame_height][frame_width][3]
};

}  // namespace rmdev

// The sample-shade-and-resolve kernel (64 lanes a workgroup, arguments: scene blob, LensArgs), instantiated as the radiance
// kernel is (rm_radiance.hpp): bvh, pow_mode, stack 4 or 32.  NULL: no such instantiation.
const void *rm_lens_kernel(bool bvh, int pow_mode, int stack);

#endif
