// rm_radiance.hpp -- what the host side (rm_radiance_host.inc) needs to know about the radiance kernels
// (rm_radiance.hip): their argument block and the function that hands out a kernel.  No device code.
#ifndef RM_RADIANCE_HPP
#define RM_RADIANCE_HPP

#include <stdint.h>

#include "rm_internal.h"

namespace rmdev {

// How a lane comes by its ray: a wave-uniform switch in front of the ray steps, not a kernel of its own.
enum { RM_RADIANCE_RAYS = 0, RM_RADIANCE_SAMPLES = 1, RM_RADIANCE_SAMPLES_ORIENTED = 2 };

struct RadianceArgs {
    rm_dev_header H;                         // the resident scene's, with off_occ = 0 (see rm_radiance.hip)
    uint64_t n;                              // one lane per answer
    uint32_t mode, max_depth;
    double bg_x, bg_y, bg_z;
    const rm_vec3 *origins, *directions;     // RM_RADIANCE_RAYS
    const double *xy;                        // RM_RADIANCE_SAMPLES*: n pairs (sx, sy)
    double width, height, half_fov, ratio;   // ... the params' Renderer
    double cam_x, cam_y, cam_z;              // ... the context's camera
    double cam_rx, cam_ry, cam_rz, cam_ux, cam_uy, cam_uz, cam_fx, cam_fy, cam_fz;   // RM_RADIANCE_SAMPLES_ORIENTED
    rm_vec3 *rgb;
};

}  // namespace rmdev

// The kernel of a radiance launch (64 lanes a workgroup, arguments: scene blob, RadianceArgs).
// bvh: the scene carries a hierarchy; pow_mode: POW_GENERIC / POW_INTEGER (rm_kernel_args.hpp);
// stack: 4 or 32 parked rays a lane (4 serves max_depth <= 5).  NULL: no such instantiation.
const void *rm_radiance_kernel(bool bvh, int pow_mode, int stack);

#endif
