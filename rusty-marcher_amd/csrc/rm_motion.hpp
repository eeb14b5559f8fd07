// rm_motion.hpp -- what the host side (rm_motion_host.inc) needs to know about the kernel of the moving spheres (rm_motion.hip):
// its argument block and the function that hands out a kernel.  No device code.
#ifndef RM_MOTION_HPP
#define RM_MOTION_HPP

#include <stdint.h>

#include "rm_soft.hpp"

namespace rmdev {

struct MotionArgs {
    SoftArgs S;                              // the area lights' own block: rays, fold, sum, mean, bytes and light offsets are its
    const double *shape_offsets;             // [S.A.L.n_samples][n_shapes][3]; not read where the scene has no spheres
    const uint32_t *pid_map;                 // the resident image's, 2 words a pid: word 0 is the shape of a device primitive
    uint32_t n_shapes, _pad;                 // the scene's shape count: the length of a row
};

}  // namespace rmdev

// The sample-shade-and-accumulate kernel with moved lights and spheres (64 lanes a workgroup, arguments: scene blob,
// MotionArgs).  The family walks flat whatever `bvh` says -- a hierarchy's boxes hold for the uploaded centres only -- so it
// has four instantiations: pow_mode x stack 4 or 32.  NULL: no such instantiation.
const void *rm_motion_kernel(bool bvh, int pow_mode, int stack);

#endif
