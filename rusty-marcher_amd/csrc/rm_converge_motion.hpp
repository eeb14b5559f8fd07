// rm_converge_motion.hpp -- what the host side (rm_converge_motion_host.inc) needs to know about the shade kernel of the
// converging frames with moving spheres (rm_converge_motion.hip): its argument block and the function that hands out a kernel.
// No device code.
#ifndef RM_CONVERGE_MOTION_HPP
#define RM_CONVERGE_MOTION_HPP

#include <stdint.h>

#include "rm_converge.hpp"

namespace rmdev {

struct ConvergeMotionArgs {
    ConvergeArgs C;                          // the converging frames' own block: select, rays, fold, buffers and light offsets are its
    const double *shape_offsets;             // [table_rows][n_shapes][3]; not read where the scene has no spheres (rm_converge_moving.hip: no shapes)
    const uint32_t *pid_map;                 // the resident image's, 2 words a pid: word 0 is the shape of a device primitive
    uint32_t n_shapes, _pad;                 // the scene's shape count: the length of a row
};

}  // namespace rmdev

// The shade kernel over the list with moved lights and spheres (64 lanes a workgroup, arguments: scene blob,
// ConvergeMotionArgs); the select kernel in front of it is rm_converge.hip's, given the block's C.  The family walks flat whatever
// `bvh` says -- a hierarchy's boxes hold for the uploaded centres only -- so it has four instantiations: pow_mode x stack 4 or
// 32.  NULL: no such instantiation.
const void *rm_converge_motion_kernel(bool bvh, int pow_mode, int stack);

#endif
