// rm_converge_camera.hpp -- what the host side (rm_camera_host.inc) needs to know about the shade kernels of the converging
// frames with a moving camera (rm_converge_camera.hip): their argument block and the functions that hand out a kernel.  No
// device code.
#ifndef RM_CONVERGE_CAMERA_HPP
#define RM_CONVERGE_CAMERA_HPP

#include <stdint.h>

#include "rm_converge_motion.hpp"

namespace rmdev {

struct ConvergeCameraArgs {
    ConvergeMotionArgs M;                    // the moving shapes' own block; the static-scene kernels read M.C alone
    const double *camera_rows;               // [table_rows][12]: (off.xyz, right.xyz, up.xyz, forward.xyz)
};

}  // namespace rmdev

// The shade kernels over the list with the camera of the sample's row (64 lanes a workgroup, arguments: scene blob,
// ConvergeCameraArgs); the select kernel in front of them is rm_converge.hip's, given the block's M.C.  Static scene: moved
// lights, shapes as stored: bvh, pow_mode, stack 4 or 32.  Moving scene: moved lights and shapes, the flat walk whatever `bvh`
// says.  NULL: no such instantiation.
const void *rm_converge_camera_kernel(bool bvh, int pow_mode, int stack);
const void *rm_converge_camera_moving_kernel(bool bvh, int pow_mode, int stack);

#endif
