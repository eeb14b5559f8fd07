// rm_camera.hpp -- what the host side (rm_camera_host.inc) needs to know about the kernels of the moving camera (rm_camera.hip):
// their argument block and the functions that hand out a kernel.  No device code.
#ifndef RM_CAMERA_HPP
#define RM_CAMERA_HPP

#include <stdint.h>

#include "rm_motion.hpp"

namespace rmdev {

struct CameraArgs {
    MotionArgs M;                            // the moving shapes' own block; the static-scene kernels read M.S alone
    const double *camera_rows;               // [M.S.A.L.n_samples][12]: (off.xyz, right.xyz, up.xyz, forward.xyz)
};

}  // namespace rmdev

// The sample-shade-and-accumulate kernels with the camera of the lane's row (64 lanes a workgroup, arguments: scene blob,
// CameraArgs).  Static scene: moved lights, shapes as stored, instantiated as the area lights' kernel is (rm_soft.hpp): bvh,
// pow_mode, stack 4 or 32.  Moving scene: moved lights and shapes, the flat walk whatever `bvh` says, as the moving shapes'
// (rm_motion_shapes.hpp).  NULL: no such instantiation.
const void *rm_camera_kernel(bool bvh, int pow_mode, int stack);
const void *rm_camera_moving_kernel(bool bvh, int pow_mode, int stack);

#endif
