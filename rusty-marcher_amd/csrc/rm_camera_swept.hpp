// rm_camera_swept.hpp -- what the host side (rm_camera_swept_host.inc) needs to know about the kernel of the moving camera over a
// swept hierarchy (rm_camera_swept.hip): the function that hands out a kernel.  The argument block is the moving camera's
// (CameraArgs, rm_camera.hpp); the scene blob the launch passes is a swept one (rm_swept_image.hpp).  No device code.
#ifndef RM_CAMERA_SWEPT_HPP
#define RM_CAMERA_SWEPT_HPP

#include "rm_camera.hpp"

// The sample-shade-and-accumulate kernel with the camera of the lane's row and moved lights and shapes that walks the hierarchies
// of the blob it is given (64 lanes a workgroup, arguments: a swept scene blob, CameraArgs).  `bvh` is honoured: an image without
// a hierarchy takes the flat kernel of the moving camera's moving scene (rm_camera_moving_kernel), whose bytes these kernels
// write anyway.  Instantiations of its own: pow_mode x stack 4 or 32.  NULL: no such instantiation.
const void *rm_camera_swept_kernel(bool bvh, int pow_mode, int stack);

#endif
