// rm_converge_camera_swept.hpp -- what the host side (rm_camera_swept_host.inc) needs to know about the shade kernel of the
// converging frames with a moving camera over a swept hierarchy (rm_converge_camera_swept.hip): the function that hands out a
// kernel.  The argument block is the moving camera's (ConvergeCameraArgs, rm_converge_camera.hpp); the scene blob the launch
// passes is a swept one.  No device code.
#ifndef RM_CONVERGE_CAMERA_SWEPT_HPP
#define RM_CONVERGE_CAMERA_SWEPT_HPP

#include "rm_converge_camera.hpp"

// The shade kernel over the list with the camera of the sample's row and moved lights and shapes that walks the hierarchies of
// the blob it is given (64 lanes a workgroup, arguments: a swept scene blob, ConvergeCameraArgs); the select kernel in front of
// it is rm_converge.hip's.  `bvh` is honoured: an image without a hierarchy takes rm_converge_camera_moving_kernel.  pow_mode x
// stack 4 or 32.  NULL: no such instantiation.
const void *rm_converge_camera_swept_kernel(bool bvh, int pow_mode, int stack);

#endif
