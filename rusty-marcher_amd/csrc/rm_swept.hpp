// rm_swept.hpp -- what the host side (rm_swept_host.inc) needs to know about the kernel of the swept hierarchies (rm_swept.hip):
// the function that hands out a kernel.  The argument block is the moving shapes' (MotionArgs, rm_motion.hpp); the scene blob the
// launch passes is a swept one (rm_swept_image.hpp).  No device code.
#ifndef RM_SWEPT_HPP
#define RM_SWEPT_HPP

#include "rm_motion_shapes.hpp"

// The sample-shade-and-accumulate kernel with moved lights and shapes that walks the hierarchies of the blob it is given (64
// lanes a workgroup, arguments: a swept scene blob, MotionArgs).  `bvh` is honoured: an image without a hierarchy takes the flat
// kernel of the moving shapes (rm_motion_shapes_kernel), whose bytes these kernels write anyway.  Instantiations of its own:
// pow_mode x stack 4 or 32.  NULL: no such instantiation.
const void *rm_swept_kernel(bool bvh, int pow_mode, int stack);

#endif
