// rm_motion_shapes.hpp -- what the host side (rm_motion_shapes_host.inc) needs to know about the kernel of the moving shapes
// (rm_motion_shapes.hip): the function that hands out a kernel.  The argument block is the moving spheres' (MotionArgs,
// rm_motion.hpp): the same tables, the same map; only the rule that reads them differs.  No device code.
#ifndef RM_MOTION_SHAPES_HPP
#define RM_MOTION_SHAPES_HPP

#include "rm_motion.hpp"

// The sample-shade-and-accumulate kernel with moved lights, spheres, polygons and triangles (64 lanes a workgroup, arguments:
// scene blob, MotionArgs; shape_offsets is read where the scene holds any shape).  The family walks flat whatever `bvh` says,
// as rm_motion_kernel's does, so it has four instantiations: pow_mode x stack 4 or 32.  NULL: no such instantiation.
const void *rm_motion_shapes_kernel(bool bvh, int pow_mode, int stack);

#endif
