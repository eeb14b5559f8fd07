// rm_converge_moving.hpp -- what the host side (rm_converge_moving_host.inc) needs to know about the shade kernel of the
// converging frames with moving shapes (rm_converge_moving.hip): the function that hands out a kernel.  The argument block is
// the moving spheres' (ConvergeMotionArgs, rm_converge_motion.hpp), whose shape table is read for every shape here.  No device
// code.
#ifndef RM_CONVERGE_MOVING_HPP
#define RM_CONVERGE_MOVING_HPP

#include "rm_converge_motion.hpp"

// The shade kernel over the list with moved lights and shapes (64 lanes a workgroup, arguments: scene blob,
// ConvergeMotionArgs); the select kernel in front of it is rm_converge.hip's, given the block's C.  The family walks flat whatever
// `bvh` says -- a hierarchy's boxes hold for the uploaded records only -- so it has four instantiations: pow_mode x stack 4 or
// 32.  NULL: no such instantiation.
const void *rm_converge_moving_kernel(bool bvh, int pow_mode, int stack);

#endif
