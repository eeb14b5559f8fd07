// rm_soft.hpp -- what the host side (rm_soft_host.inc) needs to know about the kernel of the area lights (rm_soft.hip): its
// argument block and the function that hands out a kernel.  No device code.
#ifndef RM_SOFT_HPP
#define RM_SOFT_HPP

#include <stdint.h>

#include "rm_accum.hpp"

namespace rmdev {

struct SoftArgs {
    AccumArgs A;                             // the progressive launch's own block: rays, fold, sum, mean and bytes are its
    const double *offsets;                   // [A.L.n_samples][A.L.H.n_lights][3]; not read where the scene has no lights
};

}  // namespace rmdev

// The sample-shade-and-accumulate kernel with moved lights (64 lanes a workgroup, arguments: scene blob, SoftArgs),
// instantiated as the progressive frames' kernel is (rm_accum.hpp): bvh, pow_mode, stack 4 or 32.  NULL: no such instantiation.
const void *rm_soft_kernel(bool bvh, int pow_mode, int stack);

#endif
