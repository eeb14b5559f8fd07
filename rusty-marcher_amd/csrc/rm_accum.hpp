// rm_accum.hpp -- what the host side (rm_accum_host.inc) needs to know about the kernel of the progressive frames
// (rm_accum.hip): its argument block and the function that hands out a kernel.  No device code.
#ifndef RM_ACCUM_HPP
#define RM_ACCUM_HPP

#include <stdint.h>

#include "rm_lens.hpp"

namespace rmdev {

struct AccumArgs {
    LensArgs L;                              // the lens launch's own block: rays and radiance are its; L.frame is not read
    uint32_t n_before, _pad;                 // samples a pixel the sum holds already; 0: the sum is not read
    double *sum;                             // [frame_height][frame_width][3], continued
    double *mean;                            // the same shape, or NULL
    uint8_t *rgb8;                           // [frame_height][frame_width][3] bytes, or NULL
};

}  // namespace rmdev

// The sample-shade-and-accumulate kernel (64 lanes a workgroup, arguments: scene blob, AccumArgs), instantiated as the lens
// kernel is (rm_lens.hpp): bvh, pow_mode, stack 4 or 32.  NULL: no such instantiation.
const void *rm_accum_kernel(bool bvh, int pow_mode, int stack);

#endif
