// rm_converge.hpp -- what the host side (rm_converge_host.inc) needs to know about the kernels of the converging frames
// (rm_converge.hip): their argument block and the functions that hand out a kernel.  No device code.
#ifndef RM_CONVERGE_HPP
#define RM_CONVERGE_HPP

#include <stdint.h>

#include "rm_lens.hpp"

#define RM_CONVERGE_SELECT_LANES 256

namespace rmdev {

struct ConvergeArgs {
    LensArgs L;                              // the lens launch's own block: rays and radiance are its; L.table has table_rows rows, L.frame is not read
    double tolerance;                        // rm_converge's three
    uint32_t min_samples, max_samples;
    uint32_t fresh;                          // != 0: every count is 0 and sum, stats and count are not read
    uint32_t last_first;                     // table_rows - n_samples: the last row a pixel's slice may begin at
    double *sum;                             // [frame_height][frame_width][3], continued
    double *stats;                           // [frame_height][frame_width][2]: (Y, Q)
    uint32_t *count;                         // [frame_height][frame_width]
    uint32_t *ws;                            // the list: its length, then the pixels' indices
    double *mean;                            // the sum's shape, or NULL
    uint8_t *rgb8;                           // [frame_height][frame_width][3] bytes, or NULL
    uint8_t *mask;                           // [frame_height][frame_width] bytes, or NULL
    const double *offsets;                   // [table_rows][L.H.n_lights][3]; the kernels with stored lights never read it
};

}  // namespace rmdev

// The select kernel (RM_CONVERGE_SELECT_LANES lanes a workgroup, one lane a pixel; argument: ConvergeArgs).
const void *rm_converge_select_kernel();
// The shade kernel over the list (64 lanes a workgroup, arguments: scene blob, ConvergeArgs), instantiated as the progressive
// frames' kernel is (rm_accum.hpp): bvh, pow_mode, stack 4 or 32 -- each with the lights where the scene image says
// (offset == false) and moved by the sample's row of the offset table.  NULL: no such instantiation.
const void *rm_converge_shade_kernel(bool bvh, int pow_mode, int stack, bool offset);

#endif
