// rm_bounce.hpp -- what the host side (rm_bounce_host.inc) needs to know about the kernels of the diffuse bounce (rm_bounce.hip,
// rm_converge_bounce.hip): their argument blocks and the functions that hand out a kernel.  No device code.
#ifndef RM_BOUNCE_HPP
#define RM_BOUNCE_HPP

#include <stdint.h>

#include "rm_converge.hpp"
#include "rm_soft.hpp"

namespace rmdev {

struct BounceArgs {
    SoftArgs S;                              // the area lights' own block: rays, moved lights, fold, sum, mean and bytes are its
    const double *bounce;                    // [S.A.L.n_samples][2]: points of [0,1)^2; not read where strength == 0
    double strength;                         // finite, >= 0
};

struct ConvergeBounceArgs {
    ConvergeArgs C;                          // the converging launch's own block; C.offsets NULL: lights where the scene image says
    const double *bounce;                    // [table_rows][2]; not read where strength == 0
    double strength;                         // finite, >= 0
};

}  // namespace rmdev

// The sample-shade-and-accumulate kernel with moved lights and a diffuse bounce (64 lanes a workgroup, arguments: scene blob,
// BounceArgs), instantiated as the area lights' kernel is (rm_soft.hpp): bvh, pow_mode, stack 4 or 32.  NULL: no such instantiation.
const void *rm_bounce_kernel(bool bvh, int pow_mode, int stack);
// The converging frames' shade kernel with a diffuse bounce (arguments: scene blob, ConvergeBounceArgs), instantiated as
// rm_converge_shade_kernel is (rm_converge.hpp); the select kernel is rm_converge.hip's own.
const void *rm_converge_bounce_kernel(bool bvh, int pow_mode, int stack, bool offset);

#endif
