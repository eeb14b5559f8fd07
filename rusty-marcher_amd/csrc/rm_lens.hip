// rm_lens.hip -- the thin-lens camera: depth-of-field frames (include/rusty_marcher_amd.h, "thin-lens camera").
//
// One launch covers the rows a render writes, no pixel list and nothing through the host:
//
//   shade    the radiance ray step (radiance_steps, rm_radiance_step.inc -- the radiance kernels' own, not a copy) over every
//            pixel of [0, rows x frame_width), n_samples rays each.  A wave takes groups of P = 64 / n_samples consecutive
//            pixels; lane l < P n_samples casts table row l % n_samples of the group's pixel l / n_samples, so the rays of a
//            pixel sit in neighbouring lanes and walk the scene together.  The other lanes, and lanes past the last pixel,
//            have their `on` off from the start, as the radiance kernel's tail lanes.  After the ray steps every lane puts its
//            answer into LDS (64 x 24 B); the lane of row 0 adds its pixel's entries in table order, divides once and stores
//            the pixel.  No sample ever reaches global memory.
//            The grid is what the device holds at once, at most what the frame needs; a workgroup loops over the groups
//            g = blockIdx.x, + gridDim.x, ... while g P < rows x frame_width.
//
//   ray      table row (dx, dy, u, v): D = sample_direction(x + dx, y + dy); F = cam + D focus; O = cam + (aperture u right +
//            aperture v up); the ray leaves O along normalized(F - O).  Every product and sum is rounded once: the unit is
//            compiled with contraction off and this is the strict flavour.  aperture == 0 (wave-uniform, a kernel argument)
//            casts the sample ray itself, cam along normalized(D): the refine kernel's ray, bit for bit.
//
// A lane's table row is loaded once, in front of the group loop, and stays in registers (8 VGPRs): see DESIGN.md section 6g for
// the resource-usage line that decided it.
//
// Strict flavour, scene in global memory, occluder masks off: a sample is what rm_radiance_rays returns for its ray.
#define RM_KERNEL_FAST 0
#include "rm_render_kernel.hpp"
#include "rm_lens.hpp"

using namespace rmdev;
using namespace rmdev_strict;

#include "rm_radiance_step.inc"

namespace rmlens {

using namespace rmradiance;

template <bool BVH, int POW, int STACK>
__global__ __launch_bounds__(64) void rm_lens_shade_t(const double *__restrict__ scene_blob, LensArgs q) {
    __shared__ uint32_t bstack[64];
    __shared__ double sums[64 * 3];
    const SceneView sc = global_scene_view(scene_blob, q.H, bstack);

    const uint32_t total = q.rows * q.frame_width;                       // (below 2^31: the host checked)
    const uint32_t ns = q.n_samples, P = 64u / ns;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t slot = lane / ns, s = lane % ns;                      // the lane's pixel within the group, its table row
    const double *row = q.table + 4u * s;                                // (s < n_samples in every lane)
    const double dx = row[0], dy = row[1];
    const double au = q.aperture * row[2], av = q.aperture * row[3];
    const V3 bg = mk(q.bg_x, q.bg_y, q.bg_z);
    const V3 cam = mk(q.cam_x, q.cam_y, q.cam_z);
    // the lane's point of the lens: the same for every pixel it takes
    const V3 lens = mk(q.cam_x + ((au * q.cam_rx) + (av * q.cam_ux)), q.cam_y + ((au * q.cam_ry) + (av * q.cam_uy)),
                       q.cam_z + ((au * q.cam_rz) + (av * q.cam_uz)));
    const bool pinhole = q.aperture == 0.;                               // wave-uniform

    for (uint32_t g = blockIdx.x; (unsigned long long)g * P < total; g += gridDim.x) {
        const uint32_t k = g * P + slot;                                 // (g P < total < 2^31, slot < 64)
        const bool on = (slot < P) & (k < total);
        const uint32_t pix = on ? k : 0u;
        V3 orig = mk(0., 0., 0.), dir = mk(0., 0., -1.);                 // (a lane without a sample holds a harmless ray it never casts)
        if (on) {
            const double sx = (double)(pix % q.frame_width) + dx, sy = (double)(pix / q.frame_width) + dy;
            const V3 D = sample_direction(q, q.oriented != 0u, sx, sy);
            if (pinhole) {
                orig = cam;
                dir = normalized(D);
            } else {
                const V3 F = mk(q.cam_x + D.x * q.focus, q.cam_y + D.y * q.focus, q.cam_z + D.z * q.focus);
                orig = lens;
                dir = normalized(F - lens);
            }
        }
        // renderer.rs:262-264 at n_recursion = 1: no ray is cast under a cap of 0 (wave-uniform)
        const V3 acc = q.max_depth == 0u ? bg : radiance_steps<BVH, POW, STACK>(sc, orig, dir, on, bg, q.max_depth);
        sums[lane * 3u] = acc.x; sums[lane * 3u + 1u] = acc.y; sums[lane * 3u + 2u] = acc.z;
        __syncthreads();
        if (on & (s == 0u)) {
            double rx = sums[lane * 3u], ry = sums[lane * 3u + 1u], rz = sums[lane * 3u + 2u];
            for (uint32_t t = 1u; t < ns; t++) {                         // table order (lane + t <= 63: lane = slot ns, slot < P)
                rx = rx + sums[(lane + t) * 3u]; ry = ry + sums[(lane + t) * 3u + 1u]; rz = rz + sums[(lane + t) * 3u + 2u];
            }
            const double div = (double)ns;
            double *out = q.frame + (size_t)pix * 3u;
            out[0] = rx / div; out[1] = ry / div; out[2] = rz / div;
        }
        __syncthreads();                                                 // the next group's answers overwrite `sums`
    }
}

}  // namespace rmlens

using namespace rmlens;

const void *rm_lens_kernel(bool bvh, int pow_mode, int stack) {
    RM_SHADING_TABLE(RM_SHADING_KERNEL, rm_lens_shade_t)
    return nullptr;
}
