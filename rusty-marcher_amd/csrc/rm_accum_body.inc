// rm_accum_body.inc -- the body the kernels of the progressive frames share: rm_accum.hip's (lights where the scene image says),
// rm_soft.hip's (lights moved by the lane's row of an offset table), rm_motion.hip's (spheres moved as well) and
// rm_motion_shapes.hip's (every shape moved).  Included
// behind rm_radiance_step.inc.  rm_camera.hip's kernels (the camera moved as well) include it behind rm_camera_ray.inc with
// RM_CAMERA_ROWS defined, which no other unit does: every other unit sees the tokens it always saw.  rm_bounce.hip's kernels (a
// diffuse bounce behind the camera ray's hit) include it with RM_BOUNCE_ROWS defined, under the same rule.
//
// `lights_of(s)`: the rule that says where the lights of table row s stand (rm_trace.inc, StoredLights), asked once a lane
// before the loop over the groups; `spheres_of(s)`: the same for the spheres (StoredSpheres where none is given).  `bstack` (64 words) and `sums` (64 x 3 doubles) are the workgroup's LDS.

namespace rmaccum {

using namespace rmradiance;

struct stored_spheres_of {
    __device__ __forceinline__ StoredSpheres operator()(uint32_t) const { return StoredSpheres(); }
};

template <bool BVH, int POW, int STACK, class LIGHTS_OF, class SPHERES_OF = stored_spheres_of>
__device__ __forceinline__ void accum_shade(const double *__restrict__ scene_blob, const AccumArgs &a, uint32_t *bstack, double *sums,
#ifdef RM_CAMERA_ROWS
                                            const double *__restrict__ camera_rows,   // [n_samples][12]: rmcamera::camera_row_ray
#endif
#ifdef RM_BOUNCE_ROWS
                                            const double *__restrict__ bounce_table,  // [n_samples][2]: rmradiance::bounce_ray
                                            double bounce_strength,
                                            double *bounce_park,                      // 64 x 6 doubles of LDS
#endif
                                            LIGHTS_OF lights_of, SPHERES_OF spheres_of = SPHERES_OF()) {
    const LensArgs &q = a.L;
    const SceneView sc = global_scene_view(scene_blob, q.H, bstack);

    const uint32_t total = q.rows * q.frame_width;                       // (below 2^31: the host checked)
    const uint32_t ns = q.n_samples, P = 64u / ns;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t slot = lane / ns, s = lane % ns;                      // the lane's pixel within the group, its table row
    const double *row = q.table + 4u * s;                                // (s < n_samples in every lane)
    const double dx = row[0], dy = row[1];
    const double au = q.aperture * row[2], av = q.aperture * row[3];
    const auto lights = lights_of(s);
    const auto spheres = spheres_of(s);
    const V3 bg = mk(q.bg_x, q.bg_y, q.bg_z);
#ifndef RM_CAMERA_ROWS
    const V3 cam = mk(q.cam_x, q.cam_y, q.cam_z);
    const V3 lens = mk(q.cam_x + ((au * q.cam_rx) + (av * q.cam_ux)), q.cam_y + ((au * q.cam_ry) + (av * q.cam_uy)),
                       q.cam_z + ((au * q.cam_rz) + (av * q.cam_uz)));
#endif
    const bool pinhole = q.aperture == 0.;                               // wave-uniform
    const bool resume = a.n_before > 0u;                                 // wave-uniform
    const double div = (double)(a.n_before + ns);                        // (at most 65536: the host checked)

    for (uint32_t g = blockIdx.x; (unsigned long long)g * P < total; g += gridDim.x) {
        const uint32_t k = g * P + slot;                                 // (g P < total < 2^31, slot < 64)
        const bool on = (slot < P) & (k < total);
        const uint32_t pix = on ? k : 0u;
        V3 orig = mk(0., 0., 0.), dir = mk(0., 0., -1.);                 // (a lane without a sample holds a harmless ray it never casts)
        if (on) {
            const double sx = (double)(pix % q.frame_width) + dx, sy = (double)(pix / q.frame_width) + dy;
#ifdef RM_CAMERA_ROWS
            // the row is fetched here, a group at a time, not in front of the loop: twelve values alive across the ray walk
            // cost a wave a SIMD (rm_camera.hip, the head of the file)
            rmcamera::camera_row_ray(q, camera_rows + 12u * s, sx, sy, au, av, pinhole, orig, dir);
#else
            const V3 D = sample_direction(q, q.oriented != 0u, sx, sy);
            if (pinhole) {
                orig = cam;
                dir = normalized(D);
            } else {
                const V3 F = mk(q.cam_x + D.x * q.focus, q.cam_y + D.y * q.focus, q.cam_z + D.z * q.focus);
                orig = lens;
                dir = normalized(F - lens);
            }
#endif
        }
#ifdef RM_BOUNCE_ROWS
        // (the row is fetched in the step that bounces: here only its index and the pixel go along)
        const V3 acc = q.max_depth == 0u ? bg : radiance_steps<BVH, POW, STACK>(sc, orig, dir, on, bg, q.max_depth, lights, spheres,
                                                                               Bounce{bounce_table, bounce_strength, bounce_park, s, pix});
#else
        const V3 acc = q.max_depth == 0u ? bg : radiance_steps<BVH, POW, STACK>(sc, orig, dir, on, bg, q.max_depth, lights, spheres);
#endif
        sums[lane * 3u] = acc.x; sums[lane * 3u + 1u] = acc.y; sums[lane * 3u + 2u] = acc.z;
        __syncthreads();
        if (on & (s == 0u)) {
            double *sum = a.sum + (size_t)pix * 3u;                      // (pix < rows x frame_width: inside the three buffers)
            double rx, ry, rz;
            uint32_t t;
            if (resume) {
                rx = sum[0]; ry = sum[1]; rz = sum[2];
                t = 0u;
            } else {
                rx = sums[lane * 3u]; ry = sums[lane * 3u + 1u]; rz = sums[lane * 3u + 2u];
                t = 1u;
            }
            for (; t < ns; t++) {                                        // table order (lane + t <= 63: lane = slot ns, slot < P)
                rx = rx + sums[(lane + t) * 3u]; ry = ry + sums[(lane + t) * 3u + 1u]; rz = rz + sums[(lane + t) * 3u + 2u];
            }
            sum[0] = rx; sum[1] = ry; sum[2] = rz;
            const double mx = rx / div, my = ry / div, mz = rz / div;
            if (a.mean) {
                double *out = a.mean + (size_t)pix * 3u;
                out[0] = mx; out[1] = my; out[2] = mz;
            }
            if (a.rgb8) {
                uint8_t *out = a.rgb8 + (size_t)pix * 3u;
                out[0] = to_byte(mx); out[1] = to_byte(my); out[2] = to_byte(mz);
            }
        }
        __syncthreads();                                                 // the next group's answers overwrite `sums`
    }
}

}  // namespace rmaccum
