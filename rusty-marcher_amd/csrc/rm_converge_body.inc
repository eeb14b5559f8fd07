// rm_converge_body.inc -- the body the shade kernels of the converging frames share: rm_converge.hip's (lights where the scene
// image says, or moved by the sample's row of an offset table), rm_converge_motion.hip's (spheres moved as well) and
// rm_converge_moving.hip's (every shape moved).  Statements,
// not a function: a kernel includes this file as the rest of its body, behind rm_radiance_step.inc, with these names in scope --
//
//   BVH, POW, STACK      the compile-time arguments of radiance_steps
//   scene_blob           the kernel's first argument
//   a                    the launch's ConvergeArgs (rm_converge.hpp)
//   bstack, sums         the workgroup's LDS: 64 words and 64 x 3 doubles
//   lights_of(r)         the rule that says where the lights of table row r stand (rm_trace.inc: StoredLights, OffsetLights)
//   spheres_of(r)        the same for the spheres (StoredSpheres, OffsetSpheres) or for every shape (OffsetShapes)
//   camera_rows          rm_converge_camera.hip alone, which defines RM_CAMERA_ROWS and includes rm_camera_ray.inc: the camera
//                        table, [table_rows][12].  No other unit defines the symbol: each sees the tokens it always saw.
//   bounce_table,        rm_converge_bounce.hip alone, which defines RM_BOUNCE_ROWS: the bounce table, [table_rows][2], the
//   bounce_strength,     strength of the diffuse bounce and the workgroup's 64 x 6 doubles of LDS for it (rm_radiance_step.inc,
//   bounce_park          Bounce).  The same holds for this symbol.
//
// -- the parameters of rm_accum_body.inc's accum_shade, with one difference: both rules are asked inside the loop over the
// groups, once a lane and group, with the lane's own row r = count[pixel] + sample.  r < table_rows in every lane, idle ones
// included (rm_converge.hip, the head of the file, has the argument), so a rule may fetch its row without a predicate.
//
// Why text and not a template as accum_shade is: rm_converge.hip's kernels were written with these statements in them, and a
// function inlined into a kernel comes out of the compiler with its blocks laid out and its scalar registers numbered otherwise
// -- the same figures, other assembly.  Included as text, rm_converge.hip compiles to the assembly it had before the body was
// shared (profiles/converge_motion_resource_usage.txt).
//
// And why not rm_accum_body.inc generalised: there the row, the lens point and the rules are hoisted out of the loop over the
// groups and the divisor is the launch's; here every pixel continues the sequence where it stopped.

    const LensArgs &q = a.L;
    const SceneView sc = global_scene_view(scene_blob, q.H, bstack);

    const uint32_t total = q.rows * q.frame_width;                       // (below 2^31: the host checked)
    const uint32_t listed = min(uniform_u32(a.ws[0]), total);            // read once; held to the frame (rm_converge.hip, the head of the file: a workspace damaged between the launches)
    const uint32_t ns = q.n_samples, P = 64u / ns;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t slot = lane / ns, s = lane % ns;                      // the lane's list entry within the group, its sample of that pixel
    const V3 bg = mk(q.bg_x, q.bg_y, q.bg_z);
#ifndef RM_CAMERA_ROWS
    const V3 cam = mk(q.cam_x, q.cam_y, q.cam_z);
#endif
    const bool pinhole = q.aperture == 0.;                               // wave-uniform

    for (uint32_t g = blockIdx.x; (unsigned long long)g * P < listed; g += gridDim.x) {
        const uint32_t k = g * P + slot;                                 // (g P < listed < 2^31, slot < 64)
        bool on = (slot < P) & (k < listed);
        uint32_t pix = on ? a.ws[1u + k] : 0u;
        on = on & (pix < total);                                         // (the same: an entry that is no pixel is dropped)
        pix = on ? pix : 0u;
        const uint32_t n = on ? min(a.fresh ? 0u : a.count[pix], a.last_first) : 0u;   // (the same: a count changed since the select launch stays a row of the table)
        const uint32_t r = n + s;                                        // the lane's table row, < table_rows in every lane
        const double *row = q.table + 4u * (size_t)r;
        V3 orig = mk(0., 0., 0.), dir = mk(0., 0., -1.);                 // (a lane without a sample holds a harmless ray it never casts)
        if (on) {
            const double sx = (double)(pix % q.frame_width) + row[0], sy = (double)(pix / q.frame_width) + row[1];
#ifdef RM_CAMERA_ROWS
            rmcamera::camera_row_ray(q, camera_rows + 12u * (size_t)r, sx, sy, q.aperture * row[2], q.aperture * row[3], pinhole, orig, dir);
#else
            const V3 D = sample_direction(q, q.oriented != 0u, sx, sy);
            if (pinhole) {
                orig = cam;
                dir = normalized(D);
            } else {
                const double au = q.aperture * row[2], av = q.aperture * row[3];
                const V3 lens = mk(q.cam_x + ((au * q.cam_rx) + (av * q.cam_ux)), q.cam_y + ((au * q.cam_ry) + (av * q.cam_uy)),
                                   q.cam_z + ((au * q.cam_rz) + (av * q.cam_uz)));
                const V3 F = mk(q.cam_x + D.x * q.focus, q.cam_y + D.y * q.focus, q.cam_z + D.z * q.focus);
                orig = lens;
                dir = normalized(F - lens);
            }
#endif
        }
        V3 acc = bg;
        if (q.max_depth != 0u)                                           // wave-uniform
#ifdef RM_BOUNCE_ROWS
            acc = radiance_steps<BVH, POW, STACK>(sc, orig, dir, on, bg, q.max_depth, lights_of(r), spheres_of(r),
                                                  Bounce{bounce_table, bounce_strength, bounce_park, r, pix});
#else
            acc = radiance_steps<BVH, POW, STACK>(sc, orig, dir, on, bg, q.max_depth, lights_of(r), spheres_of(r));
#endif
        sums[lane * 3u] = acc.x; sums[lane * 3u + 1u] = acc.y; sums[lane * 3u + 2u] = acc.z;
        __syncthreads();
        if (on & (s == 0u)) {
            double *sum = a.sum + (size_t)pix * 3u;                      // (pix < rows x frame_width: inside every buffer)
            double *st = a.stats + (size_t)pix * 2u;
            double rx, ry, rz, Y, Q;
            uint32_t t;
            if (n > 0u) {
                rx = sum[0]; ry = sum[1]; rz = sum[2];
                Y = st[0]; Q = st[1];
                t = 0u;
            } else {
                rx = sums[lane * 3u]; ry = sums[lane * 3u + 1u]; rz = sums[lane * 3u + 2u];
                Y = (rx + ry) + rz;
                Q = Y * Y;
                t = 1u;
            }
            for (; t < ns; t++) {                                        // table order (lane + t <= 63: lane = slot ns, slot < P)
                const double cx = sums[(lane + t) * 3u], cy = sums[(lane + t) * 3u + 1u], cz = sums[(lane + t) * 3u + 2u];
                const double y = (cx + cy) + cz;
                rx = rx + cx; ry = ry + cy; rz = rz + cz;
                Y = Y + y;
                Q = Q + y * y;
            }
            sum[0] = rx; sum[1] = ry; sum[2] = rz;
            st[0] = Y; st[1] = Q;
            a.count[pix] = n + ns;
            const double div = (double)(n + ns);                         // (at most 65536: the host checked)
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
