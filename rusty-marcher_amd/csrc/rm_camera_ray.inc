// rm_camera_ray.inc -- the moving camera's one rule: the ray of a sample whose camera is a row of a table
// (include/rusty_marcher_amd.h, "moving camera").  Included by rm_camera.hip and rm_converge_camera.hip behind
// rm_radiance_step.inc and in front of the sample body, which calls it where RM_CAMERA_ROWS is defined.
//
// A row is twelve doubles: (off.x, off.y, off.z, right.xyz, up.xyz, forward.xyz).  The sample's camera stands at
// cam' = cam + off, one addition a component, and looks along the row's basis -- absolute, not an offset.  Steps 1-4 of the
// thin-lens camera follow with cam' and that basis in place of the context's, operation for operation: the direction is
// sample_direction's oriented formula itself, handed a view of the row.  Nothing read from a row forms an address.

namespace rmcamera {

using namespace rmradiance;

// What sample_direction reads of an argument block, with a row's basis in the context's place
struct RowView {
    double width, height, half_fov, ratio;
    double cam_rx, cam_ry, cam_rz, cam_ux, cam_uy, cam_uz, cam_fx, cam_fy, cam_fz;
};

// The ray of the sample at (sx, sy) through the lens point (au, av) = aperture x (u, v), seen from the camera of row `c`.
// A: LensArgs.  `pinhole`: aperture == 0, where the ray leaves cam' itself.
template <class A>
__device__ __forceinline__ void camera_row_ray(const A &q, const double *__restrict__ c, double sx, double sy, double au, double av,
                                               bool pinhole, V3 &orig, V3 &dir) {
    const V3 cam = mk(q.cam_x + c[0], q.cam_y + c[1], q.cam_z + c[2]);
    const RowView v{q.width, q.height, q.half_fov, q.ratio, c[3], c[4], c[5], c[6], c[7], c[8], c[9], c[10], c[11]};
    const V3 D = sample_direction(v, true, sx, sy);
    if (pinhole) {
        orig = cam;
        dir = normalized(D);
    } else {
        const V3 F = mk(cam.x + D.x * q.focus, cam.y + D.y * q.focus, cam.z + D.z * q.focus);
        const V3 lens = mk(cam.x + ((au * v.cam_rx) + (av * v.cam_ux)), cam.y + ((au * v.cam_ry) + (av * v.cam_uy)),
                           cam.z + ((au * v.cam_rz) + (av * v.cam_uz)));
        orig = lens;
        dir = normalized(F - lens);
    }
}

}  // namespace rmcamera
