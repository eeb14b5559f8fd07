// rm_sampling.hpp -- what the sampled frames (progressive, area lights, moving spheres, converging: the ticks of rm_motion_host.inc
// and rm_converge_motion_host.inc) decide on the host without a device: the three sample sequences of the C ABI, the checks of radii,
// velocities and shutter, the sampling rules of a tick as one view, the identity of the frame a running sum belongs to, and which
// offset tables a tick stages.  rm_sampling.cpp computes them; like rm_plan.cpp it is a host-only unit: this header and it include
// nothing of HIP, and nothing here takes an rm_ctx.  Errors are the host error text (rm_set_host_error); a caller with a context
// copies it over (rm_get_host_error), as rm_camera_orient does.
#ifndef RM_SAMPLING_HPP
#define RM_SAMPLING_HPP

#include <stdint.h>

#include <vector>

#include "rm_internal.h"

#pragma GCC visibility push(hidden)

// A radius is a finite number >= 0, a velocity finite, the shutter a finite number >= 0 (a NaN fails the comparisons)
rm_status rm_check_radii(const char *who, const double *radii, uint32_t n_lights);
rm_status rm_check_velocities(const char *who, const rm_vec3 *velocities, uint32_t n_shapes, double shutter);
// The strength of a diffuse bounce is a finite number >= 0
rm_status rm_check_strength(const char *who, double strength);

// The sampling rules of a tick, a view of the caller's arrays.  soft: area lights of n_lights radii (0 lights' worth of radii is
// not "no radii"); else radii is NULL and n_lights 0.  motion: moving spheres, a velocity for each of n_shapes shapes and the
// shutter (velocities of zero are not "no velocities"); else NULL, 0, 0.
struct rm_sampling_rules {
    bool soft = false;
    const double *radii = nullptr;
    uint32_t n_lights = 0;
    bool motion = false;
    const rm_vec3 *velocities = nullptr;
    uint32_t n_shapes = 0;
    double shutter = 0.;
    // camera: the moving camera's ticks (rm_camera_host.inc), whose frames are their own: the motion's bytes join the key.  The
    // shutter is the one above, with velocities (motion) or without
    const rm_camera_motion *camera = nullptr;
    // bounce: the diffuse bounce's ticks (rm_bounce_host.inc), whose frames are their own: the strength joins the key (a
    // strength of 0 is not "no bounce")
    bool bounce = false;
    double strength = 0.;
};

// The view a sum belongs to, byte for byte (no padding: doubles and pairs of words)
struct rm_progressive_key {
    double fov, half_fov, height, width, ratio;
    uint32_t frame_width, frame_height, max_depth, oriented;
    rm_vec3 background;
    double aperture, focus;
    rm_vec3 camera;
    rm_camera_basis basis;
    uint64_t copies;
    uint32_t soft, n_lights;                 // frames with radii: 1 and the radii's count (their bytes: rm_frame_identity::radii); else 0, 0
    uint32_t motion, n_shapes;               // frames with velocities: 1 (2: the moving shapes' tick sets it) and their count (bytes: rm_frame_identity::velocities)
    double shutter;                          // and the shutter; else 0, 0, 0
    uint32_t camera_moves, _pad;             // frames of the moving camera's ticks: 1 and the bytes of their rm_camera_motion; else zeros
    rm_camera_motion camera_motion;
    uint32_t bounce, _pad2;                  // frames of the diffuse bounce's ticks: 1 and the strength; else zeros
    double strength;
};

// The frame a tick samples: the key and, beside it, copies of the radii and the velocities it was begun with
struct rm_frame_identity {
    rm_progressive_key key;
    std::vector<double> radii;               // empty: point lights
    std::vector<rm_vec3> velocities;         // empty: nothing moves
};

rm_frame_identity rm_frame_identity_of(const rm_params &p, const rm_lens &lens, const rm_vec3 &camera, const rm_camera_basis &basis, bool oriented,
                                       uint64_t upload_copies, const rm_sampling_rules &rules);
// Counts and bytes: a velocity of -0. is not one of 0.
bool rm_same_radii(const rm_frame_identity &a, const rm_frame_identity &b);
bool rm_same_frame(const rm_frame_identity &a, const rm_frame_identity &b);

// The offset tables a tick stages beside the lens table: a motion tick's kernel, and a moving camera's, reads a row for every
// light of the scene -- zeros where the lights are points -- and, with velocities, for every shape; a soft tick's for every radius.  The converging tick stages no shape
// table for a scene without spheres, the progressive one does; the converging tick of the moving shapes, whose kernel reads a
// row of polygons and meshes as well, stages one whenever the scene holds a shape.
enum rm_tick_kind { RM_TICK_PROGRESSIVE, RM_TICK_CONVERGING, RM_TICK_CONVERGING_MOVING };
struct rm_staging {
    uint32_t light_columns;                  // 0: no light table
    bool light_zeros;
    uint32_t shape_columns;                  // 0: no shape table
    uint32_t bounce_columns;                 // 2: a slice of rm_bounce_sequence; 0: no bounce table
};
rm_staging rm_staging_of(rm_tick_kind kind, const rm_sampling_rules &rules, uint32_t scene_lights, uint32_t scene_spheres, uint32_t scene_shapes);

// Rows [first, first + count) of a staged table: 4 doubles of rm_lens_sequence, light_columns x 3 of rm_light_sequence or zeros,
// shape_columns x 3 of rm_motion_sequence, 2 of rm_bounce_sequence
inline rm_status rm_fill_bounce_rows(uint32_t first, uint32_t count, double *out) { return rm_bounce_sequence(first, count, out); }
inline rm_status rm_fill_lens_rows(uint32_t first, uint32_t count, double *out) { return rm_lens_sequence(first, count, out); }
rm_status rm_fill_light_rows(const rm_sampling_rules &rules, const rm_staging &staged, uint32_t first, uint32_t count, double *out);
rm_status rm_fill_shape_rows(const rm_sampling_rules &rules, uint32_t first, uint32_t count, double *out);

// The instant of table row s within a shutter: shutter x phi_17(s), what rm_motion_sequence gives the row -- and
// rm_camera_sequence (rm_camera_motion.cpp), so that the camera and the shapes of a sample share it
double rm_shutter_time(uint32_t s, double shutter);
// A camera motion is six finite numbers (rm_camera_motion.cpp)
rm_status rm_check_camera_motion(const char *who, const rm_camera_motion *motion);

#pragma GCC visibility pop

#endif
