// rm_query.hpp -- what the host side (rm_query_host.inc) needs to know about the query kernels
// (rm_query.hip): their argument block and the function that hands out a kernel.  No device code.
#ifndef RM_QUERY_HPP
#define RM_QUERY_HPP

#include <stdint.h>

#include "rm_internal.h"

namespace rmdev {

enum { RM_QUERY_CLOSEST = 0, RM_QUERY_OCCLUDED = 1, RM_QUERY_PIXELS = 2 };

struct QueryArgs {
    rm_dev_header H;
    const uint32_t *pid_map;                 // 2 words per pid: index into Scene.shapes, triangle index inside the Obj
    // ray lists (RM_QUERY_CLOSEST / RM_QUERY_OCCLUDED): one lane per ray
    const rm_vec3 *origins, *directions;
    uint32_t n_rays;
    // pixels (RM_QUERY_PIXELS): one wave per TILE_W x TILE_H tile of the render, or one lane for one pixel
    uint32_t frame_width;
    uint32_t tiles_per_row, n_tiles;         // n_tiles == 0: the single pixel (pick_x, pick_y) into hits[0]
    uint32_t pick_x, pick_y;
    const double *bp_x, *bp_y;               // the render's backproject tables (rm_device.hip backproject_tables)
    double cam_x, cam_y, cam_z;
    rm_hit *hits;                            // RM_QUERY_CLOSEST / RM_QUERY_PIXELS
    uint8_t *occluded;                       // RM_QUERY_OCCLUDED
    // RM_QUERY_PIXELS under an oriented camera (rm_camera_orient): right, up, forward, as the oriented render kernels get them
    double cam_rx, cam_ry, cam_rz, cam_ux, cam_uy, cam_uz, cam_fx, cam_fy, cam_fz;
};

// The ranged queries (rm_*_ranged, rm_visible_segments, rm_lights_visible): kernels and an argument block of their own, beside
// the ones above.
enum { RM_RANGED_CLOSEST = 0, RM_RANGED_OCCLUDED = 1, RM_RANGED_SEGMENTS = 2, RM_RANGED_LIGHTS = 3 };

struct RangedArgs {
    rm_dev_header H;
    const uint32_t *pid_map;
    // one lane per answer: ray (CLOSEST / OCCLUDED), segment (SEGMENTS), (point, light) pair with the point index major (LIGHTS)
    uint64_t n;
    const rm_vec3 *a, *b;                    // origins, directions | from, to | points, normals
    const rm_range *ranges;                  // CLOSEST / OCCLUDED
    double skin;                             // SEGMENTS
    uint32_t n_lights, mode;                 // LIGHTS (mode: RM_LIGHTS_AS_RENDERED / RM_LIGHTS_CLIPPED)
    rm_hit *hits;                            // CLOSEST
    uint8_t *out;                            // OCCLUDED: occluded; SEGMENTS: visible; LIGHTS: lit
};

}  // namespace rmdev

// The kernel of a ranged query launch (64 lanes a workgroup, arguments: scene blob, RangedArgs).
const void *rm_ranged_kernel(int kind, bool bvh);

// The kernel of a query launch (64 lanes a workgroup, arguments: scene blob, QueryArgs).
// bvh: the scene carries a hierarchy (rm_dev_header::off_bvh_spheres / off_bvh_triangles).
// oriented (RM_QUERY_PIXELS only): the pixels' rays are formed from the camera's basis.
const void *rm_query_kernel(int kind, bool bvh, bool oriented);

#endif
