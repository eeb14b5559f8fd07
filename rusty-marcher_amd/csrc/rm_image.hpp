// rm_image.hpp -- the device image of a scene description: header, blob, the queries' pid map and what the launches need to
// know of it.  Built by host arithmetic alone (rm_image.cpp: nothing of HIP in sight, like rm_plan.cpp); rm_device.hip's
// upload compares it with the resident image and copies it across.  Not part of the public ABI.
#ifndef RM_IMAGE_HPP
#define RM_IMAGE_HPP

#include <string>
#include <vector>

#include "rm_internal.h"

struct rm_image {
    rm_dev_header H{};
    std::vector<double> blob;
    std::vector<uint32_t> pid_map;     // the queries' pid -> (index into Scene.shapes, triangle index inside the Obj), 2 words per pid
    double occ_camera_limit = 0.;      // |camera|_1 beyond which the render does not use the occluder masks
    std::vector<unsigned char> empty_sides;   // per pid: the sides of its plane that hold nothing (scenes of up to 64 pids)
    double dead_camera_limit = 0.;     // |camera|_1 beyond which the render does not use them (0: no glass word carries any)
    bool exact_only = false;           // outside what the checked numerics are proven for (rm_image.cpp scene_exact_only)
    bool integer_exponents = false;    // every material's specular_exponent is a small non-negative integer
    uint32_t scene_sig = 0;            // the compiled-in signature its shape counts are (rm_plan.cpp rm_scene_signature; 0: none)
};

struct rm_image_options {
    bool use_bvh = true;               // hierarchies over the spheres / mesh triangles once there are enough of them
    bool shadow_masks = true;          // the shadow rays' occluder masks behind the image (scenes of up to 64 pids)
};

// false: an array of `d` is NULL while its count is not 0 (nothing of such a description may be read)
bool rm_desc_arrays_present(const rm_scene_desc *d);

// The image of `*d` (not NULL).  A description it refuses comes back as a status with its text in `error`.
rm_status rm_build_image(const rm_scene_desc *d, const rm_image_options &opt, rm_image &img, std::string &error);

#endif
