// rm_swept_image.hpp -- the swept hierarchy of a scene image (include/rusty_marcher_amd.h, "swept hierarchies"): the image's blob
// with the boxes of its sphere and triangle hierarchies refitted to every position a shape can take within per-shape offset
// extents.  Host arithmetic alone (rm_swept_image.cpp: nothing of HIP in sight, like rm_image.cpp); rm_device.hip's
// rm_swept_build copies the result across.  Not part of the public ABI.
#ifndef RM_SWEPT_IMAGE_HPP
#define RM_SWEPT_IMAGE_HPP

#include <string>
#include <vector>

#include "rm_image.hpp"

// `blob` becomes a copy of img.blob in which the nodes at img.H.off_bvh_spheres and img.H.off_bvh_triangles hold boxes that
// bound every primitive at record + off for lo[3 k + c] <= off.c <= hi[3 k + c], k the primitive's shape (img.pid_map); every
// other word is img.blob's.  `d` is the description `img` was built from: a triangle's box takes the z of its vertices, which no
// record holds.  lo, hi: n_shapes x 3 doubles each, finite, lo <= hi; n_shapes: d->n_shapes.  A refusal comes back as a status
// with its text, which names the shape, in `error`, and leaves `blob` alone.  `who`: the caller's name in that text.
rm_status rm_swept_refit(const char *who, const rm_scene_desc *d, const rm_image &img, const double *lo, const double *hi, uint32_t n_shapes,
                         std::vector<double> &blob, std::string &error);

#endif
