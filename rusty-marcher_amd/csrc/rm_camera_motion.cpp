// rm_camera_motion.cpp -- the host arithmetic of the moving camera (include/rusty_marcher_amd.h, "moving camera"): the check of
// an rm_camera_motion and rm_camera_sequence, the fourth sample sequence.  No device, no context, no HIP header.  A unit of its
// own beside rm_sampling.cpp, whose instant (rm_shutter_time) it takes, because its rows are turned by rm_camera_basis_turn,
// which is rm_scene.cpp's: rm_sampling.cpp links without the scene builder and stays that way.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "rm_sampling.hpp"

static rm_status refuse(const std::string &msg) {
    rm_set_host_error(msg);
    return RM_ERR_INVALID_ARG;
}

rm_status rm_check_camera_motion(const char *who, const rm_camera_motion *m) {
    if (!m) return refuse(std::string(who) + ": NULL motion");
    const double v[6] = {m->velocity.x, m->velocity.y, m->velocity.z, m->yaw, m->pitch, m->roll};
    for (double x : v)
        if (!std::isfinite(x)) {
            char buf[224];
            std::snprintf(buf, sizeof buf, "%s: motion = velocity (%g, %g, %g), yaw %g, pitch %g, roll %g is not finite", who, v[0], v[1], v[2], v[3],
                          v[4], v[5]);
            return refuse(buf);
        }
    return RM_OK;
}

extern "C" rm_status rm_camera_sequence(uint32_t first, uint32_t count, const rm_camera_motion *motion, const rm_camera_basis *basis,
                                        double shutter, double *rows) {
    const char *who = "rm_camera_sequence";
    // (rm_motion_sequence's refusals in its order: the rows, then the numbers, then the output)
    if ((uint64_t)first + count > RM_PROGRESSIVE_MAX_SAMPLES) {
        char buf[128];
        std::snprintf(buf, sizeof buf, "%s: first + count = %u + %u is more than %u", who, first, count, RM_PROGRESSIVE_MAX_SAMPLES);
        return refuse(buf);
    }
    if (count == 0u) return RM_OK;
    if (rm_status mst = rm_check_camera_motion(who, motion)) return mst;
    if (rm_status sst = rm_check_velocities(who, nullptr, 0u, shutter)) return sst;
    if (!basis) return refuse(std::string(who) + ": NULL basis");
    if (rm_camera_basis_check(basis) != RM_OK) return refuse(std::string(who) + ": " + rm_get_host_error());
    if (!rows) return refuse(std::string(who) + ": NULL rows");
    const bool turns = !(motion->yaw == 0. && motion->pitch == 0. && motion->roll == 0.);
    // (turned into a row of its own first: a refusal half-way writes nothing)
    for (int pass = turns ? 0 : 1; pass < 2; pass++)
        for (uint32_t k = 0; k < count; k++) {
            const double t = rm_shutter_time(first + k, shutter);            // (row 0: t = 0, the camera as it stands)
            rm_camera_basis b = *basis;                                       // (no turn: the given basis byte for byte)
            if (turns)
                if (rm_camera_basis_turn(basis, motion->yaw * t, motion->pitch * t, motion->roll * t, &b) != RM_OK)
                    return refuse(std::string(who) + ": " + rm_get_host_error());
            if (pass == 0) continue;
            double *r = rows + 12u * (size_t)k;
            r[0] = motion->velocity.x * t;
            r[1] = motion->velocity.y * t;
            r[2] = motion->velocity.z * t;
            std::memcpy(r + 3, &b, sizeof b);
        }
    return RM_OK;
}
