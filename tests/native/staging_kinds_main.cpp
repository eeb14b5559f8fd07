// AddressSanitizer / UBSan exercise of the sampled frames' staging rule (csrc/rm_sampling.cpp, rm_staging_of) with its three
// tick kinds side by side: the progressive tick, the converging tick and the converging tick of the moving shapes.  Links
// rm_sampling.cpp alone; the host error text it reports through lives here.  CPU only.
#include <cassert>
#include <cstdio>
#include <string>
#include <vector>

#include "rusty_marcher_amd.h"
#include "rm_internal.h"
#include "rm_sampling.hpp"

// (rm_scene.cpp's in the library: the one thing rm_sampling.cpp needs of it)
static std::string g_error;
void rm_set_host_error(const std::string &msg) { g_error = msg; }
const char *rm_get_host_error() { return g_error.c_str(); }

struct scene_counts {
    uint32_t lights, spheres, others;        // others: shapes that are not spheres
};

int main() {
    const double radii[2] = {1., 2.};
    const rm_vec3 still[6] = {};
    const rm_vec3 moving[6] = {{1., 0., 0.5}, {0., 2., 0.}, {0., 0., 0.}, {3., 1., 0.}, {0.5, 0.5, 0.5}, {0., -1., 0.}};
    int cases = 0;
    for (const scene_counts &sc : {scene_counts{0u, 0u, 0u}, scene_counts{2u, 0u, 0u}, scene_counts{0u, 0u, 3u}, scene_counts{2u, 0u, 3u},
                                   scene_counts{0u, 3u, 0u}, scene_counts{2u, 3u, 0u}, scene_counts{0u, 3u, 3u}, scene_counts{2u, 3u, 3u}})
        for (bool soft : {false, true})
            for (int motion : {0, 1, 2}) {                              // none; velocities of zero; the test velocities
                const uint32_t shapes = sc.spheres + sc.others;
                rm_sampling_rules r;
                if (soft) { r.soft = true; r.radii = radii; r.n_lights = sc.lights; }
                if (motion) { r.motion = true; r.velocities = motion == 1 ? still : moving; r.n_shapes = shapes; r.shutter = 1.; }
                const rm_staging a = rm_staging_of(RM_TICK_PROGRESSIVE, r, sc.lights, sc.spheres, shapes);
                const rm_staging c = rm_staging_of(RM_TICK_CONVERGING, r, sc.lights, sc.spheres, shapes);
                const rm_staging m = rm_staging_of(RM_TICK_CONVERGING_MOVING, r, sc.lights, sc.spheres, shapes);
                // the two old kinds answer as they did
                assert(a.light_columns == (soft || motion ? sc.lights : 0u) && c.light_columns == a.light_columns);
                assert(a.light_zeros == (motion && !soft) && c.light_zeros == a.light_zeros);
                assert(a.shape_columns == (motion ? shapes : 0u));
                assert(c.shape_columns == (motion && sc.spheres > 0u ? shapes : 0u));
                // the new kind: the converging tick's lights, and a shape table whenever there are velocities and the scene holds
                // a shape -- a sphere or not
                assert(m.light_columns == c.light_columns && m.light_zeros == c.light_zeros);
                assert(m.shape_columns == (motion ? shapes : 0u));
                assert((m.shape_columns > 0u) == (motion && shapes > 0u));
                if (motion && sc.spheres == 0u && sc.others > 0u) assert(c.shape_columns == 0u && m.shape_columns == sc.others);   // the Cornell box
                // the rows the rule asks for are what the fill functions write: not a double more
                std::vector<double> rows(3u * (m.light_columns + m.shape_columns) * 3u + 1u, 7.);
                double *end = rows.data() + 3u * m.light_columns * 3u;
                if (m.light_columns > 0u) assert(rm_fill_light_rows(r, m, 4u, 3u, rows.data()) == RM_OK);
                if (m.shape_columns > 0u) assert(rm_fill_shape_rows(r, 4u, 3u, end) == RM_OK);
                assert(rows.back() == 7.);
                for (size_t i = 0; i + 1u < rows.size(); i++) assert(rows[i] != 7. && (!m.light_zeros || i >= 3u * m.light_columns * 3u || rows[i] == 0.));
                cases++;
            }
    assert(cases == 48);
    std::printf("staging kinds ok: %d cases\n", cases);
    return 0;
}
