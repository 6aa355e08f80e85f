// probe_grid_check.cpp — the host-side rules of probe-grid shading (software-raytracer_amd/csrc/srt_probe_grid_host.h) as a stand-alone
// program, built with -fsanitize=address,undefined by tests/test_probe_grid_native.py: which grids are accepted, the positions
// (exactly nx*ny*nz float4, the kernel's expression), the defaults, the order of a call's checks, the coefficient input and the
// work record's rule.  Prints "ok <checks>" or the first failure.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "srt_probe_grid_host.h"

using namespace srt;

static int checks = 0;
#define CHECK(cond)                                              \
    do {                                                         \
        ++checks;                                                \
        if (!(cond)) {                                           \
            printf("FAILED line %d: %s\n", __LINE__, #cond);     \
            return 1;                                            \
        }                                                        \
    } while (0)

static ProbeGrid grid(float ox, float oy, float oz, float sx, float sy, float sz, int nx, int ny, int nz) {
    ProbeGrid g;
    g.origin[0] = ox, g.origin[1] = oy, g.origin[2] = oz, g.spacing[0] = sx, g.spacing[1] = sy, g.spacing[2] = sz;
    g.counts[0] = nx, g.counts[1] = ny, g.counts[2] = nz;
    return g;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    static_assert(sizeof(ProbeGrid) == 36 && sizeof(ProbeGridCall) == 32, "the structs of the header");
    const char* why = nullptr;
    // grids
    CHECK(probe_grid_check(grid(0, 0, 0, 1, 1, 1, 1, 1, 1), &why) == RAYS_OK);
    CHECK(probe_grid_check(grid(-1e30f, 5, 0, 1e-30f, 1e30f, 1, 1024, 1024, 1024), nullptr) == RAYS_OK);  // exactly 2^30 probes
    CHECK(probe_grid_check(grid(0, 0, 0, 1, 1, 1, 1025, 1024, 1024), &why) == RAYS_INVALID_ARG && strstr(why, "2^30"));
    CHECK(probe_grid_check(grid(0, 0, 0, 1, 1, 1, 0x7fffffff, 0x7fffffff, 0x7fffffff), nullptr) == RAYS_INVALID_ARG);  // (no overflow on the way)
    CHECK(probe_grid_check(grid(0, 0, 0, 1, 1, 1, 0x7fffffff, 0x7fffffff, 1), nullptr) == RAYS_INVALID_ARG);
    for (int a = 0; a < 3; ++a) {
        ProbeGrid g = grid(0, 0, 0, 1, 1, 1, 2, 2, 2);
        g.counts[a] = 0;
        CHECK(probe_grid_check(g, &why) == RAYS_INVALID_ARG && strstr(why, "counts"));
        g.counts[a] = -5;
        CHECK(probe_grid_check(g, nullptr) == RAYS_INVALID_ARG);
        g.counts[a] = 2;
        const float bad_spacing[] = {nan, inf, -inf, 0.0f, -0.0f, -1.0f};
        for (float s : bad_spacing) {
            g.spacing[a] = s;
            CHECK(probe_grid_check(g, &why) == RAYS_INVALID_ARG && strstr(why, "spacing"));
        }
        g.spacing[a] = 1e-38f;
        CHECK(probe_grid_check(g, nullptr) == RAYS_OK);
        const float bad_origin[] = {nan, inf, -inf};
        for (float o : bad_origin) {
            g.origin[a] = o;
            CHECK(probe_grid_check(g, &why) == RAYS_INVALID_ARG && strstr(why, "origin"));
        }
    }
    // positions: exactly nx * ny * nz float4 (the sanitizer watches the end of the vector), index order, the kernel's expression
    {
        const ProbeGrid g = grid(0.1f, -0.7f, 3.3f, 0.3f, 0.7f, 1.1f, 3, 4, 2);
        CHECK(probe_grid_probes(g) == 24);
        std::vector<float> p(4 * 24);
        probe_grid_positions(g, p.data());
        for (int iz = 0; iz < 2; ++iz)
            for (int iy = 0; iy < 4; ++iy)
                for (int ix = 0; ix < 3; ++ix) {
                    const float* q = &p[4 * (size_t)(ix + 3 * (iy + 4 * iz))];
                    volatile float sx = (float)ix * 0.3f, sy = (float)iy * 0.7f, sz = (float)iz * 1.1f;
                    CHECK(q[0] == 0.1f + sx && q[1] == -0.7f + sy && q[2] == 3.3f + sz && q[3] == 0.0f);
                }
        std::vector<float> one(4);
        probe_grid_positions(grid(7, 8, 9, 1, 1, 1, 1, 1, 1), one.data());
        CHECK(one[0] == 7 && one[1] == 8 && one[2] == 9 && one[3] == 0);
    }
    // defaults
    ProbeGridCall c;
    memset(&c, 0xff, sizeof c);
    probe_grid_call_default(c);
    CHECK(c.row_begin == 0 && c.row_end == 0 && c.flags == 0 && c.reserved[0] == 0 && c.reserved[1] == 0);
    CHECK(c.band_weight[0] == 3.14159274f && c.band_weight[1] == 2.09439516f && c.band_weight[2] == 0.785398185f);
    // a call's checks, in the header's order
    ProbeGridState s;
    const bool none[PROBE_GRID_GUIDES] = {false, false, false, false}, three[PROBE_GRID_GUIDES] = {true, true, true, false},
               all[PROBE_GRID_GUIDES] = {true, true, true, true};
    c.row_begin = 0, c.row_end = 20;
    ProbeGridCall bad = c;
    bad.flags = 16;
    CHECK(probe_grid_check_shade(s, bad, false, 20, none, &why) == RAYS_STATE && strstr(why, "srt_set_scene"));  // the scene first
    CHECK(probe_grid_check_shade(s, bad, true, 20, none, &why) == RAYS_INVALID_ARG && strstr(why, "flags"));    // the arguments before the inputs
    bad = c, bad.row_end = 21;
    CHECK(probe_grid_check_shade(s, bad, true, 20, none, &why) == RAYS_INVALID_ARG && strstr(why, "band"));
    bad = c, bad.row_begin = 20;
    CHECK(probe_grid_check_shade(s, bad, true, 20, none, nullptr) == RAYS_INVALID_ARG);
    bad = c, bad.row_begin = -1;
    CHECK(probe_grid_check_shade(s, bad, true, 20, none, nullptr) == RAYS_INVALID_ARG);
    bad = c, bad.row_end = 21, bad.flags = 16;  // the band before the flags
    CHECK(probe_grid_check_shade(s, bad, true, 20, none, &why) == RAYS_INVALID_ARG && strstr(why, "band"));
    for (int k = 0; k < 2; ++k) {
        bad = c, bad.reserved[k] = 1;
        CHECK(probe_grid_check_shade(s, bad, true, 20, none, &why) == RAYS_INVALID_ARG && strstr(why, "reserved"));
    }
    for (int k = 0; k < 3; ++k) {
        bad = c, bad.band_weight[k] = nan;
        CHECK(probe_grid_check_shade(s, bad, true, 20, none, &why) == RAYS_INVALID_ARG && strstr(why, "NaN"));
        bad.band_weight[k] = -inf;  // (not a NaN)
        CHECK(probe_grid_check_shade(s, bad, true, 20, none, &why) == RAYS_STATE && strstr(why, "no grid"));
    }
    CHECK(probe_grid_check_shade(s, c, true, 20, all, &why) == RAYS_STATE && strstr(why, "no grid"));
    s.grid = grid(0, 0, 0, 1, 1, 1, 5, 3, 5), s.grid_set = true;
    CHECK(probe_grid_check_shade(s, c, true, 20, all, &why) == RAYS_STATE && strstr(why, "no coefficients"));
    input_written(s.coefficients, 74);
    CHECK(probe_grid_check_shade(s, c, true, 20, none, &why) == RAYS_STATE && strstr(why, "OBJECT"));  // a guide before the count
    const bool no_position[PROBE_GRID_GUIDES] = {true, true, false, true};
    CHECK(probe_grid_check_shade(s, c, true, 20, no_position, &why) == RAYS_STATE && strstr(why, "POSITION"));
    CHECK(probe_grid_check_shade(s, c, true, 20, three, &why) == RAYS_STATE && strstr(why, "nx * ny * nz"));
    input_written(s.coefficients, 75);
    CHECK(probe_grid_check_shade(s, c, true, 20, three, nullptr) == RAYS_OK);
    c.flags = PROBE_GRID_FLAG_ALBEDO;
    CHECK(probe_grid_check_shade(s, c, true, 20, three, &why) == RAYS_STATE && strstr(why, "ALBEDO"));
    CHECK(probe_grid_check_shade(s, c, true, 20, all, nullptr) == RAYS_OK);
    c.flags = PROBE_GRID_FLAG_ALL;
    CHECK(probe_grid_check_shade(s, c, true, 20, all, nullptr) == RAYS_OK);
    // a bound array comes first, and NULL, 0 returns to the own one
    int dummy = 0;
    CHECK(input_bind(s.coefficients, &dummy, 76, PROBE_GRID_MAX_PROBES) == RAYS_OK);
    CHECK(probe_grid_check_shade(s, c, true, 20, all, &why) == RAYS_STATE && strstr(why, "nx * ny * nz"));
    CHECK(input_bind(s.coefficients, &dummy, PROBE_GRID_MAX_PROBES + 1, PROBE_GRID_MAX_PROBES) == RAYS_INVALID_ARG && s.coefficients.count() == 76);
    CHECK(input_bind(s.coefficients, nullptr, 0, PROBE_GRID_MAX_PROBES) == RAYS_OK && s.coefficients.count() == 75);
    // the work record: only of a last call that counted
    CHECK(s.call.work() == RAYS_STATE);
    probe_grid_shaded(s, PROBE_GRID_FLAG_VISIBILITY);
    CHECK(s.call.work() == RAYS_STATE);
    probe_grid_shaded(s, PROBE_GRID_FLAG_COUNT_WORK);
    CHECK(s.call.work() == RAYS_OK);
    probe_grid_shaded(s, 0);
    CHECK(s.call.work() == RAYS_STATE);
    printf("ok %d\n", checks);
    return 0;
}
