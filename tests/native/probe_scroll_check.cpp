// probe_scroll_check.cpp — the host-side rules of the scrolling probe grid (software-raytracer_amd/csrc/srt_probe_scroll_host.h) as a
// stand-alone program, built with -fsanitize=address,undefined by tests/test_probe_scroll_native.py.  The index rule (SC1) is swept
// over all shifts in [-n-1, n+1]^3, and over the int32 extremes, for grids 1x1x1, 5x3x2 and 4x1x3: every destination is either
// exposed or has a source inside the grid, retained + exposed = P, the map is injective on the retained probes and agrees with the
// closed-form count; then the moved origin (SC4), the follow shift (SC7), the order of the checks (SC8) and what a scroll makes
// stale (SC5).  Prints "ok <checks>" or the first failure.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "srt_probe_scroll_host.h"

using namespace srt;

static long long checks = 0;
#define CHECK(cond)                                              \
    do {                                                         \
        ++checks;                                                \
        if (!(cond)) {                                           \
            printf("FAILED line %d: %s\n", __LINE__, #cond);     \
            return 1;                                            \
        }                                                        \
    } while (0)

// one shift on one grid: rule SC1's properties
static int sweep(const int32_t counts[3], const int32_t shift[3]) {
    const size_t P = (size_t)counts[0] * (size_t)counts[1] * (size_t)counts[2];
    std::vector<unsigned char> taken(P, 0);
    size_t retained = 0, exposed = 0;
    for (size_t i = 0; i < P; ++i) {
        const size_t untouched = ~(size_t)0;
        size_t j = untouched;
        if (probe_scroll_source(counts, i, shift, &j)) {
            CHECK(j < P);        // a source inside the array
            CHECK(!taken[j]);    // injective on the retained probes
            taken[j] = 1, ++retained;
            // the source is i + shift, axis by axis
            const size_t nx = (size_t)counts[0], ny = (size_t)counts[1];
            CHECK((long long)(j % nx) == (long long)(i % nx) + shift[0] && (long long)((j / nx) % ny) == (long long)((i / nx) % ny) + shift[1] &&
                  (long long)(j / (nx * ny)) == (long long)(i / (nx * ny)) + shift[2]);
        } else {
            CHECK(j == untouched);  // an exposed probe has no source index at all
            ++exposed;
        }
    }
    CHECK(retained + exposed == P);
    CHECK(retained == probe_scroll_retained(counts, shift));
    for (int a = 0; a < 3; ++a) {
        const long long s = shift[a] < 0 ? -(long long)shift[a] : (long long)shift[a];
        if (s >= counts[a]) CHECK(retained == 0);  // such an axis exposes every probe
    }
    if (probe_scroll_shift_is_zero(shift)) CHECK(retained == P);
    return 0;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    static_assert(sizeof(ProbeScrollCall) == 32, "the struct of the header");
    const char* why = nullptr;
    // defaults
    ProbeScrollCall c;
    memset(&c, 0xFF, sizeof c);
    probe_scroll_call_default(c);
    CHECK(c.shift[0] == 0 && c.shift[1] == 0 && c.shift[2] == 0 && c.which == PROBE_SCROLL_COEFFICIENTS && c.flags == 0 && c.reserved[0] == 0 &&
          c.reserved[1] == 0 && c.reserved[2] == 0);
    CHECK(PROBE_SCROLL_COEFFICIENTS == PROBE_HISTORY_COEFFICIENTS && PROBE_SCROLL_MOMENTS == PROBE_HISTORY_MOMENTS && PROBE_SCROLL_STATES == 4);

    // rule SC1, swept
    const int32_t grids[3][3] = {{1, 1, 1}, {5, 3, 2}, {4, 1, 3}};
    const int32_t lo = std::numeric_limits<int32_t>::min(), hi = std::numeric_limits<int32_t>::max();
    for (const auto& n : grids) {
        for (int32_t sz = -n[2] - 1; sz <= n[2] + 1; ++sz)
            for (int32_t sy = -n[1] - 1; sy <= n[1] + 1; ++sy)
                for (int32_t sx = -n[0] - 1; sx <= n[0] + 1; ++sx) {
                    const int32_t s[3] = {sx, sy, sz};
                    if (sweep(n, s)) return 1;
                }
        for (int a = 0; a < 3; ++a)
            for (int32_t e : {lo, lo + 1, hi - 1, hi}) {
                int32_t s[3] = {0, 0, 0};
                s[a] = e;
                if (sweep(n, s)) return 1;
                s[(a + 1) % 3] = e;
                if (sweep(n, s)) return 1;
            }
    }
    // by hand: 3 x 2 x 1 moved by +1 along x
    {
        const int32_t n[3] = {3, 2, 1}, s[3] = {1, 0, 0};
        size_t j = 99;
        CHECK(probe_scroll_source(n, 0, s, &j) && j == 1);
        CHECK(probe_scroll_source(n, 4, s, &j) && j == 5);
        CHECK(!probe_scroll_source(n, 2, s, &j) && !probe_scroll_source(n, 5, s, &j) && j == 5);
        CHECK(probe_scroll_retained(n, s) == 4);
        int64_t v = 7;
        CHECK(probe_scroll_axis(0, lo, 3, &v) == false && probe_scroll_axis(2, hi, 3, &v) == false && v == 7);
        CHECK(probe_scroll_axis(2, -2, 3, &v) && v == 0);
    }

    // rule SC4: the product first, one rounding each
    ProbeGrid g{};
    g.origin[0] = 0.5f, g.origin[1] = 1.0f, g.origin[2] = -2.0f, g.spacing[0] = 0.25f, g.spacing[1] = 0.5f, g.spacing[2] = 2.0f;
    g.counts[0] = 5, g.counts[1] = 3, g.counts[2] = 2;
    float o[3];
    const int32_t s321[3] = {3, -2, 1};
    probe_scroll_origin(g, s321, o);
    CHECK(o[0] == 1.25f && o[1] == 0.0f && o[2] == 0.0f);
    {
        ProbeGrid t = g;  // not dyadic: the same expression, rounded twice
        t.origin[0] = 0.1f, t.spacing[0] = 0.3f;
        const int32_t s7[3] = {7, 0, 0};
        probe_scroll_origin(t, s7, o);
        volatile float step = 7.0f * 0.3f;
        CHECK(o[0] == 0.1f + step && o[1] == t.origin[1] && o[2] == t.origin[2]);
        const int32_t big[3] = {hi, lo, 0};
        probe_scroll_origin(g, big, o);
        CHECK(o[0] == 0.5f + 2147483648.0f * 0.25f && o[1] == 1.0f + -2147483648.0f * 0.5f);
    }

    // rule SC7
    int32_t sh[3] = {9, 9, 9};
    g.origin[0] = g.origin[1] = g.origin[2] = 0.0f, g.spacing[0] = g.spacing[1] = g.spacing[2] = 1.0f, g.counts[0] = g.counts[1] = g.counts[2] = 3;  // centre (1, 1, 1)
    const float p0[3] = {1.0f, 1.0f, 1.0f}, p1[3] = {1.999f, 0.001f, 2.0f}, p2[3] = {3.9f, -0.1f, -1.0f}, p3[3] = {nan, inf, -inf}, p4[3] = {3e38f, -3e38f, 2e6f};
    probe_grid_follow(g, p0, sh);
    CHECK(sh[0] == 0 && sh[1] == 0 && sh[2] == 0);
    probe_grid_follow(g, p1, sh);
    CHECK(sh[0] == 0 && sh[1] == 0 && sh[2] == 1);  // truncation: a whole cell off centre
    probe_grid_follow(g, p2, sh);
    CHECK(sh[0] == 2 && sh[1] == -1 && sh[2] == -2);
    probe_grid_follow(g, p3, sh);
    CHECK(sh[0] == 0 && sh[1] == 1048576 && sh[2] == -1048576);
    probe_grid_follow(g, p4, sh);
    CHECK(sh[0] == 1048576 && sh[1] == -1048576 && sh[2] == 1048576);
    g.counts[1] = 1;  // an axis of one probe: its centre is the origin
    const float p5[3] = {1.0f, 2.5f, 1.0f};
    probe_grid_follow(g, p5, sh);
    CHECK(sh[0] == 0 && sh[1] == 2 && sh[2] == 0);

    // rule SC8: the order of the checks
    ProbeGridState gs;
    ProbeUpdateState us;
    ProbeStatesState st;
    ProbeScrollCall bad = c;
    bad.which = 0;
    CHECK(probe_scroll_check(gs, us, st, false, bad, &why) == RAYS_STATE && strstr(why, "srt_set_scene"));
    CHECK(probe_scroll_check(gs, us, st, true, bad, &why) == RAYS_INVALID_ARG && strstr(why, "which"));
    bad = c, bad.which = 8;
    CHECK(probe_scroll_check(gs, us, st, true, bad, &why) == RAYS_INVALID_ARG && strstr(why, "which"));
    bad = c, bad.flags = 4;
    CHECK(probe_scroll_check(gs, us, st, true, bad, &why) == RAYS_INVALID_ARG && strstr(why, "flags"));
    for (int k = 0; k < 3; ++k) {
        bad = c, bad.reserved[k] = 1;
        CHECK(probe_scroll_check(gs, us, st, true, bad, &why) == RAYS_INVALID_ARG && strstr(why, "reserved"));
    }
    CHECK(probe_scroll_check(gs, us, st, true, c, &why) == RAYS_STATE && strstr(why, "no grid"));
    gs.grid_set = true, gs.grid = g, gs.grid.counts[0] = 5, gs.grid.counts[1] = 3, gs.grid.counts[2] = 2;
    CHECK(probe_scroll_check(gs, us, st, true, c, &why) == RAYS_STATE && strstr(why, "no coefficient history"));
    probe_history_was_reset(us, 0, 29, 0);
    CHECK(probe_scroll_check(gs, us, st, true, c, &why) == RAYS_STATE && strstr(why, "coefficient history's probe count"));
    probe_history_was_reset(us, 0, 30, 0);
    CHECK(probe_scroll_check(gs, us, st, true, c, nullptr) == RAYS_OK);
    ProbeScrollCall all = c;
    all.which = PROBE_SCROLL_WHICH_ALL, all.flags = PROBE_SCROLL_FLAG_ALL, all.shift[0] = hi, all.shift[1] = lo;
    CHECK(probe_scroll_check(gs, us, st, true, all, &why) == RAYS_STATE && strstr(why, "no moment history"));
    probe_history_was_reset(us, 1, 31, 4);
    CHECK(probe_scroll_check(gs, us, st, true, all, &why) == RAYS_STATE && strstr(why, "moment history's probe count"));
    probe_history_was_reset(us, 1, 30, 4);
    CHECK(probe_scroll_check(gs, us, st, true, all, &why) == RAYS_STATE && strstr(why, "no states"));
    input_written(st.states, 29);
    CHECK(probe_scroll_check(gs, us, st, true, all, &why) == RAYS_STATE && strstr(why, "state count"));
    input_written(st.states, 30);
    CHECK(probe_scroll_check(gs, us, st, true, all, &why) == RAYS_OK);
    bad = all, bad.which = PROBE_SCROLL_STATES;  // the records alone need no history
    ProbeUpdateState none;
    CHECK(probe_scroll_check(gs, none, st, true, bad, &why) == RAYS_OK);
    gs.grid.spacing[0] = 3e38f;  // a moved origin that overflows: only with SET_GRID
    CHECK(probe_scroll_check(gs, us, st, true, all, &why) == RAYS_INVALID_ARG && strstr(why, "not finite"));
    all.flags = PROBE_SCROLL_FLAG_COUNT_WORK;
    CHECK(probe_scroll_check(gs, us, st, true, all, &why) == RAYS_OK);

    // rule SC5, and the work record's gate
    LightProbeState lp;
    ProbeDepthState pd;
    int a0 = 0, a1 = 0;
    lp.call.ran = true, lp.last.outputs = LIGHT_PROBE_OUT_ALL, lp.last.dst[0] = &a0, lp.last.dst[1] = &a1, lp.last_probes = 30;
    pd.call.ran = true, pd.last.outputs = 3, pd.last.dst[0] = &a0, pd.last.dst[1] = &a1;
    probe_scroll_stale(lp, pd);
    CHECK(lp.last.outputs == LIGHT_PROBE_OUT_RADIANCE && lp.last.dst[0] == nullptr && lp.last.dst[1] == &a1);
    CHECK(pd.last.outputs == 2 && pd.last.dst[0] == nullptr && pd.last.dst[1] == &a1);
    ProbeBlendCall bc;
    probe_blend_call_default(bc);
    CHECK(probe_blend_check(us, lp, pd, st, true, bc, &why) == RAYS_STATE && strstr(why, "did not write COEFFICIENTS"));
    CallRecord ss;
    CHECK(ss.work() == RAYS_STATE);
    probe_scroll_scrolled(ss, 0);
    CHECK(ss.work() == RAYS_STATE);
    probe_scroll_scrolled(ss, PROBE_SCROLL_FLAG_COUNT_WORK | PROBE_SCROLL_FLAG_SET_GRID);
    CHECK(ss.work() == RAYS_OK);
    CHECK(probe_scroll_grid(1005, 4, 1024) == 252 && probe_scroll_grid(1005, 4, 100) == 100 && probe_scroll_grid(1, 4, 100) == 1);
    printf("ok %lld\n", checks);
    return 0;
}
