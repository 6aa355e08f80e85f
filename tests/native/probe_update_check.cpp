// probe_update_check.cpp — the host-side rules of the per-frame probe updates (software-raytracer_amd/csrc/srt_probe_update_host.h)
// as a stand-alone program, built with -fsanitize=address,undefined by tests/test_probe_update_native.py: the defaults, which
// parameters are accepted and in which order the checks come, the sizes of the list and of the histories, what a read returns,
// the list bound for tracing, the histories' sizes and what the blend takes as its new data.  Prints "ok <checks>" or the first
// failure.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>

#include "srt_probe_update_host.h"

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

// srt_read_probe_list_output's rule as srt_capi.hip composes it: the shared record's read of the one output, the byte count of the last listing
static RaysStatus read_probe_list_output(const ProbeUpdateState& s, const void** src, size_t* bytes) {
    if (!(*src = s.list_last.read(1u, 0))) return RAYS_STATE;
    *bytes = probe_list_bytes(s.list_probes);
    return RAYS_OK;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    static_assert(sizeof(ProbeListCall) == 16 && sizeof(ProbeBlendCall) == 24, "the structs of the header");
    const char* why = nullptr;
    // defaults
    ProbeListCall lc;
    probe_list_call_default(lc);
    CHECK(lc.skip_mask == (PROBE_BURIED | PROBE_IDLE) && lc.flags == 0 && lc.reserved[0] == 0 && lc.reserved[1] == 0);
    ProbeBlendCall bc;
    probe_blend_call_default(bc);
    CHECK(bc.hysteresis == 0.9f && bc.fast_hysteresis == 0.5f && bc.depth_hysteresis == 0.9f && bc.change_threshold == 0.25f && bc.flags == 0 && bc.reserved == 0);
    CHECK(PROBE_STATE_BITS == 15 && PROBE_LIST_HEADER == 4 && PROBE_LIST_NONE == 0xFFFFFFFFu);
    // sizes
    CHECK(probe_list_words(1) == 5 && probe_list_bytes(8925) == 4 * 8929 && probe_list_bytes((size_t)1 << 30) == ((size_t)1 << 32) + 16);
    CHECK(probe_history_slot(1) == 0 && probe_history_slot(2) == 1 && probe_history_slot(0) == -1 && probe_history_slot(3) == -1);
    CHECK(probe_history_bytes(0, 210, 0) == 210 * 9 * 16 && probe_history_bytes(1, 210, 8) == 210 * 64 * 16 && probe_history_bytes(1, 3, 16) == 3 * 256 * 16);
    // srt_list_probes' checks, in the header's order
    ProbeGridState g;
    ProbeStatesState st;
    ProbeListCall bad = lc;
    bad.flags = 2;
    CHECK(probe_list_check(g, st, false, bad, &why) == RAYS_STATE && strstr(why, "srt_set_scene"));  // the scene first
    CHECK(probe_list_check(g, st, true, bad, &why) == RAYS_INVALID_ARG && strstr(why, "flags"));     // arguments before the states
    bad = lc, bad.skip_mask = 16;
    CHECK(probe_list_check(g, st, true, bad, &why) == RAYS_INVALID_ARG && strstr(why, "skip_mask"));
    bad = lc, bad.reserved[1] = 1;
    CHECK(probe_list_check(g, st, true, bad, &why) == RAYS_INVALID_ARG && strstr(why, "reserved"));
    CHECK(probe_list_check(g, st, true, lc, &why) == RAYS_STATE && strstr(why, "no states"));
    input_written(st.states, 24);
    CHECK(probe_list_check(g, st, true, lc, nullptr) == RAYS_OK);  // without a grid any count goes
    g.grid_set = true;
    g.grid.counts[0] = 3, g.grid.counts[1] = 2, g.grid.counts[2] = 5;
    CHECK(probe_list_check(g, st, true, lc, &why) == RAYS_STATE && strstr(why, "nx * ny * nz"));
    g.grid.counts[2] = 4;
    for (uint32_t m = 0; m < 16; ++m) {  // any subset of the four bits
        bad = lc, bad.skip_mask = m, bad.flags = PROBE_LIST_FLAG_COUNT_WORK;
        CHECK(probe_list_check(g, st, true, bad, &why) == RAYS_OK);
    }
    // what a read returns
    ProbeUpdateState s;
    const void* src = nullptr;
    size_t bytes = 0;
    CHECK(read_probe_list_output(s, &src, &bytes) == RAYS_STATE && s.list_call.work() == RAYS_STATE);
    char own[16], other[16];
    probe_list_listed(s, 24, 0, own);
    CHECK(read_probe_list_output(s, &src, &bytes) == RAYS_OK && src == own && bytes == 28 * 4 && s.list_call.work() == RAYS_STATE);
    probe_list_listed(s, 7, PROBE_LIST_FLAG_COUNT_WORK, own);
    CHECK(read_probe_list_output(s, &src, &bytes) == RAYS_OK && bytes == 11 * 4 && s.list_call.work() == RAYS_OK);
    s.list_last.released(0, other);  // another buffer: nothing happens
    CHECK(read_probe_list_output(s, &src, &bytes) == RAYS_OK);
    s.list_last.released(0, own);
    CHECK(read_probe_list_output(s, &src, &bytes) == RAYS_STATE);
    // the list bound for tracing
    CHECK(probe_list_check_trace(s, 24, &why) == RAYS_STATE && strstr(why, "no list"));
    CHECK(probe_list_bind(s, own, 4) == RAYS_INVALID_ARG && probe_list_bind(s, own, 0) == RAYS_INVALID_ARG && probe_list_bind(s, nullptr, 28) == RAYS_INVALID_ARG);
    CHECK(probe_list_bind(s, own, ((size_t)1 << 30) + 5) == RAYS_INVALID_ARG && s.list.count() == 0);
    CHECK(probe_list_capacity_ok(5) && probe_list_capacity_ok(((size_t)1 << 30) + 4) && !probe_list_capacity_ok(4) && !probe_list_capacity_ok(0));
    CHECK(probe_list_bind(s, own, 27) == RAYS_OK && probe_list_check_trace(s, 24, &why) == RAYS_STATE && strstr(why, "capacity"));
    CHECK(probe_list_bind(s, own, 28) == RAYS_OK && probe_list_check_trace(s, 24, nullptr) == RAYS_OK && probe_list_check_trace(s, 23, &why) == RAYS_STATE);
    input_written(s.list, 28);  // a write ends the binding
    CHECK(s.list.bound == nullptr && probe_list_check_trace(s, 24, &why) == RAYS_OK);
    CHECK(probe_list_bind(s, own, 11) == RAYS_OK && probe_list_bind(s, nullptr, 0) == RAYS_OK && s.list.count() == 28);  // unbound: back to the own array
    // the histories
    CHECK(probe_history_check_reset(0, 24, 8, &why) == RAYS_INVALID_ARG && probe_history_check_reset(4, 24, 8, &why) == RAYS_INVALID_ARG && strstr(why, "which"));
    CHECK(probe_history_check_reset(1, 0, 0, &why) == RAYS_INVALID_ARG && probe_history_check_reset(1, ((size_t)1 << 30) + 1, 0, &why) == RAYS_INVALID_ARG);
    CHECK(probe_history_check_reset(1, 24, 5, &why) == RAYS_OK);  // the resolution is ignored without the moments
    CHECK(probe_history_check_reset(3, 24, 5, &why) == RAYS_INVALID_ARG && strstr(why, "resolution"));
    CHECK(probe_history_check_reset(2, (size_t)1 << 23, 16, &why) == RAYS_INVALID_ARG && probe_history_check_reset(2, (size_t)1 << 22, 16, &why) == RAYS_OK);
    int slot = -1;
    CHECK(probe_history_check_read(s, 1, &slot, &bytes) == RAYS_STATE && probe_history_check_read(s, 3, &slot, &bytes) == RAYS_INVALID_ARG);
    // srt_blend_probes' checks, in the header's order
    LightProbeState lp;
    ProbeDepthState pd;
    ProbeStatesState cur;
    ProbeBlendCall b = bc;
    b.flags = 16;
    CHECK(probe_blend_check(s, lp, pd, cur, false, b, &why) == RAYS_STATE && strstr(why, "srt_set_scene"));
    CHECK(probe_blend_check(s, lp, pd, cur, true, b, &why) == RAYS_INVALID_ARG && strstr(why, "flags"));
    const float bad_h[] = {-0.1f, 1.0f, 1.5f, nan, inf, -inf};
    for (float v : bad_h) {
        b = bc, b.hysteresis = v;
        CHECK(probe_blend_check(s, lp, pd, cur, true, b, &why) == RAYS_INVALID_ARG && strstr(why, "hysteresis"));
        b = bc, b.fast_hysteresis = v;
        CHECK(probe_blend_check(s, lp, pd, cur, true, b, &why) == RAYS_INVALID_ARG && strstr(why, "fast_hysteresis"));
        b = bc, b.depth_hysteresis = v;
        CHECK(probe_blend_check(s, lp, pd, cur, true, b, &why) == RAYS_INVALID_ARG && strstr(why, "depth_hysteresis"));
    }
    const float bad_t[] = {-1.0f, nan, inf};
    for (float v : bad_t) {
        b = bc, b.change_threshold = v;
        CHECK(probe_blend_check(s, lp, pd, cur, true, b, &why) == RAYS_INVALID_ARG && strstr(why, "change_threshold"));
    }
    b = bc, b.reserved = 1;
    CHECK(probe_blend_check(s, lp, pd, cur, true, b, &why) == RAYS_INVALID_ARG && strstr(why, "reserved"));
    b = bc, b.hysteresis = 0.0f, b.fast_hysteresis = 0.0f, b.depth_hysteresis = 0.99999994f, b.change_threshold = 0.0f;
    CHECK(probe_blend_check(s, lp, pd, cur, true, b, &why) == RAYS_STATE && strstr(why, "no coefficient history"));  // arguments before the inputs
    probe_history_was_reset(s, 0, 24, 8);
    CHECK(probe_history_check_read(s, 1, &slot, &bytes) == RAYS_OK && slot == 0 && bytes == 24 * 9 * 16 && s.history[0].resolution == 0);
    CHECK(probe_blend_check(s, lp, pd, cur, true, bc, &why) == RAYS_STATE && strstr(why, "did not write COEFFICIENTS"));
    char co[16], ra[16], mo[16];
    void* ldst[LIGHT_PROBE_SLOTS] = {co, ra};
    light_probe_traced(lp, 24, 64, LIGHT_PROBE_OUT_RADIANCE, ldst, 0);
    CHECK(probe_blend_check(s, lp, pd, cur, true, bc, &why) == RAYS_STATE && strstr(why, "did not write COEFFICIENTS"));
    light_probe_traced(lp, 23, 64, LIGHT_PROBE_OUT_ALL, ldst, 0);
    CHECK(probe_blend_check(s, lp, pd, cur, true, bc, &why) == RAYS_STATE && strstr(why, "another probe count"));
    light_probe_traced(lp, 24, 64, LIGHT_PROBE_OUT_COEFFICIENTS, ldst, 0);
    CHECK(probe_blend_check(s, lp, pd, cur, true, bc, nullptr) == RAYS_OK);
    lp.last.released(0, co);  // the own output was re-allocated: its data are gone
    CHECK(probe_blend_check(s, lp, pd, cur, true, bc, &why) == RAYS_STATE);
    light_probe_traced(lp, 24, 64, LIGHT_PROBE_OUT_COEFFICIENTS, ldst, 0);
    // ... the moments
    b = bc, b.flags = PROBE_BLEND_FLAG_MOMENTS;
    CHECK(probe_blend_check(s, lp, pd, cur, true, b, &why) == RAYS_STATE && strstr(why, "no moment history"));
    probe_history_was_reset(s, 1, 23, 8);
    CHECK(probe_blend_check(s, lp, pd, cur, true, b, &why) == RAYS_STATE && strstr(why, "different probe counts"));
    probe_history_was_reset(s, 1, 24, 8);
    CHECK(probe_history_check_read(s, 2, &slot, &bytes) == RAYS_OK && slot == 1 && bytes == 24 * 64 * 16);
    CHECK(probe_blend_check(s, lp, pd, cur, true, b, &why) == RAYS_STATE && strstr(why, "did not write MOMENTS"));
    ProbeDepthCall dc;
    probe_depth_call_default(dc);
    void* ddst[PROBE_DEPTH_SLOTS] = {mo, nullptr};
    probe_depth_traced(pd, 24, 64, dc, ddst);  // R = 16
    CHECK(probe_blend_check(s, lp, pd, cur, true, b, &why) == RAYS_STATE && strstr(why, "resolution"));
    dc.resolution = 8;
    probe_depth_traced(pd, 24, 64, dc, ddst);
    CHECK(probe_blend_check(s, lp, pd, cur, true, b, &why) == RAYS_OK);
    // ... the list
    b.flags |= PROBE_BLEND_FLAG_LISTED;
    CHECK(probe_blend_check(s, lp, pd, cur, true, b, &why) == RAYS_OK);  // the own list of 28 words
    input_written(s.list, 27);
    CHECK(probe_blend_check(s, lp, pd, cur, true, b, &why) == RAYS_STATE && strstr(why, "capacity"));
    input_written(s.list, 28);
    // ... the records
    b.flags |= PROBE_BLEND_FLAG_PREVIOUS_STATES;
    CHECK(probe_blend_check(s, lp, pd, cur, true, b, &why) == RAYS_STATE && strstr(why, "no states"));
    input_written(cur.states, 23);
    CHECK(probe_blend_check(s, lp, pd, cur, true, b, &why) == RAYS_STATE && strstr(why, "state count"));
    input_written(cur.states, 24);
    CHECK(probe_blend_check(s, lp, pd, cur, true, b, &why) == RAYS_STATE && strstr(why, "no previous states"));
    CHECK(input_bind(s.previous, own, 25, PROBE_GRID_MAX_PROBES) == RAYS_OK);
    CHECK(probe_blend_check(s, lp, pd, cur, true, b, &why) == RAYS_STATE && strstr(why, "previous state count"));
    input_written(s.previous, 24);
    CHECK(probe_blend_check(s, lp, pd, cur, true, b, &why) == RAYS_OK);
    // the work record and a lost history
    CHECK(s.blend_call.work() == RAYS_STATE);
    probe_blend_blended(s, b.flags);
    CHECK(s.blend_call.work() == RAYS_STATE);
    probe_blend_blended(s, b.flags | PROBE_BLEND_FLAG_COUNT_WORK);
    CHECK(s.blend_call.work() == RAYS_OK);
    probe_history_lost(s, 0);
    CHECK(probe_history_check_read(s, 1, &slot, &bytes) == RAYS_STATE && probe_blend_check(s, lp, pd, cur, true, bc, &why) == RAYS_STATE);
    CHECK(probe_blend_grid(210, 4, 1024) == 53 && probe_blend_grid(8925, 4, 1024) == 1024 && probe_blend_grid(1, 4, 1024) == 1);
    printf("ok %d\n", checks);
    return 0;
}
