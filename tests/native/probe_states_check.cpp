// probe_states_check.cpp — the host-side rules of probe classification and of the shading that obeys the records
// (software-raytracer_amd/csrc/srt_probe_states_host.h) as a stand-alone program, built with -fsanitize=address,undefined by
// tests/test_probe_states_native.py: the defaults, which parameters are accepted and in which order the checks come, the primitive
// table (exactly one float4 per sphere and two per box, |radius|, meshes and inert objects without a row), the slots and sizes of
// the outputs, what a read returns, the state input and the order of the shading call's checks.  Prints "ok <checks>" or the first
// failure.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "srt_probe_states_host.h"

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

struct Obj {  // the fields of srt_object the table reads
    int32_t type;
    float position[3];
    float radius;
    float half_size[3];
};

// srt_read_probe_states_output's rule as srt_capi.hip composes it: the slot, the shared record's read, the byte count of the last call
static RaysStatus read_probe_states_output(const ProbeStatesState& s, uint32_t output, const void** src, size_t* bytes) {
    const int i = probe_state_slot(output);
    if (i < 0) return RAYS_INVALID_ARG;
    if (!(*src = s.last.read(output, i))) return RAYS_STATE;
    *bytes = probe_state_bytes(s.last_probes);
    return RAYS_OK;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    static_assert(sizeof(ProbeClassifyCall) == 24, "the struct of the header");
    const char* why = nullptr;
    // defaults
    ProbeClassifyCall c;
    probe_classify_call_default(c);
    CHECK(c.clearance == 0.2f && c.max_offset == 0.45f && c.steps == 8 && c.flags == 0 && c.outputs == PROBE_STATE_OUT_RECORDS && c.reserved == 0);
    CHECK(PROBE_MOVED == 1 && PROBE_BURIED == 2 && PROBE_INSIDE == 4 && PROBE_IDLE == 8);
    // the classification's checks, in the header's order
    ProbeGridState g;
    ProbeClassifyCall bad = c;
    bad.flags = 8;
    CHECK(probe_classify_check(g, 0, false, bad, &why) == RAYS_STATE && strstr(why, "srt_set_scene"));  // the scene first
    CHECK(probe_classify_check(g, 0, true, bad, &why) == RAYS_INVALID_ARG && strstr(why, "flags"));     // arguments before the grid
    bad = c, bad.outputs = 0;
    CHECK(probe_classify_check(g, 0, true, bad, &why) == RAYS_INVALID_ARG && strstr(why, "outputs"));
    bad.outputs = 4;
    CHECK(probe_classify_check(g, 0, true, bad, &why) == RAYS_INVALID_ARG && strstr(why, "outputs"));
    const float bad_fraction[] = {0.0f, -0.1f, 0.5000001f, 1.0f, nan, inf, -inf};
    for (float v : bad_fraction) {
        bad = c, bad.clearance = v;
        CHECK(probe_classify_check(g, 0, true, bad, &why) == RAYS_INVALID_ARG && strstr(why, "clearance"));
        bad = c, bad.max_offset = v;
        CHECK(probe_classify_check(g, 0, true, bad, &why) == RAYS_INVALID_ARG && strstr(why, "max_offset"));
    }
    const uint32_t bad_steps[] = {0, 65, 0xFFFFFFFFu};
    for (uint32_t s : bad_steps) {
        bad = c, bad.steps = s;
        CHECK(probe_classify_check(g, 0, true, bad, &why) == RAYS_INVALID_ARG && strstr(why, "steps"));
    }
    bad = c, bad.reserved = 1;
    CHECK(probe_classify_check(g, 0, true, bad, &why) == RAYS_INVALID_ARG && strstr(why, "reserved"));
    bad = c, bad.clearance = 0.5f, bad.max_offset = 0.5f, bad.steps = 64, bad.flags = PROBE_CLASSIFY_FLAG_RELOCATE, bad.outputs = PROBE_STATE_OUT_ALL;
    CHECK(probe_classify_check(g, 0, true, bad, &why) == RAYS_STATE && strstr(why, "no grid"));  // the grid before the directions
    g.grid_set = true;
    g.grid.counts[0] = 3, g.grid.counts[1] = 2, g.grid.counts[2] = 4;
    CHECK(probe_classify_check(g, 0, true, bad, &why) == RAYS_STATE && strstr(why, "directions"));
    CHECK(probe_classify_check(g, 1, true, bad, nullptr) == RAYS_OK);
    CHECK(probe_classify_check(g, 0, true, c, &why) == RAYS_OK);  // without relocation no directions are needed
    bad = c, bad.clearance = 1e-30f, bad.max_offset = 1e-30f, bad.steps = 1;
    CHECK(probe_classify_check(g, 0, true, bad, &why) == RAYS_OK);
    // the primitive table
    const Obj objs[] = {{PROBE_TABLE_OBJ_BOX, {1, 2, 3}, 9.0f, {4, 5, 6}},     {0, {7, 7, 7}, 7.0f, {7, 7, 7}},
                        {PROBE_TABLE_OBJ_SPHERE, {-1, -2, -3}, -2.5f, {8, 8, 8}}, {PROBE_TABLE_OBJ_MESH, {0, 0, 0}, 1.0f, {1, 1, 1}},
                        {PROBE_TABLE_OBJ_SPHERE, {10, 11, 12}, nan, {0, 0, 0}},  {PROBE_TABLE_OBJ_BOX, {-4, -5, -6}, 0.0f, {0.5f, inf, 0.0f}}};
    ProbeTable t;
    probe_table_build(objs, 6, t);
    CHECK(t.spheres == 2 && t.boxes == 2 && t.has_mesh && t.vec4() == 6 && t.rows.size() == 24);
    const float want[] = {-1, -2, -3, 2.5f, 10, 11, 12, 0 /* NaN, checked below */, 1, 2, 3, 0, 4, 5, 6, 0, -4, -5, -6, 0, 0.5f, inf, 0.0f, 0};
    for (size_t i = 0; i < 24; ++i) CHECK(i == 7 ? t.rows[i] != t.rows[i] : t.rows[i] == want[i]);
    probe_table_build(objs, 3, t);  // a rebuild replaces the table
    CHECK(t.spheres == 1 && t.boxes == 1 && !t.has_mesh && t.rows.size() == 12 && t.rows[3] == 2.5f);
    probe_table_build((const Obj*)nullptr, 0, t);
    CHECK(t.spheres == 0 && t.boxes == 0 && !t.has_mesh && t.rows.empty() && t.vec4() == 0);
    // slots and sizes
    CHECK(probe_state_slot(1) == 0 && probe_state_slot(2) == 1 && probe_state_slot(0) == -1 && probe_state_slot(3) == -1 && probe_state_slot(4) == -1);
    CHECK(probe_state_bytes(24) == 24 * 16 && probe_state_bytes((size_t)1 << 30) == (size_t)1 << 34);
    // what a read returns
    ProbeStatesState s;
    const void* src = nullptr;
    size_t bytes = 0;
    CHECK(read_probe_states_output(s, 1, &src, &bytes) == RAYS_STATE && read_probe_states_output(s, 3, &src, &bytes) == RAYS_INVALID_ARG);
    CHECK(s.call.work() == RAYS_STATE);
    char own0[16], own1[16];
    void* dst[PROBE_STATE_SLOTS] = {own0, own1};
    probe_states_classified(s, 24, c, dst);  // RECORDS only, not counting
    CHECK(read_probe_states_output(s, 1, &src, &bytes) == RAYS_OK && src == own0 && bytes == 24 * 16);
    CHECK(read_probe_states_output(s, 2, &src, &bytes) == RAYS_STATE && s.call.work() == RAYS_STATE);
    ProbeClassifyCall both = c;
    both.outputs = PROBE_STATE_OUT_ALL, both.flags = PROBE_CLASSIFY_FLAG_COUNT_WORK;
    probe_states_classified(s, 7, both, dst);
    CHECK(read_probe_states_output(s, 2, &src, &bytes) == RAYS_OK && src == own1 && bytes == 7 * 16 && s.call.work() == RAYS_OK);
    s.last.released(1, own0);  // another buffer: nothing happens
    CHECK(read_probe_states_output(s, 2, &src, &bytes) == RAYS_OK);
    s.last.released(1, own1);
    CHECK(read_probe_states_output(s, 2, &src, &bytes) == RAYS_STATE && read_probe_states_output(s, 1, &src, &bytes) == RAYS_OK);
    CHECK(probe_classify_grid(729, 4, 1000) == 183 && probe_classify_grid(100000, 4, 1024) == 1024 && probe_classify_grid(1, 4, 1024) == 1);
    // the shading call's checks: the parent's first, then the records
    ProbeGridState pg;
    ProbeGridDepthState pd;
    ProbeStatesState st;
    ProbeGridCall call;
    probe_grid_call_default(call);
    call.row_begin = 0, call.row_end = 20;
    ProbeGridDepthCall dc;
    probe_grid_depth_call_default(dc);
    bool present[PROBE_GRID_GUIDES] = {true, true, true, false};
    CHECK(probe_grid_states_check_shade(pg, pd, st, call, nullptr, false, 20, present, &why) == RAYS_STATE && strstr(why, "srt_set_scene"));
    ProbeGridCall vis = call;
    vis.flags = PROBE_GRID_FLAG_VISIBILITY | PROBE_GRID_FLAG_ALBEDO;
    CHECK(probe_grid_states_check_shade(pg, pd, st, vis, nullptr, true, 20, present, &why) == RAYS_INVALID_ARG && strstr(why, "SRT_PROBE_GRID_VISIBILITY"));
    CHECK(probe_grid_states_check_shade(pg, pd, st, vis, &dc, true, 20, present, &why) == RAYS_INVALID_ARG && strstr(why, "SRT_PROBE_GRID_VISIBILITY"));
    vis = call, vis.row_end = 21;
    CHECK(probe_grid_states_check_shade(pg, pd, st, vis, nullptr, true, 20, present, &why) == RAYS_INVALID_ARG && strstr(why, "band"));
    CHECK(probe_grid_states_check_shade(pg, pd, st, call, nullptr, true, 20, present, &why) == RAYS_STATE && strstr(why, "no grid"));
    pg.grid_set = true;
    pg.grid.counts[0] = 3, pg.grid.counts[1] = 2, pg.grid.counts[2] = 4;
    for (int a = 0; a < 3; ++a) pg.grid.spacing[a] = 1.0f;
    CHECK(probe_grid_states_check_shade(pg, pd, st, call, nullptr, true, 20, present, &why) == RAYS_STATE && strstr(why, "no coefficients"));
    input_written(pg.coefficients, 24);
    CHECK(probe_grid_states_check_shade(pg, pd, st, call, nullptr, true, 20, present, &why) == RAYS_STATE && strstr(why, "no states"));
    CHECK(probe_grid_states_check_shade(pg, pd, st, call, &dc, true, 20, present, &why) == RAYS_STATE && strstr(why, "no depth maps"));  // the parent's come first
    probe_grid_depth_written(pd, 24, 8);
    ProbeGridDepthCall bad_dc = dc;
    bad_dc.bias = -1.0f;
    CHECK(probe_grid_states_check_shade(pg, pd, st, call, &bad_dc, true, 20, present, &why) == RAYS_INVALID_ARG && strstr(why, "bias"));
    CHECK(probe_grid_states_check_shade(pg, pd, st, call, &dc, true, 20, present, &why) == RAYS_STATE && strstr(why, "no states"));
    // the state input: written, bound, unbound
    char dev[16];
    CHECK(input_bind(st.states, dev, 23, PROBE_GRID_MAX_PROBES) == RAYS_OK);
    CHECK(probe_grid_states_check_shade(pg, pd, st, call, nullptr, true, 20, present, &why) == RAYS_STATE && strstr(why, "state count"));
    input_written(st.states, 24);  // a write ends the binding
    CHECK(st.states.bound == nullptr && probe_grid_states_check_shade(pg, pd, st, call, nullptr, true, 20, present, &why) == RAYS_OK);
    CHECK(probe_grid_states_check_shade(pg, pd, st, call, &dc, true, 20, present, &why) == RAYS_OK);
    CHECK(input_bind(st.states, nullptr, 5, PROBE_GRID_MAX_PROBES) == RAYS_INVALID_ARG && input_bind(st.states, dev, 0, PROBE_GRID_MAX_PROBES) == RAYS_INVALID_ARG);
    CHECK(input_bind(st.states, dev, PROBE_GRID_MAX_PROBES + 1, PROBE_GRID_MAX_PROBES) == RAYS_INVALID_ARG && st.states.count() == 24);
    vis = call, vis.flags = PROBE_GRID_FLAG_ALBEDO;
    CHECK(probe_grid_states_check_shade(pg, pd, st, vis, nullptr, true, 20, present, &why) == RAYS_STATE && strstr(why, "ALBEDO"));
    printf("ok %d\n", checks);
    return 0;
}
