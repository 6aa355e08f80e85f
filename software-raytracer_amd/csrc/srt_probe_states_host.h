// srt_probe_states_host.h — host-side rules of probe classification and relocation (srt_classify_probes,
// srt_bind_probe_states_output, srt_read_probe_states_output, srt_get_probe_classify_work) and of the probe-grid shading that obeys
// the records (srt_write_probe_grid_states, srt_bind_probe_grid_states, srt_shade_probe_grid_states) that need no device: argument
// validation in the header's order, the primitive table the classify kernel reads (built from the object list, NOT from the scene
// image, which stores r*r), the sizes of the outputs, the record of what the last classification wrote and where, which state
// array is current.  Plain C++ without HIP, shared by srt_capi.hip and by tests/native/probe_states_check.cpp, which runs it under
// the address and undefined-behaviour sanitizers on the CPU.
#pragma once

#include <math.h>

#include <vector>

#include "srt_probe_depth_host.h"

namespace srt {

constexpr uint32_t PROBE_CLASSIFY_FLAG_RELOCATE = 1u, PROBE_CLASSIFY_FLAG_NORMALIZE = 2u, PROBE_CLASSIFY_FLAG_COUNT_WORK = 4u, PROBE_CLASSIFY_FLAG_ALL = 7u;
constexpr uint32_t PROBE_STATE_OUT_RECORDS = 1u, PROBE_STATE_OUT_POSITIONS = 2u, PROBE_STATE_OUT_ALL = 3u;
constexpr uint32_t PROBE_MOVED = 1u, PROBE_BURIED = 2u, PROBE_INSIDE = 4u, PROBE_IDLE = 8u;  // the bits of a record's w lane; 0: clear
constexpr int PROBE_STATE_SLOTS = 2;
constexpr uint32_t PROBE_CLASSIFY_MAX_STEPS = 64;
constexpr int PROBE_TABLE_OBJ_SPHERE = 1, PROBE_TABLE_OBJ_BOX = 2, PROBE_TABLE_OBJ_MESH = 3;  // srt_object_type's values

// the fields of srt_probe_classify_params, in its order
struct ProbeClassifyCall {
    float clearance, max_offset;
    uint32_t steps, flags, outputs, reserved;
};

inline void probe_classify_call_default(ProbeClassifyCall& c) {
    c.clearance = 0.2f, c.max_offset = 0.45f, c.steps = 8, c.flags = 0, c.outputs = PROBE_STATE_OUT_RECORDS, c.reserved = 0;
}

// The primitive table: the spheres of the list as one float4 each (centre, |radius|), then the boxes as two (centre, 0) and
// (half size, 0), both in list order.  Inert objects and meshes have no row; a mesh only sets has_mesh (rule S1: meshes contribute
// no distance, and rule S3: no probe of such a scene is IDLE).
struct ProbeTable {
    std::vector<float> rows;  // 4 floats per row
    uint32_t spheres = 0, boxes = 0;
    bool has_mesh = false;
    size_t vec4() const { return (size_t)spheres + 2 * (size_t)boxes; }
};

// Obj: srt_object or anything with its type, position, radius and half_size
template <class Obj>
inline void probe_table_build(const Obj* objects, size_t count, ProbeTable& t) {
    t.rows.clear(), t.spheres = 0, t.boxes = 0, t.has_mesh = false;
    for (size_t i = 0; i < count; ++i) {
        t.spheres += objects[i].type == PROBE_TABLE_OBJ_SPHERE, t.boxes += objects[i].type == PROBE_TABLE_OBJ_BOX;
        t.has_mesh = t.has_mesh || objects[i].type == PROBE_TABLE_OBJ_MESH;
    }
    t.rows.reserve(4 * t.vec4());
    for (size_t i = 0; i < count; ++i)
        if (objects[i].type == PROBE_TABLE_OBJ_SPHERE) {
            const float row[4] = {objects[i].position[0], objects[i].position[1], objects[i].position[2], fabsf(objects[i].radius)};
            t.rows.insert(t.rows.end(), row, row + 4);
        }
    for (size_t i = 0; i < count; ++i)
        if (objects[i].type == PROBE_TABLE_OBJ_BOX) {
            const float row[8] = {objects[i].position[0], objects[i].position[1], objects[i].position[2], 0.0f,
                                  objects[i].half_size[0], objects[i].half_size[1], objects[i].half_size[2], 0.0f};
            t.rows.insert(t.rows.end(), row, row + 8);
        }
}

// slot of a single output bit, -1 for anything else
inline int probe_state_slot(uint32_t output) { return output == PROBE_STATE_OUT_RECORDS ? 0 : output == PROBE_STATE_OUT_POSITIONS ? 1 : -1; }
// bytes of an output of a classification of P probes: P float4 either way
inline size_t probe_state_bytes(size_t probes) { return probes * (4 * sizeof(float)); }

struct ProbeStatesState {
    // the last successful srt_classify_probes
    CallRecord call;  // counted: it had SRT_PROBE_CLASSIFY_COUNT_WORK
    size_t last_probes = 0;
    LastOutputs<PROBE_STATE_SLOTS> last;
    // the records srt_shade_probe_grid_states reads, counted in probes
    InputArray states;
};

// srt_classify_probes' checks in the header's order (rule S9): the scene, the arguments, the inputs; touches nothing.
// `directions`: the current direction count of the light-probe block.
inline RaysStatus probe_classify_check(const ProbeGridState& g, size_t directions, bool scene_set, const ProbeClassifyCall& c, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!scene_set) return *why = "srt_set_scene has not been called", RAYS_STATE;
    if (c.flags & ~PROBE_CLASSIFY_FLAG_ALL) return *why = "unknown flags", RAYS_INVALID_ARG;
    if (c.outputs == 0 || (c.outputs & ~PROBE_STATE_OUT_ALL)) return *why = "outputs: want a non-empty set of SRT_PROBE_STATE_RECORDS | SRT_PROBE_STATE_POSITIONS", RAYS_INVALID_ARG;
    if (!(c.clearance > 0.0f) || !(c.clearance <= 0.5f)) return *why = "clearance must be in (0, 0.5]", RAYS_INVALID_ARG;  // (a NaN fails the comparisons)
    if (!(c.max_offset > 0.0f) || !(c.max_offset <= 0.5f)) return *why = "max_offset must be in (0, 0.5]", RAYS_INVALID_ARG;
    if (c.steps < 1 || c.steps > PROBE_CLASSIFY_MAX_STEPS) return *why = "steps outside 1 .. 64", RAYS_INVALID_ARG;
    if (c.reserved != 0) return *why = "reserved must be 0", RAYS_INVALID_ARG;
    if (!g.grid_set) return *why = "no grid (srt_set_probe_grid)", RAYS_STATE;
    if ((c.flags & PROBE_CLASSIFY_FLAG_RELOCATE) && directions == 0)
        return *why = "no directions have been written or bound (srt_write_light_probe_directions, srt_bind_light_probe_directions)", RAYS_STATE;
    return RAYS_OK;
}

// srt_classify_probes once the launch is enqueued: dst[slot] is where each requested output went.
inline void probe_states_classified(ProbeStatesState& s, size_t probes, const ProbeClassifyCall& c, void* const dst[PROBE_STATE_SLOTS]) {
    s.call.done((c.flags & PROBE_CLASSIFY_FLAG_COUNT_WORK) != 0);
    s.last_probes = probes;
    s.last.wrote(c.outputs, dst);
}

// The grid: one wave per probe, persistent workgroups of `waves` waves, at most `resident`.
inline unsigned probe_classify_grid(size_t probes, int waves, long long resident) { return persistent_grid((long long)probes, waves, resident); }

// srt_shade_probe_grid_states' checks: the parent call's (srt_shade_probe_grid's with SRT_PROBE_GRID_VISIBILITY refused, or
// srt_shade_probe_grid_depth's when `dc` is given), then the records; touches nothing.
inline RaysStatus probe_grid_states_check_shade(const ProbeGridState& s, const ProbeGridDepthState& d, const ProbeStatesState& st, const ProbeGridCall& c,
                                                const ProbeGridDepthCall* dc, bool scene_set, int height, const bool guide_present[PROBE_GRID_GUIDES],
                                                const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (dc) {
        if (const RaysStatus rs = probe_grid_depth_check_shade(s, d, c, *dc, scene_set, height, guide_present, why)) return rs;
    } else {
        if (!scene_set) return *why = "srt_set_scene has not been called", RAYS_STATE;
        if (c.row_begin < 0 || c.row_end > height || c.row_begin >= c.row_end) return *why = "bad row band", RAYS_INVALID_ARG;
        if (c.flags & PROBE_GRID_FLAG_VISIBILITY)
            return *why = "SRT_PROBE_GRID_VISIBILITY: the exact test towards relocated probes is not available", RAYS_INVALID_ARG;
        if (const RaysStatus rs = probe_grid_check_shade(s, c, scene_set, height, guide_present, why)) return rs;
    }
    if (st.states.count() == 0) return *why = "no states have been written or bound (srt_write_probe_grid_states, srt_bind_probe_grid_states)", RAYS_STATE;
    if (st.states.count() != probe_grid_probes(s.grid)) return *why = "the state count is not nx * ny * nz", RAYS_STATE;
    return RAYS_OK;
}

}  // namespace srt
