// srt_probe_update_host.h — host-side rules of the per-frame probe updates (srt_list_probes, srt_bind_probe_list_output,
// srt_read_probe_list_output, srt_get_probe_list_work; srt_bind_probe_list, srt_write_probe_list and the two listed traces;
// srt_reset_probe_history, srt_bind_probe_history, srt_read_probe_history, srt_write_probe_previous_states,
// srt_bind_probe_previous_states, srt_blend_probes, srt_get_probe_blend_work) that need no device: argument validation in the
// header's order, the sizes of the list and of the histories, the record of what the last listing wrote and where, which list is
// bound for tracing, which P and R the histories stand for, and what the blend takes as its new data.  Plain C++ without HIP,
// shared by srt_capi.hip and by tests/native/probe_update_check.cpp, which runs it under the address and undefined-behaviour
// sanitizers on the CPU.
#pragma once

#include <math.h>

#include "srt_probe_states_host.h"

namespace srt {

constexpr uint32_t PROBE_LIST_FLAG_COUNT_WORK = 1u, PROBE_LIST_FLAG_ALL = 1u;
constexpr uint32_t PROBE_STATE_BITS = PROBE_MOVED | PROBE_BURIED | PROBE_INSIDE | PROBE_IDLE;  // (CLEAR is the absence of all four)
constexpr size_t PROBE_LIST_HEADER = 4;  // words in front of the indices: n, P, 0, 0
constexpr uint32_t PROBE_LIST_NONE = 0xFFFFFFFFu;
constexpr size_t PROBE_LIST_MAX_PROBES = (size_t)1 << 30;
constexpr uint32_t PROBE_BLEND_FLAG_MOMENTS = 1u, PROBE_BLEND_FLAG_LISTED = 2u, PROBE_BLEND_FLAG_PREVIOUS_STATES = 4u, PROBE_BLEND_FLAG_COUNT_WORK = 8u,
                   PROBE_BLEND_FLAG_ALL = 15u;
constexpr uint32_t PROBE_HISTORY_COEFFICIENTS = 1u, PROBE_HISTORY_MOMENTS = 2u, PROBE_HISTORY_ALL = 3u;
constexpr int PROBE_HISTORY_SLOTS = 2;

// the fields of srt_probe_list_params, in its order
struct ProbeListCall {
    uint32_t skip_mask, flags, reserved[2];
};
// the fields of srt_probe_blend_params, in its order
struct ProbeBlendCall {
    float hysteresis, fast_hysteresis, depth_hysteresis, change_threshold;
    uint32_t flags, reserved;
};

inline void probe_list_call_default(ProbeListCall& c) { c.skip_mask = PROBE_BURIED | PROBE_IDLE, c.flags = 0, c.reserved[0] = 0, c.reserved[1] = 0; }
// (picks, not measurements: DDGI's customary values)
inline void probe_blend_call_default(ProbeBlendCall& c) {
    c.hysteresis = 0.9f, c.fast_hysteresis = 0.5f, c.depth_hysteresis = 0.9f, c.change_threshold = 0.25f, c.flags = 0, c.reserved = 0;
}

// words and bytes of a list over P probes: the header, then one word per probe
inline size_t probe_list_words(size_t probes) { return PROBE_LIST_HEADER + probes; }
inline size_t probe_list_bytes(size_t probes) { return probe_list_words(probes) * sizeof(uint32_t); }
// slot of a single history bit, -1 for anything else
inline int probe_history_slot(uint32_t which) { return which == PROBE_HISTORY_COEFFICIENTS ? 0 : which == PROBE_HISTORY_MOMENTS ? 1 : -1; }
// bytes of a history of P probes (and resolution R): [P][9] float4, [P][R*R] float4
inline size_t probe_history_bytes(int slot, size_t probes, uint32_t resolution) {
    return probes * (slot == 0 ? (size_t)LIGHT_PROBE_COEFFS : (size_t)resolution * resolution) * (4 * sizeof(float));
}

struct ProbeHistory {
    const void* bound = nullptr;  // the caller's buffer (srt_bind_probe_history); NULL: the handle's own
    bool reset = false;           // srt_reset_probe_history has given it a size
    size_t probes = 0;
    uint32_t resolution = 0;      // (the moments only)
};

struct ProbeUpdateState {
    // the last successful srt_list_probes
    CallRecord list_call;  // counted: it had SRT_PROBE_LIST_COUNT_WORK
    size_t list_probes = 0;
    LastOutputs<1> list_last;              // (one output: bit 1, slot 0)
    const void* list_out_bound = nullptr;  // srt_bind_probe_list_output; NULL: the handle's own buffer
    // the list the listed traces and a listed blend read, counted in words
    InputArray list;
    // the records a blend with PREVIOUS_STATES compares the current ones with, counted in probes
    InputArray previous;
    ProbeHistory history[PROBE_HISTORY_SLOTS];
    // the last successful srt_blend_probes
    CallRecord blend_call;  // counted: it had SRT_PROBE_BLEND_COUNT_WORK
};

// srt_list_probes' checks in the header's order: the scene, the arguments, the inputs; touches nothing.
inline RaysStatus probe_list_check(const ProbeGridState& g, const ProbeStatesState& st, bool scene_set, const ProbeListCall& c, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!scene_set) return *why = "srt_set_scene has not been called", RAYS_STATE;
    if (c.flags & ~PROBE_LIST_FLAG_ALL) return *why = "unknown flags", RAYS_INVALID_ARG;
    if (c.skip_mask & ~PROBE_STATE_BITS) return *why = "skip_mask: want a subset of the SRT_PROBE_* state bits", RAYS_INVALID_ARG;
    if (c.reserved[0] != 0 || c.reserved[1] != 0) return *why = "reserved must be 0", RAYS_INVALID_ARG;
    const size_t P = st.states.count();
    if (P == 0) return *why = "no states have been written or bound (srt_write_probe_grid_states, srt_bind_probe_grid_states)", RAYS_STATE;
    if (P > PROBE_LIST_MAX_PROBES) return *why = "more than 2^30 states", RAYS_INVALID_ARG;
    if (g.grid_set && P != probe_grid_probes(g.grid)) return *why = "the state count is not nx * ny * nz", RAYS_STATE;
    return RAYS_OK;
}

// srt_list_probes once the launch is enqueued
inline void probe_list_listed(ProbeUpdateState& s, size_t probes, uint32_t flags, const void* dst) {
    s.list_call.done((flags & PROBE_LIST_FLAG_COUNT_WORK) != 0), s.list_probes = probes, s.list_last.wrote(1u, &dst);
}

// srt_write_probe_list, srt_bind_probe_list: is `capacity` words a list?  4 + P, P in 1 .. 2^30.
inline bool probe_list_capacity_ok(size_t capacity) { return capacity > PROBE_LIST_HEADER && capacity - PROBE_LIST_HEADER <= PROBE_LIST_MAX_PROBES; }
// srt_bind_probe_list: NULL, 0 unbinds; otherwise a device array and its capacity.  On an error the state is left as it was.
inline RaysStatus probe_list_bind(ProbeUpdateState& s, const void* d_list, size_t capacity) {
    if (d_list && !probe_list_capacity_ok(capacity)) return RAYS_INVALID_ARG;
    return input_bind(s.list, d_list, capacity, PROBE_LIST_HEADER + PROBE_LIST_MAX_PROBES);
}

// The listed traces, after all of the parent call's checks: a list of 4 + P words for the current positions' P.
inline RaysStatus probe_list_check_trace(const ProbeUpdateState& s, size_t probes, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (s.list.count() == 0) return *why = "no list has been written or bound (srt_write_probe_list, srt_bind_probe_list)", RAYS_STATE;
    if (s.list.count() != probe_list_words(probes)) return *why = "the list's capacity is not 4 + the probe count", RAYS_STATE;
    return RAYS_OK;
}

// srt_reset_probe_history's arguments: a non-empty set of history bits, P in 1 .. 2^30, and with the moments R in {4, 8, 16}
// and P*R*R <= 2^30.
inline RaysStatus probe_history_check_reset(uint32_t which, size_t probes, uint32_t resolution, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (which == 0 || (which & ~PROBE_HISTORY_ALL)) return *why = "which: want a non-empty set of SRT_PROBE_HISTORY_COEFFICIENTS | SRT_PROBE_HISTORY_MOMENTS", RAYS_INVALID_ARG;
    if (probes < 1 || probes > PROBE_LIST_MAX_PROBES) return *why = "probes outside 1 .. 2^30", RAYS_INVALID_ARG;
    if ((which & PROBE_HISTORY_MOMENTS) && probe_grid_depth_check_input(probes, resolution) != RAYS_OK)
        return *why = "resolution must be 4, 8 or 16, and probes x resolution^2 at most 2^30", RAYS_INVALID_ARG;
    return RAYS_OK;
}
inline void probe_history_was_reset(ProbeUpdateState& s, int slot, size_t probes, uint32_t resolution) {
    s.history[slot].reset = true, s.history[slot].probes = probes, s.history[slot].resolution = slot == 1 ? resolution : 0;
}
// a failed re-allocation of the own history leaves none
inline void probe_history_lost(ProbeUpdateState& s, int slot) { s.history[slot].reset = false, s.history[slot].probes = 0, s.history[slot].resolution = 0; }

// srt_blend_probes' checks in the header's order: the scene, the arguments, the inputs; touches nothing.  `lp`, `pd`: the
// records of the last light-probe trace and the last depth trace; `st`: the current state records.
inline RaysStatus probe_blend_check(const ProbeUpdateState& s, const LightProbeState& lp, const ProbeDepthState& pd, const ProbeStatesState& st, bool scene_set,
                                    const ProbeBlendCall& c, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!scene_set) return *why = "srt_set_scene has not been called", RAYS_STATE;
    if (c.flags & ~PROBE_BLEND_FLAG_ALL) return *why = "unknown flags", RAYS_INVALID_ARG;
    if (!(c.hysteresis >= 0.0f) || !(c.hysteresis < 1.0f)) return *why = "hysteresis must be in [0, 1)", RAYS_INVALID_ARG;  // (a NaN fails the comparisons)
    if (!(c.fast_hysteresis >= 0.0f) || !(c.fast_hysteresis < 1.0f)) return *why = "fast_hysteresis must be in [0, 1)", RAYS_INVALID_ARG;
    if (!(c.depth_hysteresis >= 0.0f) || !(c.depth_hysteresis < 1.0f)) return *why = "depth_hysteresis must be in [0, 1)", RAYS_INVALID_ARG;
    if (!(c.change_threshold >= 0.0f) || !isfinite(c.change_threshold)) return *why = "change_threshold must be finite and >= 0", RAYS_INVALID_ARG;
    if (c.reserved != 0) return *why = "reserved must be 0", RAYS_INVALID_ARG;
    const ProbeHistory& hc = s.history[0];
    if (!hc.reset) return *why = "no coefficient history (srt_reset_probe_history)", RAYS_STATE;
    const size_t P = hc.probes;
    if (!lp.last.read(LIGHT_PROBE_OUT_COEFFICIENTS, 0))
        return *why = "the last srt_trace_light_probes did not write COEFFICIENTS", RAYS_STATE;
    if (lp.last_probes != P) return *why = "the last srt_trace_light_probes wrote COEFFICIENTS for another probe count than the history's", RAYS_STATE;
    if (c.flags & PROBE_BLEND_FLAG_MOMENTS) {
        const ProbeHistory& hm = s.history[1];
        if (!hm.reset) return *why = "no moment history (srt_reset_probe_history)", RAYS_STATE;
        if (hm.probes != P) return *why = "the two histories stand for different probe counts", RAYS_STATE;
        if (!pd.last.read(PROBE_DEPTH_OUT_MOMENTS, 0)) return *why = "the last srt_trace_probe_depth did not write MOMENTS", RAYS_STATE;
        if (pd.last_probes != P || pd.last_resolution != hm.resolution)
            return *why = "the last srt_trace_probe_depth wrote MOMENTS for another probe count or resolution than the history's", RAYS_STATE;
    }
    if (c.flags & PROBE_BLEND_FLAG_LISTED)
        if (const RaysStatus rs = probe_list_check_trace(s, P, why)) return rs;
    if (c.flags & PROBE_BLEND_FLAG_PREVIOUS_STATES) {
        if (st.states.count() == 0) return *why = "no states have been written or bound (srt_write_probe_grid_states, srt_bind_probe_grid_states)", RAYS_STATE;
        if (st.states.count() != P) return *why = "the state count is not the history's probe count", RAYS_STATE;
        if (s.previous.count() == 0) return *why = "no previous states have been written or bound (srt_write_probe_previous_states, srt_bind_probe_previous_states)", RAYS_STATE;
        if (s.previous.count() != P) return *why = "the previous state count is not the history's probe count", RAYS_STATE;
    }
    return RAYS_OK;
}
inline void probe_blend_blended(ProbeUpdateState& s, uint32_t flags) { s.blend_call.done((flags & PROBE_BLEND_FLAG_COUNT_WORK) != 0); }

// srt_read_probe_history: only a history that has a size
inline RaysStatus probe_history_check_read(const ProbeUpdateState& s, uint32_t which, int* slot, size_t* bytes) {
    const int i = probe_history_slot(which);
    if (i < 0) return RAYS_INVALID_ARG;
    if (!s.history[i].reset) return RAYS_STATE;
    *slot = i, *bytes = probe_history_bytes(i, s.history[i].probes, s.history[i].resolution);
    return RAYS_OK;
}

// The blend's grid: one wave per probe, persistent workgroups of `waves` waves, at most `resident`.
inline unsigned probe_blend_grid(size_t probes, int waves, long long resident) { return persistent_grid((long long)probes, waves, resident); }

}  // namespace srt
