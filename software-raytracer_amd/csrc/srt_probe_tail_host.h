// srt_probe_tail_host.h — host-side rules of the probe tail (srt_probe_tail, srt_probe_tail_params_default,
// srt_get_probe_tail_work; the mode of srt_trace_radiance and the two light-probe traces that ends a path at the bounce limit in
// the probe grid) that need no device: parameter validation in the header's order, the context's setting, what an affected trace
// requires of the grid's inputs, the byte-range overlap that makes a feedback loop read the buffer it writes, and when the work
// record may be read.  Plain C++ without HIP, shared by srt_capi.hip and by tests/native/probe_tail_check.cpp, which runs it
// under the address and undefined-behaviour sanitizers on the CPU.
#pragma once

#include <math.h>

#include "srt_probe_states_host.h"

namespace srt {

constexpr uint32_t PROBE_TAIL_FLAG_NORMAL_WEIGHT = 1u, PROBE_TAIL_FLAG_DEPTH = 2u, PROBE_TAIL_FLAG_STATES = 4u, PROBE_TAIL_FLAG_COUNT_WORK = 8u,
                   PROBE_TAIL_FLAG_ALL = 15u;

// the fields of srt_probe_tail_params, in its order
struct ProbeTailCall {
    int32_t enabled;
    uint32_t flags;
    float band_weight[3];
    float bias, min_variance;
    uint32_t reserved;
};

// the context's setting (off until the first accepted srt_probe_tail) and what the last affected trace did
struct ProbeTailState {
    bool enabled = false;
    ProbeTailCall call{0, 0u, {1.0f, 0.5f, 0.0f}, 0.0f, 1e-4f, 0u};
    CallRecord last;  // ran: the last affected trace ran with the mode ON; counted: ... and with SRT_PROBE_TAIL_COUNT_WORK
};

// the defaults of srt_probe_tail_params_default: on, no flags, the hemisphere mean of probe-grid rule 10, rule 7b's defaults
inline ProbeTailCall probe_tail_defaults() { return ProbeTailCall{1, 0u, {1.0f, 0.5f, 0.0f}, 0.0f, 1e-4f, 0u}; }

// srt_probe_tail's checks; touches nothing.  (The comparisons are written so that a NaN fails.)
inline RaysStatus probe_tail_check(const ProbeTailCall& c, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (c.enabled < 0 || c.enabled > 1) return *why = "enabled must be 0 or 1", RAYS_INVALID_ARG;
    if (c.flags & ~PROBE_TAIL_FLAG_ALL) return *why = "unknown flags", RAYS_INVALID_ARG;
    for (int b = 0; b < 3; ++b)
        if (c.band_weight[b] != c.band_weight[b]) return *why = "band_weight is NaN", RAYS_INVALID_ARG;
    if (!(c.bias >= 0.0f) || !isfinite(c.bias)) return *why = "bias must be finite and >= 0", RAYS_INVALID_ARG;
    if (!(c.min_variance > 0.0f) || !isfinite(c.min_variance)) return *why = "min_variance must be finite and > 0", RAYS_INVALID_ARG;
    if (c.reserved != 0) return *why = "reserved must be 0", RAYS_INVALID_ARG;
    return RAYS_OK;
}

// An accepted call takes effect.
inline void probe_tail_set(ProbeTailState& s, const ProbeTailCall& c) { s.enabled = c.enabled != 0, s.call = c; }

// do the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte?  An empty or absent range shares none.
inline bool probe_tail_ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    if (!a || !b || a_bytes == 0 || b_bytes == 0) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    // (written without a0 + a_bytes, which may wrap: a0 < b0 + b_bytes && b0 < a0 + a_bytes)
    return a0 >= b0 ? a0 - b0 < b_bytes : b0 - a0 < a_bytes;
}

// Does the mode change this trace?  Off, or max_bounces == 0 (rule T1): the call launches what it launched before.
inline bool probe_tail_applies(const ProbeTailState& s, int32_t max_bounces) { return s.enabled && max_bounces >= 1; }

// What an affected trace requires, checked after its own errors and before anything is touched: the grid and its inputs as
// srt_shade_probe_grid[_depth|_states] would read them now, and a coefficient array that is not the buffer about to be written
// (`written`: RADIANCE, or the light-probe COEFFICIENTS output; NULL when it is not allocated yet — a buffer this call allocates
// cannot be the bound coefficient array).
inline RaysStatus probe_tail_check_trace(const ProbeTailState& s, const ProbeGridState& g, const ProbeGridDepthState& d, const ProbeStatesState& st,
                                         const void* coefficients, const void* written, size_t written_bytes, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!g.grid_set) return *why = "srt_probe_tail is on and there is no grid (srt_set_probe_grid)", RAYS_STATE;
    if (g.coefficients.count() == 0)
        return *why = "srt_probe_tail is on and no coefficients have been written or bound (srt_write_probe_grid_coefficients, srt_bind_probe_grid_coefficients)", RAYS_STATE;
    const size_t probes = probe_grid_probes(g.grid);
    if (g.coefficients.count() != probes) return *why = "srt_probe_tail is on and the coefficient count is not nx * ny * nz", RAYS_STATE;
    if (s.call.flags & PROBE_TAIL_FLAG_DEPTH) {
        if (d.moments.count() == 0)
            return *why = "SRT_PROBE_TAIL_DEPTH and no depth maps have been written or bound (srt_write_probe_grid_depth, srt_bind_probe_grid_depth)", RAYS_STATE;
        if (d.moments.count() != probes) return *why = "SRT_PROBE_TAIL_DEPTH and the depth probe count is not nx * ny * nz", RAYS_STATE;
    }
    if (s.call.flags & PROBE_TAIL_FLAG_STATES) {
        if (st.states.count() == 0)
            return *why = "SRT_PROBE_TAIL_STATES and no states have been written or bound (srt_write_probe_grid_states, srt_bind_probe_grid_states)", RAYS_STATE;
        if (st.states.count() != probes) return *why = "SRT_PROBE_TAIL_STATES and the state count is not nx * ny * nz", RAYS_STATE;
    }
    if (probe_tail_ranges_overlap(coefficients, probes * (size_t)LIGHT_PROBE_COEFFS * (4 * sizeof(float)), written, written_bytes))
        return *why = "srt_probe_tail would read the coefficient array this call writes: read the history or the previous frame's buffer", RAYS_STATE;
    return RAYS_OK;
}

// an affected trace once its launch is enqueued.  True when the mode is on and counts: the record is this trace's (all zeros when
// max_bounces == 0 kept the mode from applying: the caller zeroes it).
inline bool probe_tail_traced(ProbeTailState& s) {
    s.last = CallRecord{s.enabled, s.enabled && (s.call.flags & PROBE_TAIL_FLAG_COUNT_WORK) != 0};
    return s.last.counted;
}

}  // namespace srt
