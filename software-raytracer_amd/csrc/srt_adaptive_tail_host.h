// srt_adaptive_tail_host.h — host-side rules of srt_render_adaptive_tail (the adaptive render whose paths end in the probe grid)
// that need no device: the order of its checks (rule R1 of srt_pathtrace.h: srt_render_adaptive's own errors, then the mode, then
// what an affected trace requires of the grid's inputs, with the accumulator AND the framebuffer as the buffers about to be
// written), which kernel the call launches (R2), and what it leaves in the adaptive and the probe-tail state (R6).  A composition
// of srt_adaptive_host.h and srt_probe_tail_host.h.  Plain C++ without HIP, shared by srt_capi.hip and by
// tests/native/adaptive_tail_check.cpp, which runs it under the address and undefined-behaviour sanitizers on the CPU.
#pragma once

#include "srt_adaptive_host.h"
#include "srt_probe_tail_host.h"

namespace srt {

// the two buffers the call writes that the tail's coefficient array may not share a byte with (the counts are uint32 per pixel
// and are read before they are written by the same lane: no path reads them)
struct AdaptiveTailTargets {
    const void* accumulator;  // W*H float4
    size_t accumulator_bytes;
    const void* framebuffer;  // W*H uint32
    size_t framebuffer_bytes;
};

inline AdaptiveTailTargets adaptive_tail_targets(const void* accumulator, const void* framebuffer, int width, int height) {
    const size_t pixels = (width > 0 && height > 0) ? (size_t)width * (size_t)height : 0;
    return AdaptiveTailTargets{accumulator, pixels * (4 * sizeof(float)), framebuffer, pixels * sizeof(uint32_t)};
}

// Rule R1, in its order; touches nothing.
//   1. srt_render_adaptive's own errors (adaptive_check), in its order
//   2. RAYS_STATE when the mode is off (also: there has never been an accepted srt_probe_tail with enabled = 1)
//   3. only for max_bounces >= 1: probe_tail_check_trace's refusals, the coefficient array against the accumulator, then against
//      the framebuffer
inline RaysStatus adaptive_tail_check(const AdaptiveCall& c, bool scene_set, bool camera_set, int height, bool counts_present, bool budget_present,
                                      const ProbeTailState& tail, const ProbeGridState& g, const ProbeGridDepthState& d, const ProbeStatesState& st,
                                      const void* coefficients, const AdaptiveTailTargets& w, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (const RaysStatus rs = adaptive_check(c, scene_set, camera_set, height, counts_present, budget_present, why)) return rs;
    if (!tail.enabled) return *why = "srt_probe_tail is off (srt_probe_tail with enabled = 1 comes first)", RAYS_STATE;
    if (!probe_tail_applies(tail, c.max_bounces)) return RAYS_OK;  // R2 (T1): no grid input is checked
    if (const RaysStatus rs = probe_tail_check_trace(tail, g, d, st, coefficients, w.accumulator, w.accumulator_bytes, why)) return rs;
    if (probe_tail_ranges_overlap(coefficients, probe_grid_probes(g.grid) * (size_t)LIGHT_PROBE_COEFFS * (4 * sizeof(float)), w.framebuffer, w.framebuffer_bytes))
        return *why = "srt_probe_tail would read the coefficient array this call writes: the framebuffer overlaps it", RAYS_STATE;
    return RAYS_OK;
}

// Rule R2: an accepted call with max_bounces == 0 launches exactly what srt_render_adaptive launches.
inline bool adaptive_tail_launches_tail(const ProbeTailState& tail, const AdaptiveCall& c) { return probe_tail_applies(tail, c.max_bounces); }

// Rule R6, once the launch is enqueued: an adaptive render for srt_get_adaptive_work and the last affected trace for
// srt_get_probe_tail_work.  True when the tail's record is this call's (the caller has zeroed it in front of the launch: all
// zeros under R2).
inline bool adaptive_tail_rendered(AdaptiveState& a, ProbeTailState& tail, uint32_t flags) {
    adaptive_rendered(a, flags);
    return probe_tail_traced(tail);
}

}  // namespace srt
