// srt_adaptive_sun_host.h — host-side rules of SRT_ADAPTIVE_SUN_SAMPLING (rules AS1 - AS8 of srt_pathtrace.h) that need no device:
// the flag's acceptance in front of the two adaptive calls' own checks (which keep refusing every bit they do not know, 4 and 8
// among them, and keep ADAPTIVE_FLAG_ALL == 3), the order of the errors (AS5) and which of the four adaptive kernels an accepted
// call launches (AS6).  A composition of srt_adaptive_tail_host.h and srt_sun_sampling_host.h.  Plain C++ without HIP, shared by
// srt_capi.hip and by tests/native/adaptive_sun_check.cpp, which runs it under the address and undefined-behaviour sanitizers on
// the CPU.
#pragma once

#include "srt_adaptive_tail_host.h"
#include "srt_sun_sampling_host.h"

namespace srt {

constexpr uint32_t ADAPTIVE_FLAG_SUN_SAMPLING = SUN_SAMPLING_FLAG;  // SRT_ADAPTIVE_SUN_SAMPLING: the bit in srt_adaptive_params.flags

// AS5 for srt_render_adaptive: the call's own errors in their order with the bit taken out, then the direction test.  The call
// ignores the probe-tail mode (AS1), so S5's tail-mode refusal is not asked for.
inline RaysStatus sun_adaptive_check(AdaptiveCall c, bool scene_set, bool camera_set, int height, bool counts_present, bool budget_present,
                                     const float sun_direction[3], const char** why) {
    const bool asked = sun_sampling_asked(c.flags);
    c.flags &= ~ADAPTIVE_FLAG_SUN_SAMPLING;
    if (const RaysStatus rs = adaptive_check(c, scene_set, camera_set, height, counts_present, budget_present, why)) return rs;
    return asked ? sun_sampling_check(sun_direction, false, why) : RAYS_OK;
}

// AS5 for srt_render_adaptive_tail: all of R1 with the bit taken out, then the direction test.  The mode is on here by R1; the
// combination is built for this call (AS4), so the tail-mode refusal is not asked for either.
inline RaysStatus sun_adaptive_tail_check(AdaptiveCall c, bool scene_set, bool camera_set, int height, bool counts_present, bool budget_present,
                                          const ProbeTailState& tail, const ProbeGridState& g, const ProbeGridDepthState& d, const ProbeStatesState& st,
                                          const void* coefficients, const AdaptiveTailTargets& w, const float sun_direction[3], const char** why) {
    const bool asked = sun_sampling_asked(c.flags);
    c.flags &= ~ADAPTIVE_FLAG_SUN_SAMPLING;
    if (const RaysStatus rs = adaptive_tail_check(c, scene_set, camera_set, height, counts_present, budget_present, tail, g, d, st, coefficients, w, why)) return rs;
    return asked ? sun_sampling_check(sun_direction, false, why) : RAYS_OK;
}

// AS6: which kernel an accepted call launches.  `tail_call`: the call is srt_render_adaptive_tail (srt_render_adaptive ignores the
// mode).  With max_bounces == 0 there is neither a vertex nor a path end on a surface: adaptive_kernel, whatever was asked for.
enum AdaptiveKernelChoice { ADAPTIVE_KERNEL_PLAIN = 0, ADAPTIVE_KERNEL_TAIL = 1, ADAPTIVE_KERNEL_SUN = 2, ADAPTIVE_KERNEL_TAIL_SUN = 3 };
inline AdaptiveKernelChoice adaptive_kernel_choice(bool tail_call, const ProbeTailState& tail, const AdaptiveCall& c) {
    const bool t = tail_call && adaptive_tail_launches_tail(tail, c);
    const bool s = sun_sampling_applies(c.flags, c.max_bounces);
    return (AdaptiveKernelChoice)((t ? 1 : 0) | (s ? 2 : 0));
}

}  // namespace srt
