// srt_occlusion_host.h — host-side rules of the any-hit queries (srt_trace_occlusion, srt_get_occlusion_work) that need no
// device: argument validation in the header's order, the "last trace" record — an occlusion trace is a trace that wrote the
// SRT_RAYS_OCCLUDED output alone, so srt_read_ray_output reads it through srt_rays_host.h's RaysState unchanged — and whether
// the last occlusion trace counted its work (a CallRecord).  Plain C++ without HIP, shared by srt_capi.hip and by
// tests/native/occlusion_check.cpp, which runs it under the address and undefined-behaviour sanitizers on the CPU.
#pragma once

#include "srt_rays_host.h"

namespace srt {

constexpr uint32_t OCCLUSION_FLAG_NORMALIZE = 1u, OCCLUSION_FLAG_COUNT_WORK = 2u, OCCLUSION_FLAG_ALL = 3u;
constexpr int OCCLUSION_SLOT = 4;  // rays_slot(RAYS_OUT_OCCLUDED)

// srt_trace_occlusion's checks, in srt_trace_rays' order: the scene, the arguments, the rays; touches nothing.
inline RaysStatus occlusion_check_trace(const RaysState& s, bool scene_set, uint32_t flags, uint32_t reserved, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!scene_set) return *why = "srt_set_scene has not been called", RAYS_STATE;
    if (flags & ~OCCLUSION_FLAG_ALL) return *why = "unknown flags", RAYS_INVALID_ARG;
    if (reserved != 0) return *why = "reserved must be 0", RAYS_INVALID_ARG;
    if (s.count() == 0) return *why = "no rays have been written or bound (srt_write_rays, srt_bind_rays)", RAYS_STATE;
    if (!rays_count_ok(s.count())) return *why = "ray count outside 1 .. 2^30", RAYS_INVALID_ARG;
    return RAYS_OK;
}

// srt_trace_occlusion once the launch is enqueued: it is the last trace and wrote OCCLUDED, to `dst`, and nothing else.  `w`: what
// srt_get_occlusion_work may report — nothing before the first occlusion trace, and nothing after one without COUNT_WORK.
inline void occlusion_traced(RaysState& s, CallRecord& w, void* dst, uint32_t flags) {
    void* slots[RAYS_SLOTS] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    slots[OCCLUSION_SLOT] = dst;
    rays_traced(s, RAYS_OUT_OCCLUDED, slots);
    w.done((flags & OCCLUSION_FLAG_COUNT_WORK) != 0);
}

}  // namespace srt
