// srt_visibility_host.h — host-side rules of the per-pixel visibility pass (srt_render_visibility, srt_bind_visibility,
// srt_read_visibility, srt_get_visibility_work) that need no device: argument validation in the header's order, the record of
// which outputs the last call wrote to which buffers (srt_read_visibility reads no other), and when the work record may be
// read (srt_outputs_host.h's LastOutputs and CallRecord).  Plain C++ without HIP, shared by srt_capi.hip and by tests/native/visibility_check.cpp, which runs it under the
// address and undefined-behaviour sanitizers on the CPU.
#pragma once

#include "srt_rays_host.h"

namespace srt {

constexpr uint32_t VIS_OUT_AO = 1u, VIS_OUT_SUN = 2u, VIS_OUT_ALL = 3u;
constexpr uint32_t VIS_FLAG_COUNT_WORK = 1u, VIS_FLAG_ALL = 1u;
constexpr int VIS_SLOTS = 2;
constexpr int VIS_GUIDES = 3;  // OBJECT, NORMAL_DEPTH, POSITION: the first three G-buffer slots
constexpr uint32_t VIS_MAX_SAMPLES = 4096u;

// the fields of srt_visibility_params, in its order
struct VisibilityCall {
    int32_t row_begin, row_end;
    uint32_t outputs, flags;
    uint32_t ao_samples, first_sample, seed;
    float ao_radius;
};

// what the last successful srt_render_visibility left behind
struct VisibilityState {
    CallRecord call;  // counted: it had SRT_VIS_COUNT_WORK
    LastOutputs<VIS_SLOTS> last;
};

// slot of a single output bit, -1 for anything else (no bit, both bits, an unknown bit)
inline int visibility_slot(uint32_t output) { return output == VIS_OUT_AO ? 0 : output == VIS_OUT_SUN ? 1 : -1; }

// srt_render_visibility's checks, in srt_trace_occlusion's order — the scene, the arguments, the inputs; touches nothing.
// guide_present[i]: G-buffer slot i has been bound or rendered.
inline RaysStatus visibility_check(const VisibilityCall& v, bool scene_set, int height, const bool guide_present[VIS_GUIDES], const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!scene_set) return *why = "srt_set_scene has not been called", RAYS_STATE;
    if (v.row_begin < 0 || v.row_end > height || v.row_begin >= v.row_end) return *why = "bad row band", RAYS_INVALID_ARG;
    if (v.outputs == 0 || (v.outputs & ~VIS_OUT_ALL)) return *why = "outputs: want a non-empty set of SRT_VIS_AO / SRT_VIS_SUN", RAYS_INVALID_ARG;
    if (v.flags & ~VIS_FLAG_ALL) return *why = "unknown flags", RAYS_INVALID_ARG;
    if (v.outputs & VIS_OUT_AO) {
        if (v.ao_samples < 1 || v.ao_samples > VIS_MAX_SAMPLES) return *why = "ao_samples outside 1 .. 4096", RAYS_INVALID_ARG;
        if (v.first_sample == 0) return *why = "first_sample must be >= 1", RAYS_INVALID_ARG;
        if ((uint64_t)v.first_sample + v.ao_samples - 1u > 0xFFFFFFFFull) return *why = "first_sample + ao_samples - 1 exceeds 2^32 - 1", RAYS_INVALID_ARG;
        if (!(v.ao_radius > 0.0f)) return *why = "ao_radius must be > 0 (+inf allowed)", RAYS_INVALID_ARG;  // (a NaN fails the comparison)
    }
    static const char* const missing[VIS_GUIDES] = {"the OBJECT guide has neither been bound nor rendered (srt_render_gbuffer)",
                                                    "the NORMAL_DEPTH guide has neither been bound nor rendered (srt_render_gbuffer)",
                                                    "the POSITION guide has neither been bound nor rendered (srt_render_gbuffer)"};
    for (int i = 0; i < VIS_GUIDES; ++i)
        if (!guide_present[i]) return *why = missing[i], RAYS_STATE;
    return RAYS_OK;
}

// srt_render_visibility once the launch is enqueued: it wrote `outputs`, output of slot i to dst[i], and nothing else.
inline void visibility_rendered(VisibilityState& s, uint32_t outputs, void* const dst[VIS_SLOTS], uint32_t flags) {
    s.call.done((flags & VIS_FLAG_COUNT_WORK) != 0);
    s.last.wrote(outputs, dst);
}

}  // namespace srt
