// srt_reflection_host.h — host-side rules of the reflection guides (srt_render_reflection_gbuffer, srt_bind_reflection,
// srt_read_reflection, srt_device_reflection, srt_get_reflection_work) that need no device: argument validation in the header's
// order, the five output slots with their element sizes, the read rule (srt_read_gbuffer's: the current buffer, bound or own,
// once there is one) and when the work record may be read.  Plain C++ without HIP, shared by srt_capi.hip and by
// tests/native/reflection_check.cpp, which runs it under the address and undefined-behaviour sanitizers on the CPU.
#pragma once

#include "srt_rays_host.h"

namespace srt {

constexpr uint32_t REFL_OUT_OBJECT = 1u, REFL_OUT_NORMAL_DEPTH = 2u, REFL_OUT_POSITION = 4u, REFL_OUT_ALBEDO = 8u, REFL_OUT_BOUNCES = 16u;
constexpr uint32_t REFL_OUT_GUIDES = 15u, REFL_OUT_ALL = 31u;
constexpr uint32_t REFL_FLAG_COUNT_WORK = 1u, REFL_FLAG_ALL = 1u;
constexpr int REFL_SLOTS = 5;
constexpr int REFL_MAX_BOUNCES = 64;

// the fields of srt_reflection_params, in its order
struct ReflectionCall {
    int32_t row_begin, row_end;
    uint32_t outputs, flags;
    int32_t max_bounces;
    float min_smoothness, min_specular;
    uint32_t reserved;
};

// the five outputs: the handle's own buffers are the caller's business (srt_capi.hip); the slots say which buffer is current
struct ReflectionSlots {
    OutputSlot out[REFL_SLOTS];
};

// slot of a single output bit, -1 for anything else (no bit, several bits, an unknown bit)
inline int reflection_slot(uint32_t output) {
    switch (output) {
        case REFL_OUT_OBJECT: return 0;
        case REFL_OUT_NORMAL_DEPTH: return 1;
        case REFL_OUT_POSITION: return 2;
        case REFL_OUT_ALBEDO: return 3;
        case REFL_OUT_BOUNCES: return 4;
        default: return -1;
    }
}
// bytes per pixel of a slot: int32 for OBJECT and BOUNCES, float4 for the three between (the SRT_GBUF_* element types)
inline size_t reflection_elem_bytes(int slot) { return slot == 0 || slot == 4 ? 4u : 16u; }

// the defaults of srt_reflection_params_default: all five outputs, no flags, 8 reflections, mirrors only; the band is the caller's
inline ReflectionCall reflection_defaults() { return ReflectionCall{0, 0, REFL_OUT_ALL, 0u, 8, 1.0f, 1.0f, 0u}; }

// srt_render_reflection_gbuffer's checks, in the header's order; touches nothing.
inline RaysStatus reflection_check(const ReflectionCall& r, bool scene_set, bool camera_set, int height, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!scene_set) return *why = "srt_set_scene has not been called", RAYS_STATE;
    if (!camera_set) return *why = "srt_set_camera has not been called", RAYS_STATE;
    if (r.row_begin < 0 || r.row_end > height || r.row_begin >= r.row_end) return *why = "bad row band", RAYS_INVALID_ARG;
    if (r.outputs == 0 || (r.outputs & ~REFL_OUT_ALL)) return *why = "outputs: want a non-empty set of SRT_REFL_* bits", RAYS_INVALID_ARG;
    if (r.flags & ~REFL_FLAG_ALL) return *why = "unknown flags", RAYS_INVALID_ARG;
    if (r.reserved != 0) return *why = "reserved must be 0", RAYS_INVALID_ARG;
    if (r.max_bounces < 0 || r.max_bounces > REFL_MAX_BOUNCES) return *why = "max_bounces outside 0 .. 64", RAYS_INVALID_ARG;
    if (r.min_smoothness != r.min_smoothness) return *why = "min_smoothness is NaN", RAYS_INVALID_ARG;
    if (r.min_specular != r.min_specular) return *why = "min_specular is NaN", RAYS_INVALID_ARG;
    return RAYS_OK;
}

// srt_render_reflection_gbuffer once the launch is enqueued: it wrote `outputs`, output of slot i to dst[i].  `s`: what
// srt_get_reflection_work may report — only the record of a last call with SRT_REFL_COUNT_WORK.
inline void reflection_rendered(CallRecord& s, ReflectionSlots& slots, uint32_t outputs, void* const dst[REFL_SLOTS], uint32_t flags) {
    s.done((flags & REFL_FLAG_COUNT_WORK) != 0);
    for (int i = 0; i < REFL_SLOTS; ++i)
        if (outputs & (1u << i)) slots.out[i].wrote(dst[i]);
}

// srt_read_reflection: the buffer to copy W * H elements from — the current one, bound or own (own[i]: NULL before its first
// use) — or why not.
inline RaysStatus reflection_check_read(const ReflectionSlots& slots, uint32_t output, const void* const own[REFL_SLOTS], const void** src) {
    const int i = reflection_slot(output);
    if (i < 0) return RAYS_INVALID_ARG;
    const void* c = slots.out[i].current(own[i]);
    if (!c) return RAYS_STATE;
    *src = c;
    return RAYS_OK;
}

}  // namespace srt
