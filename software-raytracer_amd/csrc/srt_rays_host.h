// srt_rays_host.h — host-side rules of the ray queries (srt_write_rays, srt_bind_rays, srt_bind_ray_output, srt_trace_rays,
// srt_read_ray_output) that need no device: argument validation, which arrays are the current rays, element sizes, and the
// record of what the last trace wrote (srt_outputs_host.h's LastOutputs, with the ray count that sizes a read).  Plain C++ without HIP, shared by srt_capi.hip and by tests/native/rays_check.cpp,
// which runs it under the address and undefined-behaviour sanitizers on the CPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "srt_outputs_host.h"

namespace srt {

constexpr uint32_t RAYS_OUT_OBJECT = 1u, RAYS_OUT_NORMAL_DEPTH = 2u, RAYS_OUT_POSITION = 4u, RAYS_OUT_ALBEDO = 8u, RAYS_OUT_OCCLUDED = 16u;
constexpr uint32_t RAYS_OUT_ALL = 31u;
constexpr uint32_t RAYS_FLAG_NORMALIZE = 1u, RAYS_FLAG_ALL = 1u;
constexpr int RAYS_SLOTS = 5;
constexpr size_t RAYS_MAX_COUNT = (size_t)1 << 30;

// slot of a single output bit, -1 for anything else (no bit, several bits, an unknown bit)
inline int rays_slot(uint32_t output) {
    switch (output) {
        case RAYS_OUT_OBJECT: return 0;
        case RAYS_OUT_NORMAL_DEPTH: return 1;
        case RAYS_OUT_POSITION: return 2;
        case RAYS_OUT_ALBEDO: return 3;
        case RAYS_OUT_OCCLUDED: return 4;
        default: return -1;
    }
}
// bytes of one element of a slot: int32 for OBJECT and OCCLUDED, float4 for the others
inline size_t rays_elem_bytes(int slot) { return slot == 0 || slot == 4 ? sizeof(int32_t) : 4 * sizeof(float); }
inline bool rays_count_ok(size_t count) { return count >= 1 && count <= RAYS_MAX_COUNT; }

// Which arrays are the current rays.  The handle's own buffers hold origins.own_count rays (0: never written); the caller's
// bound arrays, when there are any, come first.
struct RaysState {
    InputArray origins;                     // the origins, and the one count of both arrays
    const void* bound_direction = nullptr;  // the directions bound with origins.bound
    // the last trace: how many rays, which outputs, and the buffer each was written to (srt_read_ray_output reads no other)
    size_t last_count = 0;
    LastOutputs<RAYS_SLOTS> last;

    bool bound() const { return origins.bound != nullptr; }
    size_t count() const { return origins.count(); }  // 0: no current rays
};

// srt_bind_rays: NULL, NULL, 0 returns to the own buffers; otherwise both arrays and a count in range.  On an error the state
// is left as it was.
inline RaysStatus rays_bind(RaysState& s, const void* d_origins, const void* d_directions, size_t count) {
    if (!d_origins && !d_directions && count == 0) return s.bound_direction = nullptr, input_bind(s.origins, nullptr, 0, RAYS_MAX_COUNT);
    if (!d_origins || !d_directions || input_bind(s.origins, d_origins, count, RAYS_MAX_COUNT) != RAYS_OK) return RAYS_INVALID_ARG;
    s.bound_direction = d_directions;
    return RAYS_OK;
}

// srt_write_rays once the copy has succeeded: the own buffers hold `count` rays and are the current ones.
inline void rays_written(RaysState& s, size_t count) { input_written(s.origins, count), s.bound_direction = nullptr; }

// srt_trace_rays' checks, in the order the header gives them; touches nothing.
inline RaysStatus rays_check_trace(const RaysState& s, bool scene_set, uint32_t outputs, uint32_t flags, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!scene_set) return *why = "srt_set_scene has not been called", RAYS_STATE;
    if (outputs == 0 || (outputs & ~RAYS_OUT_ALL)) return *why = "outputs: want a non-empty set of SRT_GBUF_* / SRT_RAYS_OCCLUDED bits", RAYS_INVALID_ARG;
    if (flags & ~RAYS_FLAG_ALL) return *why = "unknown flags", RAYS_INVALID_ARG;
    if (s.count() == 0) return *why = "no rays have been written or bound (srt_write_rays, srt_bind_rays)", RAYS_STATE;
    if (!rays_count_ok(s.count())) return *why = "ray count outside 1 .. 2^30", RAYS_INVALID_ARG;
    return RAYS_OK;
}

// srt_trace_rays once the launch is enqueued: dst[slot] is where each requested output goes.
inline void rays_traced(RaysState& s, uint32_t outputs, void* const dst[RAYS_SLOTS]) { s.last_count = s.count(), s.last.wrote(outputs, dst); }

// Persistent workgroups of `waves` waves for `count` rays in blocks of 64: as many as there are blocks for, at most `resident`.
inline unsigned rays_grid(size_t count, int waves, long long resident) { return persistent_grid((long long)((count + 63) / 64), waves, resident); }

}  // namespace srt
