// srt_radiance_host.h — host-side rules of the radiance queries (srt_trace_radiance, srt_bind_radiance, srt_read_radiance,
// srt_get_radiance_work) that need no device: argument validation in the header's order, the record of what the last radiance
// trace wrote and where — its own record: a radiance trace is not "the last trace" of srt_read_ray_output and leaves RaysState
// alone — whether it counted its work, and the sizes of the launch: the grid, and the sample scratch that goes with the grid.
// Plain C++ without HIP, shared by srt_capi.hip and by tests/native/radiance_check.cpp, which runs it under the address and
// undefined-behaviour sanitizers on the CPU.
#pragma once

#include "srt_rays_host.h"

namespace srt {

constexpr uint32_t RADIANCE_FLAG_RESET = 1u, RADIANCE_FLAG_NORMALIZE = 2u, RADIANCE_FLAG_COUNT_WORK = 4u, RADIANCE_FLAG_ALL = 7u;
constexpr uint32_t RADIANCE_MAX_SAMPLES = 4096u;
// samples a wave keeps in flight per slot: rows of its scratch region (the kernel's RAD_CHUNK)
constexpr int RADIANCE_CHUNK = 64;

// the fields of srt_radiance_params, in its order
struct RadianceCall {
    uint32_t first_sample, sample_count;
    int32_t max_bounces;
    uint32_t seed, id_base, flags;
};

// what the last successful srt_trace_radiance left behind
struct RadianceState {
    CallRecord call;  // counted: it had SRT_RADIANCE_COUNT_WORK
    size_t last_count = 0;
    LastOutputs<1> last;  // (one output: bit 1, slot 0)
};

inline void radiance_call_default(RadianceCall& c) {
    c.first_sample = 1, c.sample_count = 16, c.max_bounces = 8, c.seed = 0, c.id_base = 0, c.flags = RADIANCE_FLAG_RESET;
}

// srt_trace_radiance's checks, in srt_trace_occlusion's order: the scene, the arguments, the rays; touches nothing.
inline RaysStatus radiance_check_trace(const RaysState& s, bool scene_set, const RadianceCall& c, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!scene_set) return *why = "srt_set_scene has not been called", RAYS_STATE;
    if (c.flags & ~RADIANCE_FLAG_ALL) return *why = "unknown flags", RAYS_INVALID_ARG;
    if (c.first_sample == 0) return *why = "first_sample must be >= 1", RAYS_INVALID_ARG;
    if (c.sample_count < 1 || c.sample_count > RADIANCE_MAX_SAMPLES) return *why = "sample_count outside 1 .. 4096", RAYS_INVALID_ARG;
    if ((uint64_t)c.first_sample + c.sample_count - 1u > 0xFFFFFFFFull) return *why = "first_sample + sample_count - 1 exceeds 2^32 - 1", RAYS_INVALID_ARG;
    if (c.max_bounces < 0) return *why = "max_bounces must be >= 0", RAYS_INVALID_ARG;
    if (s.count() == 0) return *why = "no rays have been written or bound (srt_write_rays, srt_bind_rays)", RAYS_STATE;
    if (!rays_count_ok(s.count())) return *why = "ray count outside 1 .. 2^30", RAYS_INVALID_ARG;
    return RAYS_OK;
}

// srt_trace_radiance once the launch is enqueued: `count` float4 went to `dst`.
inline void radiance_traced(RadianceState& r, size_t count, const void* dst, uint32_t flags) {
    r.call.done((flags & RADIANCE_FLAG_COUNT_WORK) != 0);
    r.last_count = count;
    r.last.wrote(1u, &dst);
}

// The grid: rays_kernel's — persistent workgroups of `waves` waves over blocks of 64 rays, at most `resident`.
inline unsigned radiance_grid(size_t count, int waves, long long resident) { return rays_grid(count, waves, resident); }

// The sample scratch of a launch of `workgroups` workgroups: every wave's own region of RADIANCE_CHUNK rows of 64 float4.  A
// function of the grid alone — at most `resident` workgroups — and never of the number of rays or samples.
inline size_t radiance_scratch_bytes(unsigned workgroups, int waves) {
    return (size_t)workgroups * (size_t)waves * (size_t)RADIANCE_CHUNK * 64 * (4 * sizeof(float));
}

}  // namespace srt
