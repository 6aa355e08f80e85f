// srt_light_probes_host.h — host-side rules of the light probes (srt_write_light_probes, srt_bind_light_probes, the two
// direction calls, srt_trace_light_probes, srt_bind_light_probe_output, srt_read_light_probe_output, srt_get_light_probe_work)
// that need no device: which arrays are the current positions and directions (srt_outputs_host.h's InputArray), argument
// validation in the header's order, the continuation rule (no RESET needs the RADIANCE output and a previous trace of the same P
// and K into the same buffer), the record of what the last trace wrote and where and whether it counted (LastOutputs,
// CallRecord), and the sizes of the launch: the units, the grid, the
// partial buffer of a multi-block projection and the sample scratch that goes with the grid.  The two pure-host entries
// (srt_light_probe_sphere, srt_light_probe_irradiance) are here as well.  Plain C++ without HIP, shared by srt_capi.hip and by
// tests/native/light_probe_check.cpp, which runs it under the address and undefined-behaviour sanitizers on the CPU.
#pragma once

#include <math.h>

#include "srt_radiance_host.h"

namespace srt {

constexpr uint32_t LIGHT_PROBE_FLAG_RESET = 1u, LIGHT_PROBE_FLAG_NORMALIZE = 2u, LIGHT_PROBE_FLAG_COUNT_WORK = 4u, LIGHT_PROBE_FLAG_ALL = 7u;
constexpr uint32_t LIGHT_PROBE_OUT_COEFFICIENTS = 1u, LIGHT_PROBE_OUT_RADIANCE = 2u, LIGHT_PROBE_OUT_ALL = 3u;
constexpr int LIGHT_PROBE_SLOTS = 2;
constexpr int LIGHT_PROBE_COEFFS = 9;  // float4 per probe: bands 0..2
constexpr size_t LIGHT_PROBE_MAX_DIRECTIONS = 4096;
constexpr size_t LIGHT_PROBE_MAX_RAYS = RAYS_MAX_COUNT;  // P*K: srt_trace_radiance's batch limit

// the fields of srt_light_probe_params, in its order
struct LightProbeCall {
    uint32_t first_sample, sample_count;
    int32_t max_bounces;
    uint32_t seed, id_base, flags, outputs, reserved;
};

inline void light_probe_call_default(LightProbeCall& c) {
    c.first_sample = 1, c.sample_count = 16, c.max_bounces = 8, c.seed = 0, c.id_base = 0, c.flags = LIGHT_PROBE_FLAG_RESET;
    c.outputs = LIGHT_PROBE_OUT_COEFFICIENTS, c.reserved = 0;
}

// slot of a single output bit, -1 for anything else
inline int light_probe_slot(uint32_t output) { return output == LIGHT_PROBE_OUT_COEFFICIENTS ? 0 : output == LIGHT_PROBE_OUT_RADIANCE ? 1 : -1; }

struct LightProbeState {
    InputArray positions, directions;
    // the last successful srt_trace_light_probes
    CallRecord call;  // counted: it had SRT_LIGHT_PROBE_COUNT_WORK
    size_t last_probes = 0, last_directions = 0;
    LastOutputs<LIGHT_PROBE_SLOTS> last;
};

// direction blocks of 64 per probe, and the units (probe, block) of a launch
inline size_t light_probe_blocks(size_t directions) { return (directions + 63) / 64; }
inline size_t light_probe_units(size_t probes, size_t directions) { return probes * light_probe_blocks(directions); }
// elements (float4) of an output of a trace of P probes and K directions
inline size_t light_probe_elems(int slot, size_t probes, size_t directions) { return slot == 0 ? probes * (size_t)LIGHT_PROBE_COEFFS : probes * directions; }
// The partial buffer [P][J][9] float4 of a projection over J > 1 blocks; none (0) when J == 1: lane 0 writes the output itself.
inline size_t light_probe_partial_bytes(size_t probes, size_t directions) {
    const size_t J = light_probe_blocks(directions);
    return J > 1 ? probes * J * (size_t)LIGHT_PROBE_COEFFS * (4 * sizeof(float)) : 0;
}
// The grid: radiance_kernel's — persistent workgroups of `waves` waves over the units, at most `resident`.
inline unsigned light_probe_grid(size_t probes, size_t directions, int waves, long long resident) {
    return persistent_grid((long long)light_probe_units(probes, directions), waves, resident);
}
// the sample scratch of the launch: radiance_kernel's, a function of the grid alone
inline size_t light_probe_scratch_bytes(unsigned workgroups, int waves) { return radiance_scratch_bytes(workgroups, waves); }

// srt_trace_light_probes' checks in the header's order: the scene, the arguments, the inputs, the continuation; touches nothing.
// `radiance_target`: the buffer the RADIANCE output would go to now (the bound one, else the own one; NULL: no own buffer yet).
inline RaysStatus light_probe_check_trace(const LightProbeState& s, bool scene_set, const LightProbeCall& c, const void* radiance_target, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!scene_set) return *why = "srt_set_scene has not been called", RAYS_STATE;
    if (c.flags & ~LIGHT_PROBE_FLAG_ALL) return *why = "unknown flags", RAYS_INVALID_ARG;
    if (c.outputs == 0 || (c.outputs & ~LIGHT_PROBE_OUT_ALL)) return *why = "outputs: want a non-empty set of SRT_LIGHT_PROBE_COEFFICIENTS | SRT_LIGHT_PROBE_RADIANCE", RAYS_INVALID_ARG;
    if (c.first_sample == 0) return *why = "first_sample must be >= 1", RAYS_INVALID_ARG;
    if (c.sample_count < 1 || c.sample_count > RADIANCE_MAX_SAMPLES) return *why = "sample_count outside 1 .. 4096", RAYS_INVALID_ARG;
    if ((uint64_t)c.first_sample + c.sample_count - 1u > 0xFFFFFFFFull) return *why = "first_sample + sample_count - 1 exceeds 2^32 - 1", RAYS_INVALID_ARG;
    if (c.max_bounces < 0) return *why = "max_bounces must be >= 0", RAYS_INVALID_ARG;
    if (c.reserved != 0) return *why = "reserved must be 0", RAYS_INVALID_ARG;
    const size_t P = s.positions.count(), K = s.directions.count();
    if (P == 0) return *why = "no probe positions have been written or bound (srt_write_light_probes, srt_bind_light_probes)", RAYS_STATE;
    if (K == 0) return *why = "no directions have been written or bound (srt_write_light_probe_directions, srt_bind_light_probe_directions)", RAYS_STATE;
    if (K > LIGHT_PROBE_MAX_DIRECTIONS) return *why = "direction count outside 1 .. 4096", RAYS_INVALID_ARG;
    if (P > LIGHT_PROBE_MAX_RAYS || P * K > LIGHT_PROBE_MAX_RAYS) return *why = "probes x directions exceeds 2^30", RAYS_INVALID_ARG;
    if (!(c.flags & LIGHT_PROBE_FLAG_RESET)) {
        if (!(c.outputs & LIGHT_PROBE_OUT_RADIANCE)) return *why = "continuing the means (no SRT_LIGHT_PROBE_RESET) needs the RADIANCE output", RAYS_STATE;
        if (!radiance_target || s.last.read(LIGHT_PROBE_OUT_RADIANCE, 1) != radiance_target || s.last_probes != P || s.last_directions != K)
            return *why = "continuing the means (no SRT_LIGHT_PROBE_RESET) needs a previous trace of the same probe and direction counts into the current RADIANCE buffer",
                   RAYS_STATE;
    }
    return RAYS_OK;
}

// srt_trace_light_probes once the launch is enqueued: dst[slot] is where each requested output went.
inline void light_probe_traced(LightProbeState& s, size_t probes, size_t directions, uint32_t outputs, void* const dst[LIGHT_PROBE_SLOTS], uint32_t flags) {
    s.call.done((flags & LIGHT_PROBE_FLAG_COUNT_WORK) != 0);
    s.last_probes = probes, s.last_directions = directions;
    s.last.wrote(outputs, dst);
}

// srt_light_probe_sphere: the spherical Fibonacci set, computed in double and rounded once to binary32.
inline void light_probe_sphere(size_t count, float* dst) {
    const double pi = 3.14159265358979323846;
    const double golden = pi * (3.0 - sqrt(5.0));
    const float w = (float)(4.0 * pi / (double)count);
    for (size_t i = 0; i < count; ++i) {
        const double z = 1.0 - (2.0 * (double)i + 1.0) / (double)count;
        const double rr = 1.0 - z * z;
        const double r = sqrt(rr > 0.0 ? rr : 0.0);
        const double a = (double)i * golden;
        dst[4 * i + 0] = (float)(r * cos(a)), dst[4 * i + 1] = (float)(r * sin(a)), dst[4 * i + 2] = (float)z, dst[4 * i + 3] = w;
    }
}

// The nine basis values of the header's rule 3 on (x, y, z), in its order (the kernel restates them: the same expressions).
inline void light_probe_basis(float x, float y, float z, float b[LIGHT_PROBE_COEFFS]) {
    b[0] = 0.282095f;
    b[1] = 0.488603f * y;
    b[2] = 0.488603f * z;
    b[3] = 0.488603f * x;
    b[4] = 1.092548f * (x * y);
    b[5] = 1.092548f * (y * z);
    b[6] = 0.315392f * ((3.0f * (z * z)) - 1.0f);
    b[7] = 1.092548f * (x * z);
    b[8] = 0.546274f * ((x * x) - (y * y));
}

// srt_light_probe_irradiance: term_c = (A_c * coefficient_c[l]) * b_c(n), summed in ascending c.
inline void light_probe_irradiance(const float* coefficients, const float* normal, float* rgb) {
    float b[LIGHT_PROBE_COEFFS];
    light_probe_basis(normal[0], normal[1], normal[2], b);
    for (int l = 0; l < 3; ++l) {
        float e = 0.0f;
        for (int c = 0; c < LIGHT_PROBE_COEFFS; ++c) {
            const float a = c == 0 ? 3.14159274f : c < 4 ? 2.09439516f : 0.785398185f;
            const float t = (a * coefficients[4 * c + l]) * b[c];
            e = c == 0 ? t : e + t;
        }
        rgb[l] = e;
    }
}

}  // namespace srt
