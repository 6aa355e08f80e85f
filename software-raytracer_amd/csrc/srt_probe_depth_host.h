// srt_probe_depth_host.h — host-side rules of the probe depth pass (srt_trace_probe_depth, srt_bind_probe_depth_output,
// srt_read_probe_depth_output, srt_get_probe_depth_work) and of the filtered probe-grid shading (srt_write_probe_grid_depth,
// srt_bind_probe_grid_depth, srt_shade_probe_grid_depth) that need no device: argument validation in the header's order, the sizes
// of the outputs, the record of what the last depth trace wrote and where, whether it counted, which moment array is current and
// with which resolution.  The three pure-host entries (srt_probe_depth_params_default, srt_probe_depth_texels,
// srt_probe_grid_depth_params_default) are here as well.  Plain C++ without HIP, shared by srt_capi.hip and by
// tests/native/probe_depth_check.cpp, which runs it under the address and undefined-behaviour sanitizers on the CPU.
#pragma once

#include <math.h>

#include "srt_probe_grid_host.h"

namespace srt {

constexpr uint32_t PROBE_DEPTH_FLAG_NORMALIZE = 1u, PROBE_DEPTH_FLAG_COUNT_WORK = 2u, PROBE_DEPTH_FLAG_ALL = 3u;
constexpr uint32_t PROBE_DEPTH_OUT_MOMENTS = 1u, PROBE_DEPTH_OUT_DISTANCES = 2u, PROBE_DEPTH_OUT_ALL = 3u;
constexpr int PROBE_DEPTH_SLOTS = 2;
constexpr uint32_t PROBE_DEPTH_MAX_SHARPNESS = 6;
constexpr size_t PROBE_DEPTH_MAX_ELEMS = (size_t)1 << 30;  // P*K and P*R*R
constexpr size_t PROBE_DEPTH_TABLE = 16 + 64 + 256;        // float4 of the three texel tables, R = 4, 8, 16 in this order

// the fields of srt_probe_depth_params, in its order
struct ProbeDepthCall {
    uint32_t resolution, sharpness;
    float max_distance;
    uint32_t flags, outputs, reserved;
};

// the fields of srt_probe_grid_depth_params, in its order
struct ProbeGridDepthCall {
    float bias, min_variance;
    uint32_t reserved[2];
};

inline void probe_depth_call_default(ProbeDepthCall& c) {
    c.resolution = 16, c.sharpness = 5, c.max_distance = 10000.0f, c.flags = 0, c.outputs = PROBE_DEPTH_OUT_MOMENTS, c.reserved = 0;
}
inline void probe_grid_depth_call_default(ProbeGridDepthCall& c) { c.bias = 0.0f, c.min_variance = 1e-4f, c.reserved[0] = 0, c.reserved[1] = 0; }

inline bool probe_depth_resolution_ok(uint32_t r) { return r == 4 || r == 8 || r == 16; }
// where the table of resolution R starts in the three tables laid end to end
inline size_t probe_depth_table_offset(uint32_t r) { return r == 4 ? 0 : r == 8 ? 16 : 16 + 64; }

// slot of a single output bit, -1 for anything else
inline int probe_depth_slot(uint32_t output) { return output == PROBE_DEPTH_OUT_MOMENTS ? 0 : output == PROBE_DEPTH_OUT_DISTANCES ? 1 : -1; }

// bytes of an output of a trace of P probes, K directions and resolution R: MOMENTS P*R*R float4, DISTANCES P*K float
inline size_t probe_depth_bytes(int slot, size_t probes, size_t directions, uint32_t resolution) {
    return slot == 0 ? probes * (size_t)resolution * resolution * (4 * sizeof(float)) : probes * directions * sizeof(float);
}

// srt_probe_depth_texels (rule 1): texel (i, j) at index j*R + i; the octahedral direction of the texel's centre in double,
// each component rounded once to binary32, w = 0.
inline void probe_depth_texels(uint32_t R, float* dst) {
    for (uint32_t j = 0; j < R; ++j)
        for (uint32_t i = 0; i < R; ++i) {
            const double u = (2.0 * (double)i + 1.0) / (double)R - 1.0, v = (2.0 * (double)j + 1.0) / (double)R - 1.0;
            const double z = 1.0 - fabs(u) - fabs(v);
            double x = u, y = v;
            if (z < 0.0) x = (1.0 - fabs(v)) * (u >= 0.0 ? 1.0 : -1.0), y = (1.0 - fabs(u)) * (v >= 0.0 ? 1.0 : -1.0);
            const double len = sqrt(x * x + y * y + z * z);
            float* o = dst + 4 * ((size_t)j * R + i);
            o[0] = (float)(x / len), o[1] = (float)(y / len), o[2] = (float)(z / len), o[3] = 0.0f;
        }
}

struct ProbeDepthState {
    // the last successful srt_trace_probe_depth
    CallRecord call;  // counted: it had SRT_PROBE_DEPTH_COUNT_WORK
    size_t last_probes = 0, last_directions = 0;
    uint32_t last_resolution = 0;
    LastOutputs<PROBE_DEPTH_SLOTS> last;
};

// srt_trace_probe_depth's checks in the header's order (rule 7): the scene, the arguments, the inputs, the sizes; touches nothing.
inline RaysStatus probe_depth_check_trace(const LightProbeState& in, bool scene_set, const ProbeDepthCall& c, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!scene_set) return *why = "srt_set_scene has not been called", RAYS_STATE;
    if (c.flags & ~PROBE_DEPTH_FLAG_ALL) return *why = "unknown flags", RAYS_INVALID_ARG;
    if (c.outputs == 0 || (c.outputs & ~PROBE_DEPTH_OUT_ALL)) return *why = "outputs: want a non-empty set of SRT_PROBE_DEPTH_MOMENTS | SRT_PROBE_DEPTH_DISTANCES", RAYS_INVALID_ARG;
    if (!probe_depth_resolution_ok(c.resolution)) return *why = "resolution must be 4, 8 or 16", RAYS_INVALID_ARG;
    if (c.sharpness > PROBE_DEPTH_MAX_SHARPNESS) return *why = "sharpness outside 0 .. 6", RAYS_INVALID_ARG;
    if (!(c.max_distance > 0.0f) || !isfinite(c.max_distance)) return *why = "max_distance must be finite and > 0", RAYS_INVALID_ARG;  // (a NaN fails the comparison)
    if (c.reserved != 0) return *why = "reserved must be 0", RAYS_INVALID_ARG;
    const size_t P = in.positions.count(), K = in.directions.count();
    if (P == 0) return *why = "no probe positions have been written or bound (srt_write_light_probes, srt_bind_light_probes)", RAYS_STATE;
    if (K == 0) return *why = "no directions have been written or bound (srt_write_light_probe_directions, srt_bind_light_probe_directions)", RAYS_STATE;
    if (P > PROBE_DEPTH_MAX_ELEMS || P * K > PROBE_DEPTH_MAX_ELEMS) return *why = "probes x directions exceeds 2^30", RAYS_INVALID_ARG;
    if (P * (size_t)c.resolution * c.resolution > PROBE_DEPTH_MAX_ELEMS) return *why = "probes x resolution^2 exceeds 2^30", RAYS_INVALID_ARG;
    return RAYS_OK;
}

// srt_trace_probe_depth once the launch is enqueued: dst[slot] is where each requested output went.
inline void probe_depth_traced(ProbeDepthState& s, size_t probes, size_t directions, const ProbeDepthCall& c, void* const dst[PROBE_DEPTH_SLOTS]) {
    s.call.done((c.flags & PROBE_DEPTH_FLAG_COUNT_WORK) != 0);
    s.last_probes = probes, s.last_directions = directions, s.last_resolution = c.resolution;
    s.last.wrote(c.outputs, dst);
}

// The grid: one wave per probe, persistent workgroups of `waves` waves, at most `resident`.
inline unsigned probe_depth_grid(size_t probes, int waves, long long resident) { return persistent_grid((long long)probes, waves, resident); }

// ---- the moments srt_shade_probe_grid_depth reads: counted in probes, R*R float4 each --------------------------------------------
struct ProbeGridDepthState {
    InputArray moments;
    uint32_t bound_resolution = 0, own_resolution = 0;
    uint32_t resolution() const { return moments.bound ? bound_resolution : own_resolution; }
};

// srt_write_probe_grid_depth / srt_bind_probe_grid_depth: is (probes, resolution) an array of depth maps?
inline RaysStatus probe_grid_depth_check_input(size_t probes, uint32_t resolution) {
    if (!probe_depth_resolution_ok(resolution)) return RAYS_INVALID_ARG;
    if (probes < 1 || probes > PROBE_DEPTH_MAX_ELEMS || probes * (size_t)resolution * resolution > PROBE_DEPTH_MAX_ELEMS) return RAYS_INVALID_ARG;
    return RAYS_OK;
}
// srt_bind_probe_grid_depth: NULL, 0 (any resolution) returns to the own array.  On an error the state is left as it was.
inline RaysStatus probe_grid_depth_bind(ProbeGridDepthState& s, const void* d_ptr, size_t probes, uint32_t resolution) {
    if (!d_ptr && probes == 0) return s.moments.bound = nullptr, s.moments.bound_count = 0, s.bound_resolution = 0, RAYS_OK;
    if (!d_ptr || probe_grid_depth_check_input(probes, resolution) != RAYS_OK) return RAYS_INVALID_ARG;
    s.moments.bound = d_ptr, s.moments.bound_count = probes, s.bound_resolution = resolution;
    return RAYS_OK;
}
// srt_write_probe_grid_depth once the copy has succeeded: a binding ends
inline void probe_grid_depth_written(ProbeGridDepthState& s, size_t probes, uint32_t resolution) {
    input_written(s.moments, probes);
    s.own_resolution = resolution, s.bound_resolution = 0;
}

// srt_shade_probe_grid_depth's checks: srt_shade_probe_grid's (rule 16) with SRT_PROBE_GRID_VISIBILITY among the unknown flags,
// then the depth maps, then the depth parameters; touches nothing.
inline RaysStatus probe_grid_depth_check_shade(const ProbeGridState& s, const ProbeGridDepthState& d, const ProbeGridCall& c, const ProbeGridDepthCall& dc,
                                               bool scene_set, int height, const bool guide_present[PROBE_GRID_GUIDES], const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!scene_set) return *why = "srt_set_scene has not been called", RAYS_STATE;
    if (c.row_begin < 0 || c.row_end > height || c.row_begin >= c.row_end) return *why = "bad row band", RAYS_INVALID_ARG;
    if (c.flags & PROBE_GRID_FLAG_VISIBILITY) return *why = "SRT_PROBE_GRID_VISIBILITY: the exact and the filtered test exclude each other", RAYS_INVALID_ARG;
    if (const RaysStatus rs = probe_grid_check_shade(s, c, scene_set, height, guide_present, why)) return rs;
    if (d.moments.count() == 0) return *why = "no depth maps have been written or bound (srt_write_probe_grid_depth, srt_bind_probe_grid_depth)", RAYS_STATE;
    if (d.moments.count() != probe_grid_probes(s.grid)) return *why = "the depth probe count is not nx * ny * nz", RAYS_STATE;
    if (!(dc.bias >= 0.0f) || !isfinite(dc.bias)) return *why = "bias must be finite and >= 0", RAYS_INVALID_ARG;
    if (!(dc.min_variance > 0.0f) || !isfinite(dc.min_variance)) return *why = "min_variance must be finite and > 0", RAYS_INVALID_ARG;
    if (dc.reserved[0] != 0 || dc.reserved[1] != 0) return *why = "reserved must be 0", RAYS_INVALID_ARG;
    return RAYS_OK;
}

}  // namespace srt
