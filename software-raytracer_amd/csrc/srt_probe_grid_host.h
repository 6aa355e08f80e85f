// srt_probe_grid_host.h — host-side rules of the probe-grid shading pass (srt_set_probe_grid, srt_write_probe_grid_coefficients,
// srt_bind_probe_grid_coefficients, srt_shade_probe_grid, srt_get_probe_grid_work) that need no device: which grids are accepted,
// which array holds the current coefficients, argument validation in the header's order, and when the work record may be read.
// The two pure-host entries (srt_probe_grid_positions, srt_probe_grid_params_default) are here as well.  Plain C++ without HIP,
// shared by srt_capi.hip and by tests/native/probe_grid_check.cpp, which runs it under the address and undefined-behaviour
// sanitizers on the CPU.
#pragma once

#include <math.h>

#include "srt_light_probes_host.h"

namespace srt {

constexpr uint32_t PROBE_GRID_FLAG_VISIBILITY = 1u, PROBE_GRID_FLAG_NORMAL_WEIGHT = 2u, PROBE_GRID_FLAG_ALBEDO = 4u, PROBE_GRID_FLAG_COUNT_WORK = 8u,
                   PROBE_GRID_FLAG_ALL = 15u;
constexpr int PROBE_GRID_GUIDES = 4;  // OBJECT, NORMAL_DEPTH, POSITION, and ALBEDO with SRT_PROBE_GRID_ALBEDO: the G-buffer slots
constexpr size_t PROBE_GRID_MAX_PROBES = (size_t)1 << 30;

// the fields of srt_probe_grid, in its order
struct ProbeGrid {
    float origin[3], spacing[3];
    int32_t counts[3];
};

// the fields of srt_probe_grid_params, in its order
struct ProbeGridCall {
    int32_t row_begin, row_end;
    uint32_t flags;
    float band_weight[3];
    uint32_t reserved[2];
};

struct ProbeGridState {
    bool grid_set = false;
    ProbeGrid grid{};
    InputArray coefficients;  // counted in probes (nine float4 each)
    CallRecord call;          // the last srt_shade_probe_grid[_depth|_states]; counted: it had SRT_PROBE_GRID_COUNT_WORK
};

inline void probe_grid_call_default(ProbeGridCall& c) {
    c.row_begin = 0, c.row_end = 0, c.flags = 0;
    c.band_weight[0] = 3.14159274f, c.band_weight[1] = 2.09439516f, c.band_weight[2] = 0.785398185f;  // srt_light_probe_irradiance's
    c.reserved[0] = 0, c.reserved[1] = 0;
}

// probes of an accepted grid
inline size_t probe_grid_probes(const ProbeGrid& g) { return (size_t)g.counts[0] * (size_t)g.counts[1] * (size_t)g.counts[2]; }

// srt_set_probe_grid / srt_probe_grid_positions: is this a grid?
inline RaysStatus probe_grid_check(const ProbeGrid& g, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    for (int a = 0; a < 3; ++a)
        if (g.counts[a] < 1) return *why = "counts must be >= 1", RAYS_INVALID_ARG;
    if ((uint64_t)g.counts[0] * (uint64_t)g.counts[1] > PROBE_GRID_MAX_PROBES ||
        (uint64_t)g.counts[0] * (uint64_t)g.counts[1] * (uint64_t)g.counts[2] > PROBE_GRID_MAX_PROBES)
        return *why = "nx * ny * nz exceeds 2^30", RAYS_INVALID_ARG;
    for (int a = 0; a < 3; ++a)
        if (!(g.spacing[a] > 0.0f) || !isfinite(g.spacing[a])) return *why = "spacing must be finite and > 0", RAYS_INVALID_ARG;  // (a NaN fails the comparison)
    for (int a = 0; a < 3; ++a)
        if (!isfinite(g.origin[a])) return *why = "origin must be finite", RAYS_INVALID_ARG;
    return RAYS_OK;
}

// srt_probe_grid_positions: probe (ix, iy, iz) at index ix + nx * (iy + ny * iz); p_a = origin_a + (float)i_a * spacing_a in binary32
// without contraction — the kernel's expression (rule 4), so the positions agree bit for bit.
inline void probe_grid_positions(const ProbeGrid& g, float* dst) {
    size_t k = 0;
    for (int iz = 0; iz < g.counts[2]; ++iz)
        for (int iy = 0; iy < g.counts[1]; ++iy)
            for (int ix = 0; ix < g.counts[0]; ++ix, ++k) {
                volatile float sx = (float)ix * g.spacing[0], sy = (float)iy * g.spacing[1], sz = (float)iz * g.spacing[2];  // (one rounding each: no FMA)
                dst[4 * k + 0] = g.origin[0] + sx, dst[4 * k + 1] = g.origin[1] + sy, dst[4 * k + 2] = g.origin[2] + sz, dst[4 * k + 3] = 0.0f;
            }
}

// srt_shade_probe_grid's checks in the header's order: the scene, the arguments, the inputs; touches nothing.
// guide_present[i]: G-buffer slot i has been bound or rendered.
inline RaysStatus probe_grid_check_shade(const ProbeGridState& s, const ProbeGridCall& c, bool scene_set, int height, const bool guide_present[PROBE_GRID_GUIDES],
                                         const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!scene_set) return *why = "srt_set_scene has not been called", RAYS_STATE;
    if (c.row_begin < 0 || c.row_end > height || c.row_begin >= c.row_end) return *why = "bad row band", RAYS_INVALID_ARG;
    if (c.flags & ~PROBE_GRID_FLAG_ALL) return *why = "unknown flags", RAYS_INVALID_ARG;
    if (c.reserved[0] != 0 || c.reserved[1] != 0) return *why = "reserved must be 0", RAYS_INVALID_ARG;
    for (int b = 0; b < 3; ++b)
        if (c.band_weight[b] != c.band_weight[b]) return *why = "band_weight is NaN", RAYS_INVALID_ARG;
    if (!s.grid_set) return *why = "no grid (srt_set_probe_grid)", RAYS_STATE;
    if (s.coefficients.count() == 0)
        return *why = "no coefficients have been written or bound (srt_write_probe_grid_coefficients, srt_bind_probe_grid_coefficients)", RAYS_STATE;
    static const char* const missing[PROBE_GRID_GUIDES] = {"the OBJECT guide has neither been bound nor rendered (srt_render_gbuffer)",
                                                           "the NORMAL_DEPTH guide has neither been bound nor rendered (srt_render_gbuffer)",
                                                           "the POSITION guide has neither been bound nor rendered (srt_render_gbuffer)",
                                                           "the ALBEDO guide has neither been bound nor rendered (srt_render_gbuffer)"};
    const int guides = (c.flags & PROBE_GRID_FLAG_ALBEDO) ? PROBE_GRID_GUIDES : PROBE_GRID_GUIDES - 1;
    for (int i = 0; i < guides; ++i)
        if (!guide_present[i]) return *why = missing[i], RAYS_STATE;
    if (s.coefficients.count() != probe_grid_probes(s.grid)) return *why = "the coefficient count is not nx * ny * nz", RAYS_STATE;
    return RAYS_OK;
}

// srt_shade_probe_grid once the launch is enqueued
inline void probe_grid_shaded(ProbeGridState& s, uint32_t flags) { s.call.done((flags & PROBE_GRID_FLAG_COUNT_WORK) != 0); }

}  // namespace srt
