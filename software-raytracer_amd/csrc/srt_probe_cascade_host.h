// srt_probe_cascade_host.h — host-side rules of the probe cascade (srt_set_probe_cascade, srt_write_probe_cascade_level,
// srt_bind_probe_cascade_level, srt_capture_probe_cascade_level, srt_shade_probe_cascade, srt_get_probe_cascade_work) that need no
// device: which cascades are accepted and what a refused one leaves, which per-level arrays stay "present" across a new cascade,
// the capture's state checks, argument validation in the header's order, and when the work record may be read.  The three
// pure-host entries (srt_probe_cascade_params_default, srt_probe_cascade_grids, srt_probe_cascade_weights — rule C2, to which the
// kernel and the numpy reference are both held) are here as well.  Plain C++ without HIP, shared by srt_capi.hip and by
// tests/native/probe_cascade_check.cpp, which runs it under the address and undefined-behaviour sanitizers on the CPU.
#pragma once

#include <math.h>

#include "srt_probe_states_host.h"

namespace srt {

constexpr uint32_t PROBE_CASCADE_MAX_LEVELS = 4;
constexpr uint32_t PROBE_CASCADE_FLAG_NORMAL_WEIGHT = 1u, PROBE_CASCADE_FLAG_DEPTH = 2u, PROBE_CASCADE_FLAG_STATES = 4u, PROBE_CASCADE_FLAG_ALBEDO = 8u,
                   PROBE_CASCADE_FLAG_COUNT_WORK = 16u, PROBE_CASCADE_FLAG_ALL = 31u;
constexpr uint32_t PROBE_CASCADE_COEFFICIENTS = 1u, PROBE_CASCADE_MOMENTS = 2u, PROBE_CASCADE_RECORDS = 4u, PROBE_CASCADE_WHICH_ALL = 7u;
constexpr int PROBE_CASCADE_ARRAYS = 3;  // per level: coefficients, moments, records

// the fields of srt_probe_cascade, in its order
struct ProbeCascade {
    uint32_t levels, resolution;
    float blend_cells;
    uint32_t reserved;
    ProbeGrid grid[PROBE_CASCADE_MAX_LEVELS];
};

// the fields of srt_probe_cascade_params, in its order
struct ProbeCascadeCall {
    int32_t row_begin, row_end;
    uint32_t flags;
    float band_weight[3];
    float bias, min_variance;
    uint32_t reserved[2];
};

struct ProbeCascadeState {
    bool set = false;
    ProbeCascade cascade{};
    InputArray arrays[PROBE_CASCADE_MAX_LEVELS][PROBE_CASCADE_ARRAYS];  // counted in probes
    CallRecord call;  // the last srt_shade_probe_cascade; counted: it had SRT_PROBE_CASCADE_COUNT_WORK
};

inline void probe_cascade_call_default(ProbeCascadeCall& c) {
    ProbeGridCall g;
    probe_grid_call_default(g);
    ProbeGridDepthCall d;
    probe_grid_depth_call_default(d);
    c.row_begin = 0, c.row_end = 0, c.flags = 0;
    for (int b = 0; b < 3; ++b) c.band_weight[b] = g.band_weight[b];
    c.bias = d.bias, c.min_variance = d.min_variance;
    c.reserved[0] = 0, c.reserved[1] = 0;
}

// slot of a single `which` bit, -1 for anything else
inline int probe_cascade_slot(uint32_t which) {
    return which == PROBE_CASCADE_COEFFICIENTS ? 0 : which == PROBE_CASCADE_MOMENTS ? 1 : which == PROBE_CASCADE_RECORDS ? 2 : -1;
}
// bytes of one probe of array `slot` in a cascade of moment resolution R (0 for the moments of a cascade without any)
inline size_t probe_cascade_probe_bytes(int slot, uint32_t resolution) {
    return (slot == 0 ? (size_t)LIGHT_PROBE_COEFFS : slot == 1 ? (size_t)resolution * resolution : (size_t)1) * (4 * sizeof(float));
}

// srt_set_probe_cascade: is this a cascade?
inline RaysStatus probe_cascade_check(const ProbeCascade& c, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (c.levels < 1 || c.levels > PROBE_CASCADE_MAX_LEVELS) return *why = "levels outside 1 .. 4", RAYS_INVALID_ARG;
    if (c.resolution != 0 && !probe_depth_resolution_ok(c.resolution)) return *why = "resolution: want 0, 4, 8 or 16", RAYS_INVALID_ARG;
    if (!(c.blend_cells > 0.0f) || !isfinite(c.blend_cells)) return *why = "blend_cells must be finite and > 0", RAYS_INVALID_ARG;  // (a NaN fails the comparison)
    if (c.reserved != 0) return *why = "reserved must be 0", RAYS_INVALID_ARG;
    for (uint32_t l = 0; l < c.levels; ++l)
        if (const RaysStatus rs = probe_grid_check(c.grid[l], why)) return rs;
    return RAYS_OK;
}

// srt_set_probe_cascade: a refused cascade leaves the previous one and every mark.  An accepted one is copied; a level whose probe
// count changed (or that did not exist, or no longer does) loses the "present" marks of its arrays, own and bound; a level whose
// origin or spacing alone changed keeps them — the scroll case.  A changed resolution takes every level's moments.
inline RaysStatus probe_cascade_set(ProbeCascadeState& s, const ProbeCascade& c, const char** why) {
    if (const RaysStatus rs = probe_cascade_check(c, why)) return rs;
    for (uint32_t l = 0; l < PROBE_CASCADE_MAX_LEVELS; ++l) {
        const bool was = s.set && l < s.cascade.levels, is = l < c.levels;
        const bool same = was && is && probe_grid_probes(s.cascade.grid[l]) == probe_grid_probes(c.grid[l]);
        for (int i = 0; i < PROBE_CASCADE_ARRAYS; ++i)
            if (!same || (i == 1 && s.cascade.resolution != c.resolution)) s.arrays[l][i] = InputArray{};
    }
    s.cascade = c, s.set = true;
    for (uint32_t l = c.levels; l < PROBE_CASCADE_MAX_LEVELS; ++l) s.cascade.grid[l] = ProbeGrid{};  // (entries >= levels are ignored)
    return RAYS_OK;
}

// srt_write_probe_cascade_level / srt_bind_probe_cascade_level: the slot of (level, which), or why not; `probes` as the caller
// gave it (a bind's NULL, 0 is the caller's to recognise first).  Touches nothing.
inline RaysStatus probe_cascade_check_level_array(const ProbeCascadeState& s, uint32_t level, uint32_t which, size_t probes, int* slot, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!s.set) return *why = "no cascade (srt_set_probe_cascade)", RAYS_STATE;
    if (level >= s.cascade.levels) return *why = "level is not below the cascade's levels", RAYS_INVALID_ARG;
    const int i = probe_cascade_slot(which);
    if (i < 0) return *why = "which: want exactly one of SRT_PROBE_CASCADE_COEFFICIENTS, _MOMENTS, _RECORDS", RAYS_INVALID_ARG;
    if (i == 1 && s.cascade.resolution == 0) return *why = "SRT_PROBE_CASCADE_MOMENTS: the cascade's resolution is 0", RAYS_INVALID_ARG;
    if (probes < 1 || probes > PROBE_GRID_MAX_PROBES) return *why = "probes: want 1 .. 2^30", RAYS_INVALID_ARG;
    if (i == 1 && probes * (size_t)s.cascade.resolution * s.cascade.resolution > PROBE_DEPTH_MAX_ELEMS) return *why = "probes x resolution^2 exceeds 2^30", RAYS_INVALID_ARG;
    *slot = i;
    return RAYS_OK;
}

// srt_capture_probe_cascade_level's checks; touches nothing.  The sources are the single grid's current arrays.
inline RaysStatus probe_cascade_check_capture(const ProbeCascadeState& s, uint32_t level, uint32_t which_mask, const ProbeGridState& g, const ProbeGridDepthState& d,
                                              const ProbeStatesState& st, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!s.set) return *why = "no cascade (srt_set_probe_cascade)", RAYS_STATE;
    if (level >= s.cascade.levels) return *why = "level is not below the cascade's levels", RAYS_INVALID_ARG;
    if (which_mask == 0 || (which_mask & ~PROBE_CASCADE_WHICH_ALL))
        return *why = "which: want a non-empty set of SRT_PROBE_CASCADE_COEFFICIENTS | _MOMENTS | _RECORDS", RAYS_INVALID_ARG;
    if (!g.grid_set) return *why = "no grid (srt_set_probe_grid)", RAYS_STATE;
    const ProbeGrid& lg = s.cascade.grid[level];
    for (int a = 0; a < 3; ++a)
        if (g.grid.counts[a] != lg.counts[a]) return *why = "the current grid's counts are not the level's", RAYS_STATE;
    const size_t P = probe_grid_probes(lg);
    if (which_mask & PROBE_CASCADE_COEFFICIENTS) {
        if (g.coefficients.count() == 0) return *why = "no current probe-grid coefficients", RAYS_STATE;
        if (g.coefficients.count() != P) return *why = "the current coefficient count is not the level's nx * ny * nz", RAYS_STATE;
    }
    if (which_mask & PROBE_CASCADE_MOMENTS) {
        if (d.moments.count() == 0) return *why = "no current probe-grid depth maps", RAYS_STATE;
        if (d.moments.count() != P) return *why = "the current depth probe count is not the level's nx * ny * nz", RAYS_STATE;
        if (d.resolution() != s.cascade.resolution) return *why = "the current depth maps' resolution is not the cascade's", RAYS_STATE;
    }
    if (which_mask & PROBE_CASCADE_RECORDS) {
        if (st.states.count() == 0) return *why = "no current probe-grid states", RAYS_STATE;
        if (st.states.count() != P) return *why = "the current state count is not the level's nx * ny * nz", RAYS_STATE;
    }
    return RAYS_OK;
}

// srt_shade_probe_cascade's checks in the header's order (rule C7); touches nothing.
inline RaysStatus probe_cascade_check_shade(const ProbeCascadeState& s, const ProbeCascadeCall& c, bool scene_set, int height,
                                            const bool guide_present[PROBE_GRID_GUIDES], const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!scene_set) return *why = "srt_set_scene has not been called", RAYS_STATE;
    if (c.row_begin < 0 || c.row_end > height || c.row_begin >= c.row_end) return *why = "bad row band", RAYS_INVALID_ARG;
    if (c.flags & ~PROBE_CASCADE_FLAG_ALL) return *why = "unknown flags", RAYS_INVALID_ARG;
    if (c.reserved[0] != 0 || c.reserved[1] != 0) return *why = "reserved must be 0", RAYS_INVALID_ARG;
    for (int b = 0; b < 3; ++b)
        if (c.band_weight[b] != c.band_weight[b]) return *why = "band_weight is NaN", RAYS_INVALID_ARG;
    if (c.flags & PROBE_CASCADE_FLAG_DEPTH) {
        if (!(c.bias >= 0.0f)) return *why = "bias must be >= 0", RAYS_INVALID_ARG;  // (a NaN fails the comparison)
        if (!(c.min_variance >= 0.0f)) return *why = "min_variance must be >= 0", RAYS_INVALID_ARG;
    }
    if (!s.set) return *why = "no cascade (srt_set_probe_cascade)", RAYS_STATE;
    static const char* const missing[PROBE_GRID_GUIDES] = {"the OBJECT guide has neither been bound nor rendered (srt_render_gbuffer)",
                                                           "the NORMAL_DEPTH guide has neither been bound nor rendered (srt_render_gbuffer)",
                                                           "the POSITION guide has neither been bound nor rendered (srt_render_gbuffer)",
                                                           "the ALBEDO guide has neither been bound nor rendered (srt_render_gbuffer)"};
    const int guides = (c.flags & PROBE_CASCADE_FLAG_ALBEDO) ? PROBE_GRID_GUIDES : PROBE_GRID_GUIDES - 1;
    for (int i = 0; i < guides; ++i)
        if (!guide_present[i]) return *why = missing[i], RAYS_STATE;
    for (uint32_t l = 0; l < s.cascade.levels; ++l) {
        const size_t P = probe_grid_probes(s.cascade.grid[l]);
        if (s.arrays[l][0].count() == 0) return *why = "a level has no coefficients (srt_write_ / srt_bind_ / srt_capture_probe_cascade_level)", RAYS_STATE;
        if (s.arrays[l][0].count() != P) return *why = "a level's coefficient count is not its nx * ny * nz", RAYS_STATE;
        if (c.flags & PROBE_CASCADE_FLAG_DEPTH) {
            if (s.cascade.resolution == 0) return *why = "SRT_PROBE_CASCADE_DEPTH: the cascade's resolution is 0", RAYS_STATE;
            if (s.arrays[l][1].count() == 0) return *why = "a level has no moments (srt_write_ / srt_bind_ / srt_capture_probe_cascade_level)", RAYS_STATE;
            if (s.arrays[l][1].count() != P) return *why = "a level's moment probe count is not its nx * ny * nz", RAYS_STATE;
        }
        if (c.flags & PROBE_CASCADE_FLAG_STATES) {
            if (s.arrays[l][2].count() == 0) return *why = "a level has no records (srt_write_ / srt_bind_ / srt_capture_probe_cascade_level)", RAYS_STATE;
            if (s.arrays[l][2].count() != P) return *why = "a level's record count is not its nx * ny * nz", RAYS_STATE;
        }
    }
    return RAYS_OK;
}

// srt_shade_probe_cascade once the launch is enqueued
inline void probe_cascade_shaded(ProbeCascadeState& s, uint32_t flags) { s.call.done((flags & PROBE_CASCADE_FLAG_COUNT_WORK) != 0); }

// srt_probe_cascade_grids: level l has the given counts and spacing_a = ldexpf(base_spacing_a, l); its origin is snapped to whole
// cells of its own spacing: k = floorf(centre_a / spacing_a), clamped to +-1048576, a NaN gives 0;
// origin_a = (k - (float)((n_a - 1) / 2)) * spacing_a (integer division).  Binary32, one rounding per operation.  Refuses what
// srt_set_probe_cascade would refuse, and then leaves *out alone.
inline RaysStatus probe_cascade_grids(const float centre[3], const float base_spacing[3], const int32_t counts[3], uint32_t levels, ProbeCascade& out) {
    ProbeCascade c{};
    c.levels = levels, c.resolution = 0, c.blend_cells = 1.0f, c.reserved = 0;
    if (levels < 1 || levels > PROBE_CASCADE_MAX_LEVELS) return RAYS_INVALID_ARG;
    for (uint32_t l = 0; l < levels; ++l)
        for (int a = 0; a < 3; ++a) {
            const float sp = ldexpf(base_spacing[a], (int)l);
            volatile float q = centre[a] / sp;  // (one rounding each)
            float k = floorf(q);
            k = !(k == k) ? 0.0f : (k > 1048576.0f ? 1048576.0f : (k < -1048576.0f ? -1048576.0f : k));
            volatile float b = k - (float)((counts[a] - 1) / 2);
            c.grid[l].spacing[a] = sp, c.grid[l].counts[a] = counts[a];
            c.grid[l].origin[a] = b * sp;
        }
    if (probe_cascade_check(c, nullptr) != RAYS_OK) return RAYS_INVALID_ARG;
    out = c;
    return RAYS_OK;
}

// Rule C2 for one level: beta_l(x)
inline float probe_cascade_level_weight(const ProbeGrid& g, float blend_cells, const float x[3]) {
    float e = INFINITY;
    for (int a = 0; a < 3; ++a) {
        if (g.counts[a] < 2) continue;
        volatile float r = x[a] - g.origin[a];
        const float u = r / g.spacing[a], m = (float)(g.counts[a] - 1);  // rule 2's expression before its clamp
        if (!(u >= 0.0f && u <= m)) return 0.0f;                         // (a NaN, a point outside)
        const float gg = m - u, ea = u < gg ? u : gg;
        e = ea < e ? ea : e;
    }
    return e >= blend_cells ? 1.0f : e / blend_cells;
}

// srt_probe_cascade_weights: rule C2 for one point.  first_level f: the lowest level with beta > 0, else levels - 1.
// evaluations: 1 (level f alone) or 2 (f with weight beta and f + 1 with 1.0f - beta).  beta: beta_f as rule C2 gives it (1.0f
// inside the band's inner edge, 0.0f for a point no level holds).
inline void probe_cascade_weights(const ProbeCascade& c, const float x[3], int32_t* first_level, int32_t* evaluations, float* beta) {
    int f = -1;
    float bf = 0.0f;
    for (uint32_t l = 0; l < c.levels && f < 0; ++l) {
        const float b = probe_cascade_level_weight(c.grid[l], c.blend_cells, x);
        if (b > 0.0f) f = (int)l, bf = b;
    }
    if (f < 0) f = (int)c.levels - 1, bf = probe_cascade_level_weight(c.grid[f], c.blend_cells, x);
    *first_level = f, *evaluations = (f == (int)c.levels - 1 || bf >= 1.0f) ? 1 : 2, *beta = bf;
}

}  // namespace srt
