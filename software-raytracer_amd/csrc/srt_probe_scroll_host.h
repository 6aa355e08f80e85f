// srt_probe_scroll_host.h — host-side rules of the scrolling probe grid (srt_probe_scroll_params_default, srt_scroll_probes,
// srt_get_probe_scroll_work, srt_probe_grid_follow) that need no device: the index rule that says which probe of the old grid a
// probe of the moved grid takes its history from (rule SC1), the counts that go with it, the moved origin (rule SC4), the shift
// that re-centres a grid on a point (rule SC7), argument validation in the header's order (rule SC8), and what a scroll makes
// stale (rule SC5).  Plain C++ without HIP, shared by srt_capi.hip and by tests/native/probe_scroll_check.cpp, which sweeps the
// index rule on the CPU.
#pragma once

#include <math.h>

#include "srt_probe_depth_host.h"
#include "srt_probe_update_host.h"

namespace srt {

constexpr uint32_t PROBE_SCROLL_COEFFICIENTS = 1u, PROBE_SCROLL_MOMENTS = 2u, PROBE_SCROLL_STATES = 4u, PROBE_SCROLL_WHICH_ALL = 7u;
constexpr uint32_t PROBE_SCROLL_FLAG_COUNT_WORK = 1u, PROBE_SCROLL_FLAG_SET_GRID = 2u, PROBE_SCROLL_FLAG_ALL = 3u;
constexpr int PROBE_SCROLL_ARRAYS = 3;        // coefficients, moments, records: the bits of `which` in ascending order
constexpr float PROBE_FOLLOW_LIMIT = 1048576.0f;  // rule SC7's clamp, in cells

// the fields of srt_probe_scroll_params, in its order
struct ProbeScrollCall {
    int32_t shift[3];
    uint32_t which, flags, reserved[3];
};

inline void probe_scroll_call_default(ProbeScrollCall& c) {
    c.shift[0] = c.shift[1] = c.shift[2] = 0, c.which = PROBE_SCROLL_COEFFICIENTS, c.flags = 0;
    c.reserved[0] = c.reserved[1] = c.reserved[2] = 0;
}

inline bool probe_scroll_shift_is_zero(const int32_t shift[3]) { return shift[0] == 0 && shift[1] == 0 && shift[2] == 0; }

// Rule SC1 on one axis: the source coordinate j = i + shift in 64 bits; true (and *j) when 0 <= j < n.
inline bool probe_scroll_axis(int64_t i, int32_t shift, int32_t n, int64_t* j) {
    const int64_t v = i + (int64_t)shift;
    if (v < 0 || v >= (int64_t)n) return false;
    *j = v;
    return true;
}

// Rule SC1: destination probe `i` (index ix + nx * (iy + ny * iz)) of an accepted grid.  True, and *source = the index of probe
// j = i + shift, when the probe is retained; false, and *source untouched, when it is exposed.
inline bool probe_scroll_source(const int32_t counts[3], size_t i, const int32_t shift[3], size_t* source) {
    const size_t nx = (size_t)counts[0], ny = (size_t)counts[1];
    const int64_t ic[3] = {(int64_t)(i % nx), (int64_t)((i / nx) % ny), (int64_t)(i / (nx * ny))};
    int64_t j[3];
    for (int a = 0; a < 3; ++a)
        if (!probe_scroll_axis(ic[a], shift[a], counts[a], &j[a])) return false;
    *source = (size_t)j[0] + nx * ((size_t)j[1] + ny * (size_t)j[2]);
    return true;
}

// The retained probes of a scroll: per axis n_a - |shift_a| of them, none when |shift_a| >= n_a.
inline size_t probe_scroll_retained(const int32_t counts[3], const int32_t shift[3]) {
    size_t r = 1;
    for (int a = 0; a < 3; ++a) {
        const int64_t s = shift[a] < 0 ? -(int64_t)shift[a] : (int64_t)shift[a];
        r *= s >= (int64_t)counts[a] ? (size_t)0 : (size_t)((int64_t)counts[a] - s);
    }
    return r;
}

// Rule SC4: origin_a + ((float)shift_a * spacing_a), binary32, product first, no contraction.
inline void probe_scroll_origin(const ProbeGrid& g, const int32_t shift[3], float origin[3]) {
    for (int a = 0; a < 3; ++a) {
        volatile float step = (float)shift[a] * g.spacing[a];  // (one rounding: no FMA)
        origin[a] = g.origin[a] + step;
    }
}

// Rule SC7: the shift that re-centres `g` on `point`; the grid has passed probe_grid_check.
inline void probe_grid_follow(const ProbeGrid& g, const float point[3], int32_t shift[3]) {
    for (int a = 0; a < 3; ++a) {
        volatile float half = ((float)(g.counts[a] - 1)) * 0.5f;
        volatile float reach = half * g.spacing[a];
        volatile float c = g.origin[a] + reach;
        volatile float d = point[a] - c;
        float u = d / g.spacing[a];
        if (u != u) {
            shift[a] = 0;
            continue;
        }
        u = u > PROBE_FOLLOW_LIMIT ? PROBE_FOLLOW_LIMIT : u < -PROBE_FOLLOW_LIMIT ? -PROBE_FOLLOW_LIMIT : u;
        shift[a] = (int32_t)u;  // (truncation towards zero)
    }
}

// srt_scroll_probes' checks in the header's order (rule SC8): the scene, the arguments, the grid and the histories, the records;
// touches nothing.
inline RaysStatus probe_scroll_check(const ProbeGridState& g, const ProbeUpdateState& u, const ProbeStatesState& st, bool scene_set, const ProbeScrollCall& c,
                                     const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!scene_set) return *why = "srt_set_scene has not been called", RAYS_STATE;
    if (c.which == 0 || (c.which & ~PROBE_SCROLL_WHICH_ALL))
        return *why = "which: want a non-empty set of SRT_PROBE_SCROLL_COEFFICIENTS | _MOMENTS | _STATES", RAYS_INVALID_ARG;
    if (c.flags & ~PROBE_SCROLL_FLAG_ALL) return *why = "unknown flags", RAYS_INVALID_ARG;
    if (c.reserved[0] != 0 || c.reserved[1] != 0 || c.reserved[2] != 0) return *why = "reserved must be 0", RAYS_INVALID_ARG;
    if (!g.grid_set) return *why = "no grid (srt_set_probe_grid)", RAYS_STATE;
    if (c.flags & PROBE_SCROLL_FLAG_SET_GRID) {
        float o[3];
        probe_scroll_origin(g.grid, c.shift, o);
        for (int a = 0; a < 3; ++a)
            if (!isfinite(o[a])) return *why = "SRT_PROBE_SCROLL_SET_GRID: the moved origin is not finite", RAYS_INVALID_ARG;
    }
    const size_t P = probe_grid_probes(g.grid);
    static const char* const unset[PROBE_HISTORY_SLOTS] = {"no coefficient history (srt_reset_probe_history)", "no moment history (srt_reset_probe_history)"};
    static const char* const size[PROBE_HISTORY_SLOTS] = {"the coefficient history's probe count is not nx * ny * nz",
                                                          "the moment history's probe count is not nx * ny * nz"};
    for (int i = 0; i < PROBE_HISTORY_SLOTS; ++i) {
        if (!(c.which & (1u << i))) continue;
        if (!u.history[i].reset) return *why = unset[i], RAYS_STATE;
        if (u.history[i].probes != P) return *why = size[i], RAYS_STATE;
    }
    if (c.which & PROBE_SCROLL_STATES) {
        if (st.states.count() == 0) return *why = "no states have been written or bound (srt_write_probe_grid_states, srt_bind_probe_grid_states)", RAYS_STATE;
        if (st.states.count() != P) return *why = "the state count is not nx * ny * nz", RAYS_STATE;
    }
    return RAYS_OK;
}

// Rule SC5: a scroll with a non-zero shift is enqueued — what the last light-probe trace wrote as COEFFICIENTS and the last depth
// trace as MOMENTS is indexed by the old grid, and counts as not written.
inline void probe_scroll_stale(LightProbeState& lp, ProbeDepthState& pd) {
    lp.last.forget(0);  // (light_probe_slot(LIGHT_PROBE_OUT_COEFFICIENTS))
    pd.last.forget(0);  // (probe_depth_slot(PROBE_DEPTH_OUT_MOMENTS))
}

// srt_scroll_probes once the launch is enqueued.  `s`: what srt_get_probe_scroll_work may report.
inline void probe_scroll_scrolled(CallRecord& s, uint32_t flags) { s.done((flags & PROBE_SCROLL_FLAG_COUNT_WORK) != 0); }

// The scroll's grid: one wave per destination probe, persistent workgroups of `waves` waves, at most `resident`.
inline unsigned probe_scroll_grid(size_t probes, int waves, long long resident) { return persistent_grid((long long)probes, waves, resident); }

}  // namespace srt
