// srt_adaptive_host.h — host-side rules of adaptive sampling (srt_render_adaptive, srt_sample_budget and the sample-count and
// sample-budget buffers) that need no device: argument validation in the header's order, the effective budget of a pixel, what
// the last calls left behind (whether the last adaptive render counted its work, whether a budget pass has run), and the sizes
// of the launch: the grid of persistent workgroups over the band's 8 x 8 tiles and the sample scratch that goes with the grid.
// The two buffers themselves are srt::OutputSlots (srt_outputs_host.h): a buffer is "present" once it has been bound, or its own
// buffer has been written or filled.  Plain C++ without HIP, shared by srt_capi.hip and by tests/native/adaptive_check.cpp, which
// runs it under the address and undefined-behaviour sanitizers on the CPU.
#pragma once

#include <math.h>
#include <stdint.h>

#include "srt_radiance_host.h"

namespace srt {

constexpr uint32_t ADAPTIVE_FLAG_KEEP_COUNTS = 1u, ADAPTIVE_FLAG_COUNT_WORK = 2u, ADAPTIVE_FLAG_ALL = 3u;
constexpr uint32_t ADAPTIVE_MAX_SAMPLES = 4096u;
// the last frame a pixel may hold: srt_render accepts first_sample + sample_count <= 2^31 - 1
constexpr uint32_t ADAPTIVE_FRAME_LIMIT = 2147483646u;
constexpr uint32_t BUDGET_FLAG_ALBEDO = 1u, BUDGET_FLAG_ALL = 1u;
constexpr uint32_t BUDGET_MAX = 4096u;

// the fields of srt_adaptive_params, in its order
struct AdaptiveCall {
    int32_t row_begin, row_end;
    int32_t max_bounces;
    uint32_t seed, max_samples, flags, reserved;
};

// the fields of srt_budget_params, in its order
struct BudgetCall {
    float threshold, floor;
    uint32_t max_budget, flags;
};

// what the last successful calls left behind
struct AdaptiveState {
    CallRecord call;        // the last srt_render_adaptive[_tail]; counted: it had SRT_ADAPTIVE_COUNT_WORK
    bool budgeted = false;  // there has been an srt_sample_budget (srt_get_budget_total)
};

// The band is the caller's.
inline void adaptive_call_default(AdaptiveCall& c) {
    c.row_begin = 0, c.row_end = 0, c.max_bounces = 8, c.seed = 0, c.max_samples = ADAPTIVE_MAX_SAMPLES, c.flags = 0, c.reserved = 0;
}

// Picks, not swept: a relative standard error of 5 %, a floor of a hundredth of white, 64 more samples at most, the demodulated
// variance (srt_variance's default).
inline void budget_call_default(BudgetCall& c) { c.threshold = 0.05f, c.floor = 0.01f, c.max_budget = 64u, c.flags = BUDGET_FLAG_ALBEDO; }

// Rule 1: what a call adds to a pixel that holds n samples and has budget b.
inline uint32_t adaptive_effective(uint32_t b, uint32_t n, uint32_t max_samples) {
    if (n >= ADAPTIVE_FRAME_LIMIT) return 0u;
    const uint32_t room = ADAPTIVE_FRAME_LIMIT - n;
    const uint32_t e = b < max_samples ? b : max_samples;
    return e < room ? e : room;
}

// srt_render_adaptive's checks, in the header's order: scene and camera, the arguments, the two buffers; touches nothing.
inline RaysStatus adaptive_check(const AdaptiveCall& c, bool scene_set, bool camera_set, int height, bool counts_present, bool budget_present,
                                 const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!scene_set) return *why = "srt_set_scene has not been called", RAYS_STATE;
    if (!camera_set) return *why = "srt_set_camera has not been called", RAYS_STATE;
    if (c.row_begin < 0 || c.row_end > height || c.row_begin >= c.row_end) return *why = "bad row band", RAYS_INVALID_ARG;
    if (c.flags & ~ADAPTIVE_FLAG_ALL) return *why = "unknown flags", RAYS_INVALID_ARG;
    if (c.reserved != 0) return *why = "reserved must be 0", RAYS_INVALID_ARG;
    if (c.max_samples < 1 || c.max_samples > ADAPTIVE_MAX_SAMPLES) return *why = "max_samples outside 1 .. 4096", RAYS_INVALID_ARG;
    if (c.max_bounces < 0) return *why = "max_bounces must be >= 0", RAYS_INVALID_ARG;
    if (!counts_present) return *why = "the sample counts have never been written, filled or bound (srt_set_sample_counts)", RAYS_STATE;
    if (!budget_present) return *why = "the sample budget has never been written or bound (srt_sample_budget, srt_write_sample_budget)", RAYS_STATE;
    return RAYS_OK;
}

// srt_sample_budget's checks: the arguments, then the inputs.  var_own: the variance buffer is the handle's own (then
// var_own_albedo says which kind the pass that wrote it made; a bound buffer is the caller's responsibility).
inline RaysStatus budget_check(const BudgetCall& c, bool object_present, bool albedo_present, bool variance_present, bool var_own, bool var_own_albedo,
                               bool counts_present, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (!(c.threshold > 0.0f)) return *why = "threshold must be > 0 (NaN refused)", RAYS_INVALID_ARG;
    if (!(c.floor >= 0.0f)) return *why = "floor must be >= 0 (NaN refused)", RAYS_INVALID_ARG;
    if (c.max_budget < 1 || c.max_budget > BUDGET_MAX) return *why = "max_budget outside 1 .. 4096", RAYS_INVALID_ARG;
    if (c.flags & ~BUDGET_FLAG_ALL) return *why = "unknown flags", RAYS_INVALID_ARG;
    const bool demod = (c.flags & BUDGET_FLAG_ALBEDO) != 0;
    if (!object_present) return *why = "the OBJECT guide has neither been bound nor rendered (srt_render_gbuffer)", RAYS_STATE;
    if (demod && !albedo_present) return *why = "the ALBEDO guide has neither been bound nor rendered (srt_render_gbuffer)", RAYS_STATE;
    if (!variance_present) return *why = "no variance buffer has been bound (srt_bind_variance) or written (srt_variance)", RAYS_STATE;
    if (var_own && var_own_albedo != demod) return *why = "the variance was estimated with the other ALBEDO setting", RAYS_STATE;
    if (!counts_present) return *why = "the sample counts have never been written, filled or bound (srt_set_sample_counts)", RAYS_STATE;
    return RAYS_OK;
}

// Rules 3-4 of srt_sample_budget for one hit pixel with n > 0: the prefiltered variance g, the luminance l.  Binary32, one
// operation per statement: no contraction whatever the compiler's setting.
inline uint32_t budget_value(float g, float l, uint32_t n, const BudgetCall& c) {
    const volatile float sum = l + c.floor;
    const volatile float t = c.threshold * sum;
    const volatile float T = t * t;
    if (!(g > T)) return 0u;
    const volatile float r = g / T;
    const float nf = (float)n;
    const volatile float prod = nf * r;
    const volatile float e = prod - nf;
    if (!(e < (float)c.max_budget)) return c.max_budget;
    const uint32_t b = (uint32_t)ceilf(e);
    return b < 1u ? 1u : b;
}

inline void adaptive_rendered(AdaptiveState& s, uint32_t flags) { s.call.done((flags & ADAPTIVE_FLAG_COUNT_WORK) != 0); }
inline RaysStatus budget_check_total(const AdaptiveState& s) { return s.budgeted ? RAYS_OK : RAYS_STATE; }

// The grid: persistent workgroups of `waves` waves that draw the band's 8 x 8 tiles from a ticket, at most `resident`.
inline unsigned adaptive_grid(int width, int rows, int waves, long long resident) { return persistent_grid(band_tiles(width, rows), waves, resident); }

// The sample scratch of the launch: the radiance kernel's size function (and, in srt_capi.hip, its buffer: both passes run on one stream).
inline size_t adaptive_scratch_bytes(unsigned workgroups, int waves) { return radiance_scratch_bytes(workgroups, waves); }

}  // namespace srt
