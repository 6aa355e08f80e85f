// srt_mirror_history_host.h — host-side rules of the mirror history (srt_mirror_history, srt_mirror_history_params_default;
// the mode of srt_temporal_accumulate that reprojects through mirror chains) that need no device: parameter validation, the
// rule "toggling drops the history", the angle rho of radius_pixels pixels, and the tag a history pixel carries.  Plain C++
// without HIP, shared by srt_capi.hip and by tests/native/mirror_history_check.cpp, which runs it under the address and
// undefined-behaviour sanitizers on the CPU.
#pragma once

#include <math.h>

#include "srt_rays_host.h"

namespace srt {

constexpr int MIRROR_TAG_SHIFT = 32768;  // tag = J * 32768 + m: object indices are < 32768, J <= 64
constexpr int MIRROR_MAX_BOUNCES = 64;

// the fields of srt_mirror_history_params, in its order
struct MirrorHistoryCall {
    int32_t enabled;
    float radius_pixels;
    uint32_t flags, reserved;
};

// the context's setting: off until the first accepted srt_mirror_history
struct MirrorHistoryState {
    bool enabled = false;
    float radius_pixels = 2.0f;
};

// the defaults of srt_mirror_history_params_default: on, two pixels
inline MirrorHistoryCall mirror_history_defaults() { return MirrorHistoryCall{1, 2.0f, 0u, 0u}; }

// srt_mirror_history's checks; touches nothing.  (The radius test is written so that a NaN fails; +inf passes.)
inline RaysStatus mirror_history_check(const MirrorHistoryCall& m, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (m.enabled < 0 || m.enabled > 1) return *why = "enabled must be 0 or 1", RAYS_INVALID_ARG;
    if (!(m.radius_pixels > 0.0f)) return *why = "radius_pixels must be > 0", RAYS_INVALID_ARG;
    if (m.flags != 0) return *why = "flags must be 0", RAYS_INVALID_ARG;
    if (m.reserved != 0) return *why = "reserved must be 0", RAYS_INVALID_ARG;
    return RAYS_OK;
}

// An accepted call takes effect.  True when the colour and moments histories must be dropped: a history written under one
// mode carries or lacks the tags the other relies on.  A call that only changes the radius keeps them.
inline bool mirror_history_set(MirrorHistoryState& s, const MirrorHistoryCall& m) {
    const bool on = m.enabled != 0;
    const bool drop = on != s.enabled;
    s.enabled = on;
    s.radius_pixels = m.radius_pixels;
    return drop;
}

// rho: the angle of radius_pixels pixels of a frame H rows high, evaluated in double and rounded once
inline float mirror_rho(float radius_pixels, float fov_degrees, int height) {
    return (float)((double)radius_pixels * 2.0 * tan((double)fov_degrees * 3.14159265358979323846 / 360.0) / (double)height);
}

// M1: 0 for a pixel without a mirror in front of it, else the chain length and the FIRST-hit object (the mirror looked through)
inline int32_t mirror_tag(int32_t bounces, int32_t first_object) { return bounces >= 1 ? bounces * MIRROR_TAG_SHIFT + first_object : 0; }
inline int32_t mirror_tag_bounces(int32_t tag) { return tag / MIRROR_TAG_SHIFT; }
inline int32_t mirror_tag_object(int32_t tag) { return tag % MIRROR_TAG_SHIFT; }

}  // namespace srt
