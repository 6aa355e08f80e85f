// srt_sun_sampling_host.h — host-side rules of sun sampling (SRT_RADIANCE_SUN_SAMPLING, SRT_LIGHT_PROBE_SUN_SAMPLING; rules S1 - S9
// of srt_pathtrace.h) that need no device: the flag's acceptance in front of the two traces' own parameter checks (which keep
// refusing every bit they do not know, 8 among them), rule S5's frame and its two refusals, the order of the errors, and which
// calls launch a SUN kernel.  Plain C++ without HIP, shared by srt_capi.hip and by tests/native/sun_sampling_check.cpp, which
// runs it under the address and undefined-behaviour sanitizers on the CPU.
#pragma once

#include <math.h>

#include "srt_light_probes_host.h"

namespace srt {

constexpr uint32_t SUN_SAMPLING_FLAG = 16u;  // the bit in srt_radiance_params.flags and srt_light_probe_params.flags

// rule S5's frame as the kernel takes it (srt_sun_sampling.hip.h: SunIO has this layout)
struct SunFrame {
    float s[3], t1[3], t2[3];
};

// Does the call ask for sun sampling / does the launch differ?  With max_bounces == 0 there is no vertex (S1): the call launches
// what it launches without the flag.
inline bool sun_sampling_asked(uint32_t flags) { return (flags & SUN_SAMPLING_FLAG) != 0; }
inline bool sun_sampling_applies(uint32_t flags, int32_t max_bounces) { return sun_sampling_asked(flags) && max_bounces >= 1; }

// The two traces' own checks with the flag taken out: every error of the call itself comes first, in its own order.
inline RaysStatus sun_radiance_check_trace(const RaysState& s, bool scene_set, RadianceCall c, const char** why) {
    c.flags &= ~SUN_SAMPLING_FLAG;
    return radiance_check_trace(s, scene_set, c, why);
}
inline RaysStatus sun_light_probe_check_trace(const LightProbeState& s, bool scene_set, LightProbeCall c, const void* radiance_target, const char** why) {
    c.flags &= ~SUN_SAMPLING_FLAG;
    return light_probe_check_trace(s, scene_set, c, radiance_target, why);
}

// S5: s = sun_direction * -1, e = |s.x| < 0.5f ? (1,0,0) : (0,1,0), t1 = Normalized(cross(e, s)), t2 = cross(s, t1); binary32, one
// operation per expression, the cross products component by component.
inline void sun_frame(const float sun_direction[3], SunFrame& f) {
    const float sx = sun_direction[0] * -1, sy = sun_direction[1] * -1, sz = sun_direction[2] * -1;
    const bool ex = fabsf(sx) < 0.5f;
    const float e0 = ex ? 1.0f : 0.0f, e1 = ex ? 0.0f : 1.0f, e2 = 0.0f;
    const float cx = e1 * sz - e2 * sy, cy = e2 * sx - e0 * sz, cz = e0 * sy - e1 * sx;
    const float len = sqrtf((cx * cx + cy * cy) + cz * cz);
    const float ax = cx / len, ay = cy / len, az = cz / len;
    f.s[0] = sx, f.s[1] = sy, f.s[2] = sz;
    f.t1[0] = ax, f.t1[1] = ay, f.t1[2] = az;
    f.t2[0] = sy * az - sz * ay, f.t2[1] = sz * ax - sx * az, f.t2[2] = sx * ay - sy * ax;
}

// The flag's two refusals, checked after the call's own errors and before anything is touched: a sun direction that is not a
// finite unit vector (to 1e-4 in the squared length), and the probe-tail mode (the combination is not built).
inline RaysStatus sun_sampling_check(const float sun_direction[3], bool probe_tail_enabled, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    const float sx = sun_direction[0] * -1, sy = sun_direction[1] * -1, sz = sun_direction[2] * -1;
    if (!isfinite(sx) || !isfinite(sy) || !isfinite(sz)) return *why = "sun sampling needs a finite sun_direction", RAYS_STATE;
    const float ll = (sx * sx + sy * sy) + sz * sz;
    if (!(ll >= 0.9999f && ll <= 1.0001f)) return *why = "sun sampling needs a unit sun_direction (squared length in [0.9999, 1.0001])", RAYS_STATE;
    if (probe_tail_enabled) return *why = "sun sampling is not available while srt_probe_tail is on", RAYS_STATE;
    return RAYS_OK;
}

}  // namespace srt
