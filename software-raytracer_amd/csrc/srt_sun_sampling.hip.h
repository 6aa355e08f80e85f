// srt_sun_sampling.hip.h — gfx950 sun sampling at diffuse bounces (SRT_RADIANCE_SUN_SAMPLING, SRT_LIGHT_PROBE_SUN_SAMPLING; rules
// S1 - S9 of srt_pathtrace.h): at every vertex whose bounce is blind (tt = Smoothness * spec == 0) one shadow segment goes to a
// point of the sun's cap, and that vertex's own bounce sees the environment without the sun.  The path itself — its draws, its
// directions, its GetClosestObject calls — is untouched; only the colour changes.
//
// sun_sample is a phase of a pool step, between the bounce and its closest_hit, called from wave-uniform control flow by all 64
// lanes: the lanes at a diffuse vertex draw their cap point from a stream of their own (S3), the wave makes ONE any_hit call
// for them (srt_occlusion.hip.h: the early out, t_max = +inf) and the open lanes add the sun's colour with the weight that the
// blind bounce's density gives the cap (S6): the blind direction is a normalised point of the cube [-1, 1]^3 folded into the
// hemisphere, density 1 / (12 m^3) per steradian with m = max |component|, not 1 / (2 pi).
//
// LDS: any_hit keeps one word per ray in S.res and its traversal queues in S.meshq — the words closest_hit uses, dead between two
// closest_hit calls.  It touches neither the first-hit records (S.pix) nor the hand-out's match words (S.work, dead outside
// pool_hand_out in any case).  No region of its own is needed.
//
// The frame travels as a kernel argument of its own (SunIO), given only to the SUN kernels: KernelParams has no field for it, and
// the kernels without the flag compile to what they did (the probe tail's scheme).
#pragma once

#include "srt_kernel.hip.h"
#include "srt_occlusion.hip.h"

namespace srt {

// rule S5's frame, made by the host (srt_sun_sampling_host.h: sun_frame): s = -sun_direction, t1, t2
struct SunIO {
    float s[3], t1[3], t2[3];
};

// The sun's share of a diffuse vertex (S3, S4, S6).  `diffuse`: this lane runs a path whose bounce was blind; `key` = the main
// stream after the bounce's three draws (t.rng after pool_bounce); o = p + n * .00001f, the bounce's origin; T the throughput
// the bounce's result will meet.  Returns the any-hit invocations made (0 or 1, wave-uniform).
template <bool MESH, bool SCENE_LDS>
__device__ __forceinline__ unsigned long long sun_sample(const Lds& S, const KernelParams& P, const SunIO& sun, bool diffuse, uint32_t key, V3 o, V3 n, RGB T, RGB& L) {
    const float c = __uint_as_float(0x3F7D70A4u);  // environment()'s threshold
    const float k = 1.0f - c;
    const float W0 = (float)(3.14159265358979323846 / 6.0 * (double)k);
    // S3: a stream of the vertex's own; the main stream is not advanced
    const uint32_t ks = srt_mix32(key ^ 0x53554E21u);
    // S4: the first of eight points of the square that lies in the disc (none: the centre)
    float a = 0.0f, b = 0.0f, q = 0.0f;
    bool undecided = diffuse;
    for (uint32_t J = 0; J < 8u; ++J) {  // (wave-uniform)
        if (__builtin_amdgcn_ballot_w64(undecided) == 0ull) break;
        const uint32_t ra = srt_mix32(ks + (2u * J) * 0x9E3779B9U) >> 17;
        const uint32_t rb = srt_mix32(ks + (2u * J + 1u) * 0x9E3779B9U) >> 17;
        const float aa = (rand_unit(ra) - 0.5f) * 2, bb = (rand_unit(rb) - 0.5f) * 2;
        const float qq = aa * aa + bb * bb;
        const bool take = undecided && qq <= 1.0f;
        if (take) a = aa, b = bb, q = qq;
        undecided = undecided && !take;
    }
    // Lambert's equal-area map of the disc onto the cap: no trigonometry
    const float z = 1 - q * k;
    const float h = sqrt_window(k * (1 + z));  // (k * (1 + z) lies in [0.0199, 0.02]: inside the window, the IEEE root)
    const float ah = a * h, bh = b * h;
    const V3 w0 = v3((sun.t1[0] * ah + sun.t2[0] * bh) + sun.s[0] * z, (sun.t1[1] * ah + sun.t2[1] * bh) + sun.s[1] * z,
                     (sun.t1[2] * ah + sun.t2[2] * bh) + sun.s[2] * z);
    const V3 w = normalized(w0);  // (its window test is wave-level: called by all lanes; the others carry s itself)
    // S6
    const float sd = (w.x * sun.s[0] + w.y * sun.s[1]) + w.z * sun.s[2];
    const float cn = (w.x * n.x + w.y * n.y) + w.z * n.z;
    const bool go = diffuse && sd >= c && cn > 0;
    if (__builtin_amdgcn_ballot_w64(go) == 0ull) return 0ull;
    OccWork<false> no_count;
    const bool occluded = any_hit<MESH, false, SCENE_LDS>(S, P, o, w, __builtin_inff(), go, no_count);
    if (go && !occluded) {
        const float m = fmaxf(fmaxf(fabsf(w.x), fabsf(w.y)), fabsf(w.z));
        const float wt = W0 / ((m * m) * m);
        const float4 e0 = S.c[CONST_ENV_ROW], e1 = S.c[CONST_ENV_ROW + 1], e2 = S.c[CONST_ENV_ROW + 2];  // (.w: the clamped sun colour)
        L = RGB{L.r + ((e0.w * wt) * T.r), L.g + ((e1.w * wt) * T.g), L.b + ((e2.w * wt) * T.b)};
    }
    return 1ull;
}

}  // namespace srt
