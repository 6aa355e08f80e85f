// srt_radiance.hip.h — gfx950 path-traced radiance for caller-supplied rays (srt_trace_radiance): for ray i of a batch and the
// samples f = f0 .. f0 + n - 1, colour_f = RaytraceScene(origin[i], direction[i]) (the path branch, Raytracer.cpp:141-146,
// 162-185, 212) drawn from the stream srt_rng_key(seed, id_base + i, f), folded in ascending f into SetScreenPixel's running mean
// (:63-71) of output element i.  What srt_render computes for a pixel, without the camera, the pixel grid and the framebuffer: a
// batch of camera rays in pixel order gives the accumulator's bits.
//
// Launched, sized and staged exactly like rays_kernel (persistent workgroups, make_lds with four waves, each wave strides over
// blocks of 64 consecutive rays, lane l owns ray 64 * block + l, 16-byte ray loads).  Per block:
//   1. ONE closest_hit for the block's 64 primary rays: there is no jitter, every sample of a ray shares its first hit.  A ray
//      that misses, or any ray when max_bounces == 0, has a colour that does not depend on the sample; its lane folds that colour
//      n times and is done.
//   2. The other lanes leave a record (direction, first hit, the seed-and-id half of the RNG key) in slot l of the wave's LDS
//      records and become the slot's owner.  The wave then runs pathtrace_kernel's path pool over (slot, sample) tasks: every
//      step the free lanes take tasks from the slots that have samples left — the slots are dealt to the free lanes round-robin, so
//      a slot hands out as many consecutive samples in one step as it is dealt lanes (one ray x 64 samples fills the wave) — and
//      all 64 lanes go through one closest_hit; idle lanes ride along through its wave-uniform rounds.  One bounce is restated
//      here from pathtrace_kernel (which stays as it is), expression by expression: the same bits.
//   3. A finished sample's colour (r, g, b, alpha tag) goes to row (sample - chunk start), slot, of the wave's OWN region of a
//      scratch buffer in global memory: RAD_CHUNK rows of 64 float4.  When the pool has drained, the owner lanes fold their slot's
//      rows in sample order — the ROWS kernel's scheme with its workgroup-scope release / acquire pair in front of the read-back.
//      A batch with more than RAD_CHUNK samples runs chunk after chunk on the same wave, folding in between; the running mean
//      stays in the owner's registers.  The scratch is sized by the grid (waves x RAD_CHUNK x 64 x 16 B), never by N x n.
// The fold order per ray is fixed (ascending f) whatever the packing does, no atomics reach the output: repeated calls give the
// same bits.  Mesh scenes pass defer_min = 1 as rays_kernel does: every call resolves its mesh rays itself, nothing is parked.
// Work counts (COUNT instantiations only): wave-uniform 64-bit sums, added to a handle-owned record with ONE vector atomic per
// wave at the end.  Without COUNT there is no atomic.
#pragma once

#include "srt_kernel.hip.h"

namespace srt {

enum { RAD_WORK_RAYS = 0, RAD_WORK_SAMPLES, RAD_WORK_CLOSEST, RAD_WORK_WAVE_CALLS, RAD_WORK_N };

// samples per chunk: rows of the wave's scratch region (srt_radiance_host.h: RADIANCE_CHUNK; srt_capi.hip asserts that they agree)
constexpr int RAD_CHUNK = 64;

struct RadianceIO {
    const float4* origin;      // (o.xyz, ignored)
    const float4* direction;   // (d.xyz, ignored)
    uint32_t count;            // rays, 1 .. 2^30
    uint32_t normalize;        // SRT_RADIANCE_NORMALIZE: d = float3::Normalized(d) first
    uint32_t id_base;          // ray i draws from the stream of "pixel" id_base + i (mod 2^32)
    uint32_t reserved;
    float4* out;               // [count] the running means
    float4* rows;              // [grid waves][RAD_CHUNK][64] sample colours of the chunk in flight
    unsigned long long* work;  // COUNT: [RAD_WORK_N] totals of the launch (zeroed by the host before it)
};
// (the sample range, bounces, seed and SRT_RADIANCE_RESET travel in KernelParams: first_sample, sample_count, max_bounces, seed,
// flags & 1 — the fields accumulate_sample reads)

// per-wave work counts: wave-uniform 64-bit sums
template <bool ON>
struct RadWork {
    __device__ __forceinline__ void add(int, unsigned long long) {}
};
template <>
struct RadWork<true> {
    unsigned long long n[RAD_WORK_N] = {0ull, 0ull, 0ull, 0ull};
    __device__ __forceinline__ void add(int i, unsigned long long v) { n[i] += v; }
};

// LDS: the path-trace kernel's layout (make_lds with four waves), as rays_kernel.
template <bool SCENE_LDS, bool MESH, bool COUNT>
__global__ void __launch_bounds__(WG_THREADS) radiance_kernel(const KernelParams P, const RadianceIO io) {
    extern __shared__ float4 lds_scene[];
    if constexpr (SCENE_LDS) {  // staged as pathtrace_kernel stages it: every load issued before the first LDS store
        constexpr int STAGE = 8;
        const int n = P.scene_vec4;
        float4 row[STAGE];
#pragma unroll
        for (int k = 0; k < STAGE; ++k) {
            const int i = (int)threadIdx.x + k * WG_THREADS;
            row[k] = i < n ? P.scene[i] : make_float4(0, 0, 0, 0);
        }
#pragma unroll
        for (int k = 0; k < STAGE; ++k) {
            const int i = (int)threadIdx.x + k * WG_THREADS;
            if (i < n) lds_scene[i] = row[k];
        }
        for (int i = (int)threadIdx.x + STAGE * WG_THREADS; i < n; i += WG_THREADS) lds_scene[i] = P.scene[i];
        __syncthreads();
    }
    constexpr int WAVES = WG_TILES_X * WG_TILES_Y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Lds S = make_lds<SCENE_LDS>(P, lds_scene, WAVES, wave);
#if defined(SRT_STATS) && SRT_STATS == 3
    Prof prof{};
#endif
    Tally<false> no_tally;
    RadWork<COUNT> W;
    auto lanes = [](bool b) { return (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(b)); };
    auto below = [](unsigned long long m) { return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)); };
    // this wave's region of the scratch: RAD_CHUNK rows of 64 slots
    float4* const rows = io.rows + ((size_t)blockIdx.x * WAVES + (size_t)wave) * (size_t)(RAD_CHUNK * 64);
    float* const rec = S.pix;                                      // [64][12]: dir, n0, p0, prim0, the key's seed-and-id half
    unsigned* const match = reinterpret_cast<unsigned*>(S.work);  // [64] of (sample << 6 | slot), ~0 = nothing
    const uint32_t n = P.sample_count;
    const int B = P.max_bounces;
    const bool reset = (P.flags & 1u) != 0;
    const uint32_t blocks = (io.count + 63u) >> 6;  // count <= 2^30: at most 2^24 blocks
    const bool norm = io.normalize != 0u;           // (a kernel argument: wave-uniform)
    // wave-uniform loop: every lane of a wave runs the same trips, so closest_hit sees all 64 lanes in each call
    for (uint32_t b = blockIdx.x * (uint32_t)WAVES + (uint32_t)wave; b < blocks; b += gridDim.x * (uint32_t)WAVES) {
        const uint32_t i = (b << 6) + (uint32_t)lane;
        const bool active = i < io.count;
        // lanes past the batch load nothing: they carry a harmless unit ray through the primary call and own no slot
        float4 o4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), d4 = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
        if (active) o4 = io.origin[i], d4 = io.direction[i];  // 16-byte loads
        V3 dir0 = v3(d4.x, d4.y, d4.z);
        if (norm) dir0 = normalized(dir0);  // float3::Normalized (Common.hpp:159-162); its window test is wave-level: called by all lanes
        bool deferred = false;              // (defer_min = 1: every call resolves its mesh rays itself)
        // ---- primary hit: identical for every sample (Raytracer.cpp:142)
        const Hit h0 = closest_hit<MESH, false, SCENE_LDS>(S, P, v3(o4.x, o4.y, o4.z), dir0, active, 1, deferred, no_tally SRT_PROF_ARG);
        const bool traced = active && h0.prim >= 0 && B > 0;
        W.add(RAD_WORK_WAVE_CALLS, 1ull);
        W.add(RAD_WORK_RAYS, lanes(active));
        W.add(RAD_WORK_SAMPLES, lanes(active) * n);
        W.add(RAD_WORK_CLOSEST, lanes(active && !traced) * n);  // the primary counts once per sample (srt_stats.rays' rule)
        float4 acc = make_float4(0, 0, 0, 0);
        if (active && !reset) acc = io.out[i];
        // ---- rays whose colour does not depend on the sample: a miss -> env(d) every sample (:143-145); MAXBOUNCES == 0 ->
        // the first hit's EmissiveColor (:162, 212)
        if (active && !traced) {
            RGB c;
            float ca = 0.0f;  // the colour's alpha (+0 from the emissive colour)
            if (h0.prim < 0) {
                c = environment(S, dir0);
                ca = environment_alpha(dir0);
            } else {
                const float4 m1 = S.mat(h0.prim, 1);
                c = RGB{clamp0(m1.y), clamp0(m1.z), clamp0(m1.w)};
            }
            for (uint32_t s = 0; s < n; ++s) accumulate_sample(P, acc, c, ca, s);
            io.out[i] = acc;
        }
        if (__builtin_amdgcn_ballot_w64(traced) == 0ull) continue;

        // ---- wave-level path pool over (slot, sample): lane l owns slot l
        if (traced) {
            float* r = rec + lane * 12;
            r[0] = dir0.x, r[1] = dir0.y, r[2] = dir0.z;
            r[3] = h0.n.x, r[4] = h0.n.y, r[5] = h0.n.z;
            r[6] = h0.p.x, r[7] = h0.p.y, r[8] = h0.p.z;
            r[9] = __int_as_float(h0.prim);
            // srt_rng_key's first two rounds depend on seed and id only: done here once, the sample's round at the hand-out
            r[10] = __uint_as_float(srt_mix32(srt_mix32(P.seed ^ 0xA511E9B3U) + (io.id_base + i)));
        }
        __builtin_amdgcn_wave_barrier();
        // path state of the task this lane is running
        bool busy = false;
        uint32_t task = 0;  // sample << 6 | slot
        RGB L{0, 0, 0}, T{0, 0, 0};
        V3 sray = v3(0, 0, 1), hn = v3(0, 0, 0), hp = v3(0, 0, 0);
        int hprim = 0, bounce = 0;
        float spec = 0.0f;
        uint32_t rng = 0;
        int rot = 0;  // wave-uniform rotation of the slot priority
        for (uint32_t c0 = 0; c0 < n; c0 += (uint32_t)RAD_CHUNK) {  // (wave-uniform)
            const uint32_t end = n - c0 < (uint32_t)RAD_CHUNK ? n : c0 + (uint32_t)RAD_CHUNK;
            uint32_t own_next = traced ? c0 : end;  // samples [c0, own_next) of this slot have been handed out
            // the fold of the chunk before has read the rows this chunk's paths overwrite
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            while (__builtin_amdgcn_ballot_w64(busy || own_next < end) != 0ull) {
                // ---- hand out tasks: the slots that have samples left are dealt round-robin to the free lanes, and a slot hands
                // out as many consecutive samples as it is dealt lanes, up to what it has left (pathtrace_kernel's MULTI hand-out).
                // Two passes: entries that stayed empty in the first because a slot ran out find another slot in the second.
                bool fresh = false;
                for (int pass = 0; pass < 2; ++pass) {
                    const unsigned long long freem = __builtin_amdgcn_ballot_w64(!busy);
                    const int avail = own_next < end ? (int)(end - own_next) : 0;
                    const bool can = avail > 0;
                    const unsigned long long canm = __builtin_amdgcn_ballot_w64(can);
                    if (freem == 0ull || canm == 0ull) break;
                    const int nfree = __builtin_popcountll(freem), ncan = __builtin_popcountll(canm);
                    // the slot priority rotates so that all slots advance at the same pace: rank among the slots that can,
                    // counted cyclically from lane `rot`
                    rot = (rot + 23) & 63;
                    const int crank = below(canm) - __builtin_popcountll(canm & ((1ull << rot) - 1ull)) + (lane < rot ? ncan : 0);
                    const int frank = below(freem);
                    if (!busy) match[frank] = 0xFFFFFFFFu;
                    __builtin_amdgcn_wave_barrier();
                    if (can) {
                        int given = 0;
                        for (int j = crank; j < nfree && given < avail; j += ncan) {
                            match[j] = ((own_next + (uint32_t)given) << 6) | (unsigned)lane;
                            ++given;
                        }
                        own_next += (uint32_t)given;
                    }
                    __builtin_amdgcn_wave_barrier();
                    const unsigned m = !busy ? match[frank] : 0xFFFFFFFFu;
                    if (m != 0xFFFFFFFFu) {  // (the sample is set up below, once for the lanes of both passes)
                        task = m;
                        busy = true;
                        fresh = true;
                    }
                    __builtin_amdgcn_wave_barrier();
                }
                if (fresh) {  // a lane that has just taken a task: Raytracer.cpp:162-166 for sample sidx of that ray
                    const uint32_t sidx = task >> 6;
                    const float* r = rec + (int)(task & 63u) * 12;
                    const int prim0 = __float_as_int(r[9]);
                    rng = srt_mix32(__float_as_uint(r[10]) + (P.first_sample + sidx));  // = srt_rng_key(seed, id, sample), see the record
                    const uint32_t rr = srt_mix32(rng) >> 17;                            // draw 0: the specular lottery at the first hit
                    rng += 0x9E3779B9U;
                    const float4 m0 = S.mat(prim0, 0), m1 = S.mat(prim0, 1);
                    spec = (m0.y >= rand_unit(rr)) ? 1.0f : 0.0f;  // :165
                    L = RGB{m1.y, m1.z, m1.w};                     // :162 (clamped in the image)
                    T = RGB{m0.z, m0.w, m1.x};                     // :163
                    sray = v3(r[0], r[1], r[2]);                   // :164
                    hn = v3(r[3], r[4], r[5]);
                    hp = v3(r[6], r[7], r[8]);
                    hprim = prim0;
                    bounce = 0;
                }
                W.add(RAD_WORK_CLOSEST, lanes(fresh));  // the sample's primary GetClosestObject call (:142)
                // ---- one bounce for every busy lane
                V3 o = v3(0, 0, 0);
                const float ofs = .00001f;
                if (busy) {
                    if (bounce != 0) {  // :169-171
                        T = RGB{T.r * 0.8f, T.g * 0.8f, T.b * 0.8f};  // (NN)
                    }
                    // reflectedRay = sray.Reflect(normal)  (:172, Common.hpp:163-165)
                    const float k2 = 2 * dot3(sray, hn);
                    const V3 refl = v3(sray.x - hn.x * k2, sray.y - hn.y * k2, sray.z - hn.z * k2);
                    // GetRandomNormalOrientedHemisphere (:90-105): exactly three draws, x then y then z
                    const uint32_t r0 = srt_mix32(rng) >> 17;
                    const uint32_t r1 = srt_mix32(rng + 0x9E3779B9U) >> 17;
                    const uint32_t r2 = srt_mix32(rng + 2u * 0x9E3779B9U) >> 17;
                    rng += 3u * 0x9E3779B9U;
                    V3 sr = v3((rand_unit(r0) - 0.5f) * 2, (rand_unit(r1) - 0.5f) * 2, (rand_unit(r2) - 0.5f) * 2);
                    sr = normalized_in_window(sr);  // (inside normalized()'s window by construction: see there)
                    if (dot3(sr, hn) < 0) sr = v3(sr.x * -1, sr.y * -1, sr.z * -1);
                    // float3::Lerp(sray, reflectedRay, Smoothness * specularProb)  (:175)
                    const float tt = S.mat(hprim, 0).x * spec;
                    const V3 l = v3(sr.x * (1 - tt) + refl.x * tt, sr.y * (1 - tt) + refl.y * tt, sr.z * (1 - tt) + refl.z * tt);
                    sray = normalized(l);                                            // :176
                    o = v3(hp.x + hn.x * ofs, hp.y + hn.y * ofs, hp.z + hn.z * ofs);  // :177
                }
                // the scan runs in wave-uniform control flow: idle lanes help with other lanes' rays
                const Hit h = closest_hit<MESH, false, SCENE_LDS>(S, P, o, sray, busy, 1, deferred, no_tally SRT_PROF_ARG);
                W.add(RAD_WORK_WAVE_CALLS, 1ull);
                W.add(RAD_WORK_CLOSEST, lanes(busy));
                if (busy) {
                    bool end_path;
                    uint32_t atag = 0u;  // the sample's alpha: NaN only from the environment (T's alpha is +0)
                    if (h.prim < 0) {    // :178-181
                        const RGB e = environment(S, sray);
                        L = RGB{L.r + e.r * T.r, L.g + e.g * T.g, L.b + e.b * T.b};  // (NN)
                        atag = alpha_tag(environment_alpha(sray));
                        end_path = true;
                    } else {
                        const float4 m0 = S.mat(h.prim, 0), m1 = S.mat(h.prim, 1), m2 = S.mat(h.prim, 2);
                        const uint32_t r = srt_mix32(rng) >> 17;  // one lottery per further hit
                        rng += 0x9E3779B9U;
                        spec = (m0.y >= rand_unit(r)) ? 1.0f : 0.0f;  // :182
                        const RGB Em{m1.y, m1.z, m1.w};
                        L = RGB{L.r + Em.r * T.r, L.g + Em.g * T.g, L.b + Em.b * T.b};  // :183 (NN)
                        const RGB Bc{m0.z, m0.w, m1.x}, Sc{m2.x, m2.y, m2.z};
                        const float ns = 1 - spec;  // :184, Color::Lerp with t = 0 or 1 (NN)
                        const RGB f{Bc.r * ns + Sc.r * spec, Bc.g * ns + Sc.g * spec, Bc.b * ns + Sc.b * spec};
                        T = RGB{T.r * f.r, T.g * f.g, T.b * f.b};
                        hn = h.n;
                        hp = h.p;
                        hprim = h.prim;
                        ++bounce;
                        end_path = bounce >= B;
                    }
                    if (end_path) {  // the sample's colour into row (sample - c0), slot, of the wave's region; written exactly once
                        const uint32_t sidx = task >> 6;
                        rows[((sidx - c0) << 6) + (task & 63u)] = make_float4(L.r, L.g, L.b, __uint_as_float(sidx | atag));
                        busy = false;
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
            // The wave's own stores, made by whichever lane ran the path, are read back by the slots' owner lanes: the ROWS
            // kernel's release / acquire pair at workgroup scope (see pathtrace_kernel); no other wave ever touches these rows.
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            if (traced) {  // lane l folds rows 0 .. end - c0 - 1 of slot l, in sample order
                const float4* row = rows + lane;
                const uint32_t cnt = end - c0;
                uint32_t s = 0;
                for (; s + ROWS_IN_FLIGHT <= cnt; s += ROWS_IN_FLIGHT) {
                    float4 c[ROWS_IN_FLIGHT];
#pragma unroll
                    for (int k = 0; k < ROWS_IN_FLIGHT; ++k) c[k] = row[(size_t)(s + k) * 64];
#pragma unroll
                    for (int k = 0; k < ROWS_IN_FLIGHT; ++k) accumulate_sample(P, acc, RGB{c[k].x, c[k].y, c[k].z}, tag_alpha(__float_as_uint(c[k].w)), c0 + s + k);
                }
                for (; s < cnt; ++s) {
                    const float4 c = row[(size_t)s * 64];
                    accumulate_sample(P, acc, RGB{c.x, c.y, c.z}, tag_alpha(__float_as_uint(c.w)), c0 + s);
                }
            }
        }
        if (traced) io.out[i] = acc;
        __builtin_amdgcn_wave_barrier();  // (the next block rewrites the records)
    }
    if constexpr (COUNT) {  // the wave's sums: lane k adds counter k — one vector atomic per wave
        unsigned long long v = 0ull;
#pragma unroll
        for (int k = 0; k < RAD_WORK_N; ++k) v = lane == k ? W.n[k] : v;
        if (lane < RAD_WORK_N) atomicAdd(&io.work[lane], v);
    }
}

}  // namespace srt
