// srt_probe_depth.hip.h — gfx950 probe depth moments (srt_trace_probe_depth) and the probe-grid shading that reads them
// (srt_shade_probe_grid_depth).  The header blocks of srt_pathtrace.h are the rules; this file restates them.  Everything is
// binary32 without contraction.
//
// probe_depth_kernel.  For probe p of P and direction k of K, ray (p, k) = (position[p], direction[k]); its distance r is the
// clamp to [0, max_distance] of what rays_kernel (srt_rays.hip.h) writes to SRT_GBUF_NORMAL_DEPTH.w for the explicit batch of
// those rays: the same closest_hit, on the same scene image, staged the same way.  Each probe has an octahedral map of R x R
// texels; texel tau with direction e (a table computed on the host, rule 1) takes the K distances weighted by
// cos^(2^s)(e, d_k) * weight_k, in ascending k: the weighted mean distance, the weighted mean squared distance, the weight, and
// the weighted share of rays that reached max_distance.
// Launched, sized and staged like light_probe_kernel (persistent workgroups, make_lds with four waves).  ONE WAVE PER PROBE:
// probes are dealt to the persistent waves, strided.  The wave walks the directions in blocks of 64: lane l traces ray 64 j + l
// through closest_hit with the full wave and leaves (d, r) in slot l of the wave's 64 x float4 colour ring and (weight, r*r) in
// the first 128 floats of its pixel records (LDS that make_lds already lays out: nothing beyond visibility_kernel's); after a
// wave barrier every lane adds the block's directions, ascending, into the R*R / 64 texels it owns (texel lane + 64 q; at R = 4
// only 16 lanes own one) — LDS broadcast reads, the texel directions and the sums in registers.  Nothing crosses lanes, so the
// order of rule 3 is the only order; no atomics reach an output.  Work counts (COUNT instantiations only): wave-uniform 64-bit
// sums, ONE vector atomic per wave at the end.
//
// probe_grid_depth_kernel.  The corner-packed body of srt_probe_grid.hip.h (probe_grid_shade, described there) with rule 7b
// (probe_depth_weigh) in place of the any-hit query.  It traces nothing, so it stages no scene and has one template axis; its LDS
// is the pixel records and the result slots of its four waves, 16 KiB.
#pragma once

#include "srt_kernel.hip.h"
#include "srt_probe_grid.hip.h"

namespace srt {

enum { PD_WORK_PROBES = 0, PD_WORK_RAYS, PD_WORK_FAR, PD_WORK_WAVE_CALLS, PD_WORK_WAVES, PD_WORK_N };
constexpr int PD_TEXELS_PER_LANE = 4;  // R = 16: 256 texels over 64 lanes

struct ProbeDepthIO {
    const float4* position;    // [probes] (p.xyz, ignored)
    const float4* direction;   // [directions] (d.xyz, weight)
    const float4* texel;       // [R*R] the texel directions of rule 1 (e.xyz, 0)
    uint32_t probes;           // P
    uint32_t directions;       // K, 1 .. 4096; P*K <= 2^30
    uint32_t resolution;       // R: 4, 8 or 16; P*R*R <= 2^30
    uint32_t sharpness;        // s, 0 .. 6
    float max_distance;        // > 0, finite
    uint32_t normalize;        // SRT_PROBE_DEPTH_NORMALIZE: d = float3::Normalized(d) first
    float4* moments;           // [P][R*R] (NULL: not requested)
    float* distances;          // [P][K] (NULL: not requested)
    unsigned long long* work;  // COUNT: [PD_WORK_N] totals of the launch (zeroed by the host before it)
    const uint32_t* list;      // LISTED: [4 + P] SRT_PROBE_LIST's layout: n, P, 0, 0, then the probe indices
};

template <bool ON>
struct PdWork {
    __device__ __forceinline__ void add(int, unsigned long long) {}
};
template <>
struct PdWork<true> {
    unsigned long long n[PD_WORK_N] = {0ull, 0ull, 0ull, 0ull, 0ull};
    __device__ __forceinline__ void add(int i, unsigned long long v) { n[i] += v; }
};

// LDS: the path-trace kernel's layout (make_lds with four waves), as rays_kernel.
// LISTED (srt_trace_probe_depth_listed): the waves are dealt the q < n of the list, n read from its header here; probe p = list[q],
// and a word >= P skips the probe.
template <bool SCENE_LDS, bool MESH, bool COUNT, bool LISTED = false>
__global__ void __launch_bounds__(WG_THREADS) probe_depth_kernel(const KernelParams P, const ProbeDepthIO io) {
    extern __shared__ float4 lds_scene[];
    // LISTED: the list's count and the word of this wave's first probe are loaded in front of the scene staging, so that their
    // latency (the first touch of the list) hides behind it instead of standing in front of the first probe.  (Loading later words one
    // probe ahead was measured twice and made the call slower, 1.06 - 1.08 of its parent against 1.006 - 1.011: DESIGN.md §4.31.)
    uint32_t list_count = 0u, first_word = 0u;
    if constexpr (LISTED) {
        const uint32_t q0 = blockIdx.x * (uint32_t)(WG_TILES_X * WG_TILES_Y) + (threadIdx.x >> 6);
        list_count = io.list[0];                             // (one address for the launch)
        if (q0 < io.probes) first_word = io.list[4u + q0];  // (the list has 4 + P words whatever its count says)
    }
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
    PdWork<COUNT> W;
    W.add(PD_WORK_WAVES, 1ull);
    auto lanes = [](bool b) { return (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(b)); };
    float4* const slots = S.ring;  // [64] (d.x, d.y, d.z, r) of the block in flight
    float* const extra = S.pix;    // [64] the directions' weights, then [64] r*r
    const uint32_t K = io.directions, R2 = io.resolution * io.resolution;
    const uint32_t J = (K + 63u) >> 6;
    const int owned = R2 >= 64u ? (int)(R2 >> 6) : 1;  // texels per owning lane: 1, 1, 4 (wave-uniform)
    const bool owner = (uint32_t)lane < R2;             // (R = 4: lanes 0 .. 15)
    const int sharp = (int)io.sharpness;
    const float maxd = io.max_distance;
    const bool norm = io.normalize != 0u;  // (a kernel argument: wave-uniform)
    // this lane's texel directions: the same for every probe
    float ex[PD_TEXELS_PER_LANE], ey[PD_TEXELS_PER_LANE], ez[PD_TEXELS_PER_LANE];
#pragma unroll
    for (int q = 0; q < PD_TEXELS_PER_LANE; ++q) {
        float4 e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (q < owned && owner) e = io.texel[lane + 64 * q];  // (lane + 64 q < R*R)
        ex[q] = e.x, ey[q] = e.y, ez[q] = e.z;
    }
    // wave-uniform loop: every lane of a wave runs the same trips, so closest_hit sees all 64 lanes in each call
    uint32_t units = io.probes;
    if constexpr (LISTED) units = list_count < io.probes ? list_count : io.probes;  // (a list holds at most P indices: nothing is read past 4 + P)
    for (uint32_t q = blockIdx.x * (uint32_t)WAVES + (uint32_t)wave; q < units; q += gridDim.x * (uint32_t)WAVES) {
        uint32_t p = q;
        if constexpr (LISTED) {
            p = q == blockIdx.x * (uint32_t)WAVES + (uint32_t)wave ? first_word : io.list[4u + q];  // (one address for the wave)
            if (p >= io.probes) continue;                                                            // a bad word skips the probe: no store can go out of range
        }
        const float4 o4 = io.position[p];  // (one address for the wave: a broadcast 16-byte load)
        float M1[PD_TEXELS_PER_LANE], M2[PD_TEXELS_PER_LANE], Wt[PD_TEXELS_PER_LANE], Ft[PD_TEXELS_PER_LANE];
#pragma unroll
        for (int q = 0; q < PD_TEXELS_PER_LANE; ++q) M1[q] = 0.0f, M2[q] = 0.0f, Wt[q] = 0.0f, Ft[q] = 0.0f;
        W.add(PD_WORK_PROBES, 1ull);
        for (uint32_t j = 0; j < J; ++j) {
            const uint32_t k = (j << 6) + (uint32_t)lane;
            const bool active = k < K;
            // lanes past K load no direction: they carry a harmless unit ray through the call and leave nothing that is read
            float4 d4 = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
            if (active) d4 = io.direction[k];
            V3 dir = v3(d4.x, d4.y, d4.z);
            if (norm) dir = normalized(dir);  // float3::Normalized (Common.hpp:159-162); its window test is wave-level: called by all lanes
            bool deferred = false;            // (defer_min = 1: every call resolves its mesh rays itself)
            const Hit h = closest_hit<MESH, false, SCENE_LDS>(S, P, v3(o4.x, o4.y, o4.z), dir, active, 1, deferred, no_tally SRT_PROF_ARG);
            // rule 2: rays_kernel's distance (+inf on a miss), clamped to [0, max_distance]
            const float t = h.prim >= 0 ? h.t : __builtin_inff();
            const float r = !(t > 0.0f) ? 0.0f : (t > maxd ? maxd : t);
            W.add(PD_WORK_WAVE_CALLS, 1ull);
            W.add(PD_WORK_RAYS, lanes(active));
            W.add(PD_WORK_FAR, lanes(active && r >= maxd));
            if (active && io.distances) io.distances[(size_t)p * K + k] = r;  // (p*K + k < 2^30)
            if (io.moments) {  // (wave-uniform)
                slots[lane] = make_float4(dir.x, dir.y, dir.z, r);
                extra[lane] = d4.w, extra[64 + lane] = r * r;
                __builtin_amdgcn_wave_barrier();
                // rule 3: the block's directions in ascending k into this lane's texels
                const int cnt = K - (j << 6) < 64u ? (int)(K - (j << 6)) : 64;
                if (owner) {
                    for (int m = 0; m < cnt; ++m) {
                        const float4 dr = slots[m];  // (one address for the wave: LDS broadcast reads)
                        const float dw = extra[m], rr = extra[64 + m];
#pragma unroll
                        for (int q = 0; q < PD_TEXELS_PER_LANE; ++q) {
                            if (q < owned) {
                                const float c = (ex[q] * dr.x + ey[q] * dr.y) + ez[q] * dr.z;
                                if (c > 0.0f) {
                                    float w = c;
                                    for (int i = 0; i < sharp; ++i) w = w * w;
                                    w = w * dw;
                                    M1[q] = M1[q] + w * dr.w;
                                    M2[q] = M2[q] + w * rr;
                                    Wt[q] = Wt[q] + w;
                                    if (dr.w >= maxd) Ft[q] = Ft[q] + w;
                                }
                            }
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();  // (the next block rewrites the slots)
            }
        }
        if (io.moments && owner) {  // rule 4
            float4* const out = io.moments + (size_t)p * R2;  // (p*R*R + texel < 2^30)
#pragma unroll
            for (int q = 0; q < PD_TEXELS_PER_LANE; ++q)
                if (q < owned)
                    out[lane + 64 * q] = Wt[q] > 0.0f ? make_float4(M1[q] / Wt[q], M2[q] / Wt[q], Wt[q], Ft[q] / Wt[q]) : make_float4(maxd, maxd * maxd, 0.0f, 1.0f);
        }
    }
    if constexpr (COUNT) {  // the wave's sums: lane k adds counter k — one vector atomic per wave
        unsigned long long v = 0ull;
#pragma unroll
        for (int q = 0; q < PD_WORK_N; ++q) v = lane == q ? W.n[q] : v;
        if (lane < PD_WORK_N) atomicAdd(&io.work[lane], v);
    }
}

// srt_shade_probe_grid_depth: probe_grid_shade with rule 7b; 16 KiB of static LDS
template <bool COUNT>
__global__ void __launch_bounds__(WG_THREADS) probe_grid_depth_kernel(const KernelParams P, const ProbeGridIO io) {
    constexpr int WAVES = WG_TILES_X * WG_TILES_Y;
    __shared__ float pix_records[WAVES][64 * PG_REC];
    __shared__ float4 result_slots[WAVES][64];
    const int wave = threadIdx.x >> 6;
    probe_grid_shade<false, PgTest::MOMENTS, COUNT>(P, io, pix_records[wave], result_slots[wave]);
}

}  // namespace srt
