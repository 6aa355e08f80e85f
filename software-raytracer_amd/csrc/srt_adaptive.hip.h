// srt_adaptive.hip.h — gfx950 adaptive sampling: srt_render_adaptive (a path trace whose sample range is per pixel) and
// srt_sample_budget (the pass that turns the variance buffer into that per-pixel range).
//
// adaptive_kernel.  Pixel p of the band holds n_p samples (the counts buffer) and may take b_p more (the budget buffer); the
// launch adds e_p = min(b_p, max_samples, 2147483646 - n_p) of them: the frames f = n_p + 1 .. n_p + e_p of srt_render, drawn from
// srt_rng_key(seed, pixel, f) and folded in ascending f into the accumulator element, so that the element equals what
// srt_render(1 .. n_p + e_p) leaves there.  It is radiance_kernel (srt_radiance.hip.h) with three changes:
//   1. The unit is an 8 x 8 pixel TILE of the band (visibility_kernel's lane <-> pixel mapping: x = lane & 7, y = lane >> 3) whose
//      camera rays the kernel makes itself (GetRayDirection, as gbuffer_kernel), not a strip of 64 caller rays.
//   2. The sample range is per LANE: slot l hands out samples [0, e_l) of its pixel, row (sample - chunk start) of the wave's
//      scratch region, and the wave-uniform chunk loop runs to the tile's largest e in steps of RAD_CHUNK.  The frame of a sample is
//      the slot's first frame n_l + 1 (word 11 of its record) plus the sample index.  The hand-out, the bounce, the scratch rows,
//      the release / acquire pairs and the 8-in-flight fold are radiance_kernel's, expression by expression.
//   3. Waves take tiles from a GLOBAL TICKET (one relaxed device-scope atomic add by one lane, broadcast with readfirstlane):
//      budgets are skewed by design, and with static striding most waves would sit idle behind those that drew the noisy tiles.
//      No data passes between waves through the ticket, so it needs no fence.  A wave takes its next tile only when its pool has
//      drained completely: plain dynamic scheduling of whole tiles, no refilling of a running pool.
// A pixel with e = 0 is not touched: no ray, no accumulator, framebuffer or count store; a tile of such pixels costs the loads of
// its budgets and counts.  A pixel whose primary ray misses (or any pixel when max_bounces == 0) folds its sample-independent
// colour e times.  After the fold: store_pixel (accumulator + framebuffer), then the count.  No atomic reaches the three
// buffers and the fold order per pixel is fixed, so the result does not depend on which wave drew which tile.
// Work counts (COUNT instantiations only): wave-uniform 64-bit sums, ONE vector atomic per wave at the end.
//
// budget_kernel.  One thread per pixel in the image passes' tile order; the 3 x 3 prefilter of the variance is
// srt_variance.hip.h's prefiltered_variance on its LDS tile, staged here from the variance buffer itself (level 0's working
// variance: v on hit pixels).  The budgets' sum: one wave reduction and one 64-bit vector atomic per wave.
#pragma once

#include "srt_radiance.hip.h"
#include "srt_variance.hip.h"

namespace srt {

enum { ADP_WORK_PIXELS = 0, ADP_WORK_SAMPLES, ADP_WORK_CLOSEST, ADP_WORK_WAVE_CALLS, ADP_WORK_N };

// the last frame a pixel may hold (srt_render's limit: first_sample + sample_count <= 2^31 - 1)
constexpr uint32_t ADP_FRAME_LIMIT = 2147483646u;

struct AdaptiveIO {
    const uint32_t* budget;    // [W*H] b_p
    uint32_t* counts;          // [W*H] n_p: read, and written (n_p + e_p) unless keep_counts
    uint32_t max_samples;      // 1 .. 4096
    uint32_t keep_counts;      // SRT_ADAPTIVE_KEEP_COUNTS
    uint32_t* ticket;          // the next tile of the band (zeroed by the host before the launch)
    float4* rows;              // [grid waves][RAD_CHUNK][64] sample colours of the chunk in flight
    unsigned long long* work;  // COUNT: [ADP_WORK_N] totals of the launch (zeroed by the host before it)
};
// (bounces, seed, the band, accumulator and framebuffer travel in KernelParams)

// wave-wide maximum / sum of a lane value (all lanes active), as a wave-uniform value
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64);
        v = w > v ? w : v;
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// e_p of the header's rule 1
__device__ __forceinline__ uint32_t effective_budget(uint32_t b, uint32_t n, uint32_t max_samples) {
    if (n >= ADP_FRAME_LIMIT) return 0u;
    const uint32_t room = ADP_FRAME_LIMIT - n;
    uint32_t e = b < max_samples ? b : max_samples;
    return e < room ? e : room;
}

// LDS: the path-trace kernel's layout (make_lds with four waves), as radiance_kernel.
template <bool SCENE_LDS, bool MESH, bool COUNT>
__global__ void __launch_bounds__(WG_THREADS) adaptive_kernel(const KernelParams P, const AdaptiveIO io) {
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
    RadWork<COUNT> Wk;
    auto lanes = [](bool b) { return (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(b)); };
    auto below = [](unsigned long long m) { return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)); };
    // this wave's region of the scratch: RAD_CHUNK rows of 64 slots
    float4* const rows = io.rows + ((size_t)blockIdx.x * WAVES + (size_t)wave) * (size_t)(RAD_CHUNK * 64);
    float* const rec = S.pix;                                      // [64][12]: dir, n0, p0, prim0, the key's seed-and-pixel half, the first frame
    unsigned* const match = reinterpret_cast<unsigned*>(S.work);  // [64] of (sample << 6 | slot), ~0 = nothing
    const int B = P.max_bounces;
    const int W = P.width, H = P.height;
    const int tiles_x = (W + TILE_W - 1) / TILE_W, tiles_y = (P.rows + TILE_H - 1) / TILE_H;
    const uint32_t tiles = (uint32_t)(tiles_x * tiles_y);
    const V3 cam = v3(P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]);
    // wave-uniform loop: every lane of a wave runs the same trips, so closest_hit sees all 64 lanes in each call
    for (;;) {
        uint32_t t = 0u;
        if (lane == 0) t = __hip_atomic_fetch_add(io.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
        if (t >= tiles) break;
        const int tx = (int)(t % (uint32_t)tiles_x), ty = (int)(t / (uint32_t)tiles_x);
        const int px = tx * TILE_W + (lane & 7), py = ty * TILE_H + (lane >> 3);
        const bool in_range = px < W && py < P.rows;
        // lanes outside the frame or band stand on the nearest pixel, load nothing, trace nothing and store nothing
        const int x = px < W ? px : W - 1, y = P.y0 + (py < P.rows ? py : P.rows - 1);
        const uint32_t pix = (uint32_t)x + (uint32_t)y * (uint32_t)W;
        uint32_t n0 = 0u, e = 0u;
        if (in_range) {
            n0 = io.counts[pix];
            e = effective_budget(io.budget[pix], n0, io.max_samples);
        }
        const bool want = e > 0u;
        if (__builtin_amdgcn_ballot_w64(want) == 0ull) continue;
        // ---- GetRayDirection (Raytracer.cpp:106-122), as gbuffer_kernel / pathtrace_kernel ----
        float nX = ((float)x / (float)W) * 2 - 1;
        float nY = ((float)y / (float)H) * 2 - 1;
        V3 u = v3(P.right_rd[0] * nX, P.right_rd[1] * nX, P.right_rd[2] * nX);
        V3 vv = v3(P.up_ld[0] * nY, P.up_ld[1] * nY, P.up_ld[2] * nY);
        const V3 dir0 = normalized(v3((u.x + vv.x) + P.fwd_clip[0], (u.y + vv.y) + P.fwd_clip[1], (u.z + vv.z) + P.fwd_clip[2]));
        bool deferred = false;  // (defer_min = 1: every call resolves its mesh rays itself)
        // ---- primary hit: identical for every sample (Raytracer.cpp:142); pixels without a budget trace no ray
        const Hit h0 = closest_hit<MESH, false, SCENE_LDS>(S, P, cam, dir0, want, 1, deferred, no_tally SRT_PROF_ARG);
        const bool traced = want && h0.prim >= 0 && B > 0;
        const uint32_t first_frame = n0 + 1u;  // (n0 < ADP_FRAME_LIMIT where want)
        Wk.add(ADP_WORK_WAVE_CALLS, 1ull);
        Wk.add(ADP_WORK_PIXELS, lanes(want));
        if constexpr (COUNT) {
            Wk.add(ADP_WORK_SAMPLES, (unsigned long long)wave_sum_u32(e));
            Wk.add(ADP_WORK_CLOSEST, (unsigned long long)wave_sum_u32(traced ? 0u : e));  // the primary counts once per sample (srt_stats.rays' rule)
        }
        float4 acc = make_float4(0, 0, 0, 0);
        if (want && n0 != 0u) acc = P.accumulator[pix];
        // ---- pixels whose colour does not depend on the sample: a miss -> env(d) every sample (:143-145); MAXBOUNCES == 0 ->
        // the first hit's EmissiveColor (:162, 212)
        if (want && !traced) {
            RGB c;
            float ca = 0.0f;  // the colour's alpha (+0 from the emissive colour)
            if (h0.prim < 0) {
                c = environment(S, dir0);
                ca = environment_alpha(dir0);
            } else {
                const float4 m1 = S.mat(h0.prim, 1);
                c = RGB{clamp0(m1.y), clamp0(m1.z), clamp0(m1.w)};
            }
            for (uint32_t s = 0; s < e; ++s) accumulate_frame(acc, c, ca, first_frame + s, first_frame + s == 1u);
            store_pixel(P, pix, acc);
            if (!io.keep_counts) io.counts[pix] = n0 + e;
        }
        if (__builtin_amdgcn_ballot_w64(traced) == 0ull) continue;

        // ---- wave-level path pool over (slot, sample): lane l owns slot l
        if (traced) {
            float* r = rec + lane * 12;
            r[0] = dir0.x, r[1] = dir0.y, r[2] = dir0.z;
            r[3] = h0.n.x, r[4] = h0.n.y, r[5] = h0.n.z;
            r[6] = h0.p.x, r[7] = h0.p.y, r[8] = h0.p.z;
            r[9] = __int_as_float(h0.prim);
            // srt_rng_key's first two rounds depend on seed and pixel only: done here once, the sample's round at the hand-out
            r[10] = __uint_as_float(srt_mix32(srt_mix32(P.seed ^ 0xA511E9B3U) + pix));
            r[11] = __uint_as_float(first_frame);
        }
        __builtin_amdgcn_wave_barrier();
        const uint32_t lim = traced ? e : 0u;                 // samples [0, lim) of this slot
        const uint32_t e_max = wave_max_u32(lim);             // (wave-uniform: the chunk loop's end)
        // path state of the task this lane is running
        bool busy = false;
        uint32_t task = 0;  // sample << 6 | slot
        RGB L{0, 0, 0}, T{0, 0, 0};
        V3 sray = v3(0, 0, 1), hn = v3(0, 0, 0), hp = v3(0, 0, 0);
        int hprim = 0, bounce = 0;
        float spec = 0.0f;
        uint32_t rng = 0;
        int rot = 0;  // wave-uniform rotation of the slot priority
        for (uint32_t c0 = 0; c0 < e_max; c0 += (uint32_t)RAD_CHUNK) {  // (wave-uniform)
            // this slot's part of the chunk: samples [begin, end), none once the slot has run out
            const uint32_t begin = lim < c0 ? lim : c0;
            const uint32_t end = lim - begin < (uint32_t)RAD_CHUNK ? lim : begin + (uint32_t)RAD_CHUNK;
            uint32_t own_next = begin;  // samples [begin, own_next) of this slot have been handed out
            // the fold of the chunk before has read the rows this chunk's paths overwrite
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            while (__builtin_amdgcn_ballot_w64(busy || own_next < end) != 0ull) {
                // ---- hand out tasks: radiance_kernel's — the slots that have samples left are dealt round-robin to the free
                // lanes, and a slot hands out as many consecutive samples as it is dealt lanes, up to what it has left.  Two
                // passes: entries that stayed empty in the first because a slot ran out find another slot in the second.
                bool fresh = false;
                for (int pass = 0; pass < 2; ++pass) {
                    const unsigned long long freem = __builtin_amdgcn_ballot_w64(!busy);
                    const int avail = own_next < end ? (int)(end - own_next) : 0;
                    const bool can = avail > 0;
                    const unsigned long long canm = __builtin_amdgcn_ballot_w64(can);
                    if (freem == 0ull || canm == 0ull) break;
                    const int nfree = __builtin_popcountll(freem), ncan = __builtin_popcountll(canm);
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
                if (fresh) {  // a lane that has just taken a task: Raytracer.cpp:162-166 for sample sidx of that pixel
                    const uint32_t sidx = task >> 6;
                    const float* r = rec + (int)(task & 63u) * 12;
                    const int prim0 = __float_as_int(r[9]);
                    rng = srt_mix32(__float_as_uint(r[10]) + (__float_as_uint(r[11]) + sidx));  // = srt_rng_key(seed, pixel, frame), see the record
                    const uint32_t rr = srt_mix32(rng) >> 17;                                    // draw 0: the specular lottery at the first hit
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
                Wk.add(ADP_WORK_CLOSEST, lanes(fresh));  // the sample's primary GetClosestObject call (:142)
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
                Wk.add(ADP_WORK_WAVE_CALLS, 1ull);
                Wk.add(ADP_WORK_CLOSEST, lanes(busy));
                if (busy) {
                    bool end_path;
                    uint32_t atag = 0u;  // the sample's alpha: NaN only from the environment (T's alpha is +0)
                    if (h.prim < 0) {    // :178-181
                        const RGB env = environment(S, sray);
                        L = RGB{L.r + env.r * T.r, L.g + env.g * T.g, L.b + env.b * T.b};  // (NN)
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
                        const uint32_t sidx = task >> 6;  // (in [c0, c0 + RAD_CHUNK): handed out by this chunk)
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
            if (begin < end) {  // lane l folds rows 0 .. end - c0 - 1 of slot l, in sample order (begin == c0 here)
                const float4* row = rows + lane;
                const uint32_t cnt = end - begin;
                const uint32_t f0 = first_frame + begin;  // the frame of row 0
                uint32_t s = 0;
                for (; s + ROWS_IN_FLIGHT <= cnt; s += ROWS_IN_FLIGHT) {
                    float4 c[ROWS_IN_FLIGHT];
#pragma unroll
                    for (int k = 0; k < ROWS_IN_FLIGHT; ++k) c[k] = row[(size_t)(s + k) * 64];
#pragma unroll
                    for (int k = 0; k < ROWS_IN_FLIGHT; ++k)
                        accumulate_frame(acc, RGB{c[k].x, c[k].y, c[k].z}, tag_alpha(__float_as_uint(c[k].w)), f0 + s + k, f0 + s + k == 1u);
                }
                for (; s < cnt; ++s) {
                    const float4 c = row[(size_t)s * 64];
                    accumulate_frame(acc, RGB{c.x, c.y, c.z}, tag_alpha(__float_as_uint(c.w)), f0 + s, f0 + s == 1u);
                }
            }
        }
        if (traced) {
            store_pixel(P, pix, acc);
            if (!io.keep_counts) io.counts[pix] = n0 + e;
        }
        __builtin_amdgcn_wave_barrier();  // (the next tile rewrites the records)
    }
    if constexpr (COUNT) {  // the wave's sums: lane k adds counter k — one vector atomic per wave
        unsigned long long v = 0ull;
#pragma unroll
        for (int k = 0; k < ADP_WORK_N; ++k) v = lane == k ? Wk.n[k] : v;
        if (lane < ADP_WORK_N) atomicAdd(&io.work[lane], v);
    }
}

// ---- srt_sample_budget ------------------------------------------------------------------------------------------------------
// All buffers W*H, index x + y * width, SCENE rows (the accumulator's layout).
struct BudgetLaunch {
    const float* variance;      // the current variance buffer
    const uint32_t* counts;     // n_p
    const float4* acc;          // the accumulator: c_p = its rgb
    const int32_t* object;      // SRT_GBUF_OBJECT
    const float4* albedo;       // SRT_GBUF_ALBEDO, NULL without SRT_BUDGET_ALBEDO
    uint32_t* budget;           // the output b_p
    unsigned long long* total;  // the sum of all b_p (zeroed by the host before the launch)
    int width, height;
    float threshold, floor;
    uint32_t max_budget;        // 1 .. 4096
};

// stage_variance_tile for level 0 read from the variance buffer itself: (v on a hit pixel, object as bits); object -2 outside
// the frame.  Every thread of the workgroup calls it, before any returns.
__device__ __forceinline__ void stage_variance_tile_level0(float2* tile, const int32_t* object, const float* variance, int W, int H) {
    const int x0 = (int)blockIdx.x * WG_W - 1, y0 = (int)blockIdx.y * WG_H - 1;
    for (int i = (int)threadIdx.x; i < VT_W * VT_H; i += WG_THREADS) {
        const int ty = i / VT_W, tx = i - ty * VT_W;
        const int gx = x0 + tx, gy = y0 + ty;
        int o = -2;
        float v = 0.0f;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t g = (size_t)gx + (size_t)gy * (size_t)W;
            o = object[g];
            if (o >= 0) v = variance[g];  // (a miss has no working variance)
        }
        tile[ty * VT_PITCH + tx] = make_float2(v, __int_as_float(o));
    }
    __syncthreads();
}

__global__ void __launch_bounds__(WG_THREADS) budget_kernel(const BudgetLaunch L) {
    const TilePixel tp = tile_pixel();
    const int W = L.width, H = L.height;
    __shared__ float2 tile[VT_H * VT_PITCH];
    stage_variance_tile_level0(tile, L.object, L.variance, W, H);
    uint32_t b = 0u;
    if (tp.x < W && tp.y < H) {
        const size_t p = (size_t)tp.x + (size_t)tp.y * (size_t)W;
        const int op = L.object[p];
        const uint32_t n = L.counts[p];
        if (op >= 0 && n != 0u) {  // rule 1: a miss is exactly converged, a pixel without samples has no variance
            const float g = prefiltered_variance(tile, tp.lx, tp.ly, op);
            const float4 c = L.acc[p];
            float l;
            if (L.albedo) {
                const float4 a = L.albedo[p];
                l = luminance(c.x / demod_factor(a.x), c.y / demod_factor(a.y), c.z / demod_factor(a.z));
            } else {
                l = luminance(c.x, c.y, c.z);
            }
            const float t = L.threshold * (l + L.floor);
            const float T = t * t;
            if (g > T) {  // (a NaN on either side: no budget)
                const float r = g / T;
                const float nf = (float)n;
                const float ex = nf * r - nf;  // the count at which g would reach T, less what the pixel holds
                const float mb = (float)L.max_budget;
                if (!(ex < mb)) {
                    b = L.max_budget;
                } else {
                    b = (uint32_t)ceilf(ex);
                    if (b < 1u) b = 1u;
                }
            }
        }
        L.budget[p] = b;
    }
    // the wave's sum (lanes outside the frame add 0): one vector atomic per wave
    const uint32_t s = wave_sum_u32(b);
    if ((threadIdx.x & 63) == 0) atomicAdd(L.total, (unsigned long long)s);
}

}  // namespace srt
