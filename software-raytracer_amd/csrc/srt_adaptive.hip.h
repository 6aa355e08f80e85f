// srt_adaptive.hip.h — gfx950 adaptive sampling: srt_render_adaptive (a path trace whose sample range is per pixel) and
// srt_sample_budget (the pass that turns the variance buffer into that per-pixel range).
//
// adaptive_kernel.  Pixel p of the band holds n_p samples (the counts buffer) and may take b_p more (the budget buffer); the
// launch adds e_p = min(b_p, max_samples, 2147483646 - n_p) of them: the frames f = n_p + 1 .. n_p + e_p of srt_render, drawn from
// srt_rng_key(seed, pixel, f) and folded in ascending f into the accumulator element, so that the element equals what
// srt_render(1 .. n_p + e_p) leaves there.  It is radiance_kernel (srt_radiance.hip.h) with three changes:
//   1. The unit is an 8 x 8 pixel TILE of the band (visibility_kernel's lane <-> pixel mapping: x = lane & 7, y = lane >> 3) whose
//      camera rays the kernel makes itself (GetRayDirection, as gbuffer_kernel), not a strip of 64 caller rays.
//   2. The sample range is per LANE (PixelSamples below, the sample source the pool of srt_sample_pool.hip.h runs on): slot l
//      hands out samples [0, e_l) of its pixel, row (sample - chunk start) of the wave's scratch region, and the wave-uniform
//      chunk loop runs to the tile's largest e in steps of RAD_CHUNK.  The frame of a sample is the slot's first frame n_l + 1
//      (word 11 of its record) plus the sample index.  The hand-out, the bounce, the scratch rows, the release / acquire pairs
//      and the 8-in-flight fold are the pool's: the text radiance_kernel runs.
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

// the samples of adaptive_kernel (srt_sample_pool.hip.h): [0, lim) of the lane's own slot; the
// frame of a sample is the slot's first frame (word 11 of its record) plus the sample index
struct PixelSamples {
    static constexpr int CLOSEST = ADP_WORK_CLOSEST, WAVE_CALLS = ADP_WORK_WAVE_CALLS;
    uint32_t lim, first_frame;
    struct Chunk {  // this slot's part of the chunk: samples [begin, end), none once the slot has run out (else begin == c0)
        uint32_t begin, end;
        __device__ __forceinline__ uint32_t first() const { return begin; }
        __device__ __forceinline__ bool owner() const { return begin < end; }
        __device__ __forceinline__ uint32_t count() const { return end - begin; }
    };
    __device__ __forceinline__ uint32_t last() const { return wave_max_u32(lim); }  // (the tile's largest)
    __device__ __forceinline__ Chunk chunk(uint32_t c0) const {
        const uint32_t begin = lim < c0 ? lim : c0;
        return Chunk{begin, lim - begin < (uint32_t)RAD_CHUNK ? lim : begin + (uint32_t)RAD_CHUNK};
    }
    __device__ __forceinline__ uint32_t frame(const float* r, uint32_t sidx) const { return __float_as_uint(r[11]) + sidx; }
    __device__ __forceinline__ void fold(float4& acc, RGB c, float a, uint32_t s) const {
        const uint32_t f = first_frame + s;
        accumulate_frame(acc, c, a, f, f == 1u);
    }
};

// LDS: the path-trace kernel's layout (make_lds with four waves), as radiance_kernel.
template <bool SCENE_LDS, bool MESH, bool COUNT>
__global__ void __launch_bounds__(WG_THREADS) adaptive_kernel(const KernelParams P, const AdaptiveIO io) {
    extern __shared__ float4 lds_scene[];
    stage_scene<SCENE_LDS>(P, lds_scene);
    constexpr int WAVES = WG_TILES_X * WG_TILES_Y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Lds S = make_lds<SCENE_LDS>(P, lds_scene, WAVES, wave);
#if defined(SRT_STATS) && SRT_STATS == 3
    Prof prof{};
#endif
    Tally<false> no_tally;
    WaveWork<COUNT, ADP_WORK_N> Wk;
    float4* const rows = wave_sample_rows(io.rows, wave);
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
        Wk.add(ADP_WORK_PIXELS, wave_lanes(want));
        if constexpr (COUNT) {
            Wk.add(ADP_WORK_SAMPLES, (unsigned long long)wave_sum_u32(e));
            Wk.add(ADP_WORK_CLOSEST, (unsigned long long)wave_sum_u32(traced ? 0u : e));  // the primary counts once per sample (srt_stats.rays' rule)
        }
        float4 acc = make_float4(0, 0, 0, 0);
        if (want && n0 != 0u) acc = P.accumulator[pix];
        // samples [0, lim) of this slot; the chunk loop runs to the tile's largest
        const uint32_t lim = traced ? e : 0u;
        const PixelSamples samples{lim, first_frame};
        if (want && !traced) {  // the colour does not depend on the sample
            fold_constant_colour(S, samples, dir0, h0, e, acc);
            store_pixel(P, pix, acc);
            if (!io.keep_counts) io.counts[pix] = n0 + e;
        }
        if (__builtin_amdgcn_ballot_w64(traced) == 0ull) continue;
        if (traced) {  // srt_rng_key's id of a pixel: its index
            write_first_hit_record(S, lane, dir0, h0, P.seed, pix);
            S.pix[lane * 12 + 11] = __uint_as_float(first_frame);
        }
        __builtin_amdgcn_wave_barrier();
        run_sample_pool<MESH, SCENE_LDS>(S, P, samples, rows, lane, acc, Wk SRT_PROF_ARG);
        if (traced) {
            store_pixel(P, pix, acc);
            if (!io.keep_counts) io.counts[pix] = n0 + e;
        }
        __builtin_amdgcn_wave_barrier();  // (the next tile rewrites the records)
    }
    Wk.flush(io.work, lane);
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
