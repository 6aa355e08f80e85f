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
// The kernel's text is srt_adaptive_body.inc, included by the four kernels that run it, as srt_radiance.hip.h does and for its reason:
// the tail's inputs and the sun's frame are kernel arguments of their own, given only to the kernels that use them, and
// adaptive_kernel keeps the instructions it had.  The text reads P, io and the names TAIL, SUN, COUNT, tio
// and sio of the function it stands in.
template <bool SCENE_LDS, bool MESH, bool COUNT>
__global__ void __launch_bounds__(WG_THREADS) adaptive_kernel(const KernelParams P, const AdaptiveIO io) {
    constexpr bool TAIL = false, SUN = false;
    [[maybe_unused]] constexpr const ProbeTailIO* tio = nullptr;
    [[maybe_unused]] constexpr const SunIO* sio = nullptr;
#include "srt_adaptive_body.inc"
}

// srt_render_adaptive_tail: the same tiles, ticket and pool with the paths ended in the probe grid (srt_probe_tail.hip.h, rules
// T1 - T6).  The sums of both work records are always kept (they are scalar) and each is flushed when the launch has the record.
// A tile's pool drains before the wave draws its next ticket, so the lookups a wave makes depend only on the tile.
template <bool SCENE_LDS, bool MESH>
__global__ void __launch_bounds__(WG_THREADS) adaptive_tail_kernel(const KernelParams P, const AdaptiveIO io, const ProbeTailIO tail_io) {
    constexpr bool TAIL = true, SUN = false, COUNT = true;
    const ProbeTailIO* const tio = &tail_io;
    [[maybe_unused]] constexpr const SunIO* sio = nullptr;
#include "srt_adaptive_body.inc"
}

// srt_render_adaptive with SRT_ADAPTIVE_SUN_SAMPLING (srt_sun_sampling.hip.h, rules AS1 - AS3): the frame is a kernel argument of
// its own; the work sums are always kept and flushed when the launch has the record.  The segment's any_hit runs between two
// closest_hit calls on S.res and S.meshq; the first-hit records in S.pix, word 11 (the slot's first frame) among them, are not its.
template <bool SCENE_LDS, bool MESH>
__global__ void __launch_bounds__(WG_THREADS) adaptive_sun_kernel(const KernelParams P, const AdaptiveIO io, const SunIO sun_io) {
    constexpr bool TAIL = false, SUN = true, COUNT = true;
    [[maybe_unused]] constexpr const ProbeTailIO* tio = nullptr;
    const SunIO* const sio = &sun_io;
#include "srt_adaptive_body.inc"
}

// srt_render_adaptive_tail with the flag (rule AS4): every vertex a bounce is taken from gets its segment, the vertex at the
// bounce limit gets the lookup, and the hit that ends the path is read under the bounce's no_sun
template <bool SCENE_LDS, bool MESH>
__global__ void __launch_bounds__(WG_THREADS) adaptive_tail_sun_kernel(const KernelParams P, const AdaptiveIO io, const ProbeTailIO tail_io, const SunIO sun_io) {
    constexpr bool TAIL = true, SUN = true, COUNT = true;
    const ProbeTailIO* const tio = &tail_io;
    const SunIO* const sio = &sun_io;
#include "srt_adaptive_body.inc"
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
