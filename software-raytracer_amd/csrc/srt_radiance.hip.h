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
//      records and become the slot's owner.  The wave then runs the sample pool of srt_sample_pool.hip.h over (slot, sample)
//      tasks — pathtrace_kernel's path pool with the samples of one ray as the tasks of a slot — with LaunchSamples as its
//      sample source: every traced slot runs the launch's samples [0, n), chunk after chunk of RAD_CHUNK, and the owner lanes
//      fold their slot's rows of the wave's own scratch region in sample order.  The running mean stays in the owner's registers.
// The fold order per ray is fixed (ascending f) whatever the packing does, no atomics reach the output: repeated calls give the
// same bits.  Mesh scenes pass defer_min = 1 as rays_kernel does: every call resolves its mesh rays itself, nothing is parked.
// Work counts (COUNT instantiations only): wave-uniform 64-bit sums, added to a handle-owned record with ONE vector atomic per
// wave at the end.  Without COUNT there is no atomic.
#pragma once

#include "srt_sample_pool.hip.h"

namespace srt {

enum { RAD_WORK_RAYS = 0, RAD_WORK_SAMPLES, RAD_WORK_CLOSEST, RAD_WORK_WAVE_CALLS, RAD_WORK_N };

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

// LDS: the path-trace kernel's layout (make_lds with four waves), as rays_kernel.
template <bool SCENE_LDS, bool MESH, bool COUNT>
__global__ void __launch_bounds__(WG_THREADS) radiance_kernel(const KernelParams P, const RadianceIO io) {
    extern __shared__ float4 lds_scene[];
    stage_scene<SCENE_LDS>(P, lds_scene);
    constexpr int WAVES = WG_TILES_X * WG_TILES_Y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Lds S = make_lds<SCENE_LDS>(P, lds_scene, WAVES, wave);
#if defined(SRT_STATS) && SRT_STATS == 3
    Prof prof{};
#endif
    Tally<false> no_tally;
    WaveWork<COUNT, RAD_WORK_N> W;
    float4* const rows = wave_sample_rows(io.rows, wave);
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
        W.add(RAD_WORK_RAYS, wave_lanes(active));
        W.add(RAD_WORK_SAMPLES, wave_lanes(active) * n);
        W.add(RAD_WORK_CLOSEST, wave_lanes(active && !traced) * n);  // the primary counts once per sample (srt_stats.rays' rule)
        float4 acc = make_float4(0, 0, 0, 0);
        if (active && !reset) acc = io.out[i];
        const LaunchSamples<RAD_WORK_CLOSEST, RAD_WORK_WAVE_CALLS> samples{P, traced};
        if (active && !traced) {  // the colour does not depend on the sample
            fold_constant_colour(S, samples, dir0, h0, n, acc);
            io.out[i] = acc;
        }
        if (__builtin_amdgcn_ballot_w64(traced) == 0ull) continue;
        // srt_rng_key's id of ray i: id_base + i
        if (traced) write_first_hit_record(S, lane, dir0, h0, P.seed, io.id_base + i);
        __builtin_amdgcn_wave_barrier();
        run_sample_pool<MESH, SCENE_LDS>(S, P, samples, rows, lane, acc, W SRT_PROF_ARG);
        if (traced) io.out[i] = acc;
        __builtin_amdgcn_wave_barrier();  // (the next block rewrites the records)
    }
    W.flush(io.work, lane);
}

}  // namespace srt
