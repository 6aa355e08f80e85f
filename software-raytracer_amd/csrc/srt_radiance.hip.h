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

#include <type_traits>

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
// The kernel's text is srt_radiance_body.inc, included by the two kernels that run it: they differ in their ARGUMENTS (the tail's
// inputs are a kernel argument of their own, given only to the TAIL kernel), and a body they both called would be one text, but
// radiance_kernel would no longer compile to the instructions it had.  The text reads P, io and the names TAIL,
// COUNT and tio of the function it stands in.
template <bool SCENE_LDS, bool MESH, bool COUNT>
__global__ void __launch_bounds__(WG_THREADS) radiance_kernel(const KernelParams P, const RadianceIO io) {
    constexpr bool TAIL = false, SUN = false;
    [[maybe_unused]] constexpr const ProbeTailIO* tio = nullptr;
    [[maybe_unused]] constexpr const SunIO* sio = nullptr;
#include "srt_radiance_body.inc"
}

// srt_trace_radiance under srt_probe_tail (srt_probe_tail.hip.h): the sums of both work records are always kept (they are scalar)
// and flushed when the launch has the record
template <bool SCENE_LDS, bool MESH>
__global__ void __launch_bounds__(WG_THREADS) radiance_tail_kernel(const KernelParams P, const RadianceIO io, const ProbeTailIO tail_io) {
    constexpr bool TAIL = true, SUN = false, COUNT = true;
    const ProbeTailIO* const tio = &tail_io;
    [[maybe_unused]] constexpr const SunIO* sio = nullptr;
#include "srt_radiance_body.inc"
}

// srt_trace_radiance with SRT_RADIANCE_SUN_SAMPLING (srt_sun_sampling.hip.h): the frame is a kernel argument of its own; the work
// sums are always kept and flushed when the launch has the record
template <bool SCENE_LDS, bool MESH>
__global__ void __launch_bounds__(WG_THREADS) radiance_sun_kernel(const KernelParams P, const RadianceIO io, const SunIO sun_io) {
    constexpr bool TAIL = false, SUN = true, COUNT = true;
    [[maybe_unused]] constexpr const ProbeTailIO* tio = nullptr;
    const SunIO* const sio = &sun_io;
#include "srt_radiance_body.inc"
}

}  // namespace srt
