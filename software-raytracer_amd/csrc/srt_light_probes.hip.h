// srt_light_probes.hip.h — gfx950 light probes (srt_trace_light_probes): for probe p of P and direction k of K, ray (p, k) =
// (position[p], direction[k]) with the stream id id_base + p*K + k; its radiance L_{p,k} is what radiance_kernel
// (srt_radiance.hip.h) writes to element p*K + k for the explicit batch of those rays; the probe's K radiances are projected
// onto the nine real SH basis functions of bands 0..2 with the directions' weights, in the header's fixed summation order.
//
// Launched, sized and staged exactly like radiance_kernel (persistent workgroups, make_lds with four waves, the grid-sized
// sample scratch).  A unit of work is (probe p, direction block j): units u = p*J + j, J = ceil(K / 64), are dealt to the
// persistent waves, strided, as radiance_kernel's blocks of 64 rays are.  Per unit:
//   1. Lane l forms its ray from position[p] — one broadcast 16-byte load — and direction[64j + l]: there is no P*K ray array.
//   2. ONE closest_hit for the 64 primaries; then radiance_kernel's steps 1-3 (the sample-independent lanes, the wave-level path
//      pool over (slot, sample) tasks with the sample rows in the wave's own region of the scratch, the ordered fold), restated
//      here expression by expression from srt_sample_pool.hip.h, the text radiance_kernel runs (DESIGN.md §4.32 says why this
//      kernel does not call it): the same bits.
//   3. Each lane multiplies its mean by the nine terms t_c = w * b_c; lanes past K carry +0.0f.  The wave runs 36 butterfly
//      reductions (9 coefficients x 4 lanes, six levels each, lane-xor 1, 2, 4, 8, 16, 32): binary32 addition commutes, so lane 0
//      holds exactly the header's pairwise tree v'[m] = v[2m] + v[2m+1].
//   4. J == 1: lane 0 writes the probe's nine float4.  J > 1: lane 0 writes the block sum to partial[u][9], and
//      light_probe_sum_kernel, one thread per (p, c), adds the J partials in ascending j.
// The RADIANCE output, when there is one, is written (and, without RESET, read) by the owner lane, as radiance_kernel's io.out.
// No atomics reach any output.  Work counts (COUNT instantiations only): wave-uniform 64-bit sums, ONE vector atomic per wave at
// the end.
#pragma once

#include "srt_kernel.hip.h"
#include "srt_radiance.hip.h"

namespace srt {

enum { LP_WORK_PROBES = 0, LP_WORK_RAYS, LP_WORK_SAMPLES, LP_WORK_CLOSEST, LP_WORK_WAVE_CALLS, LP_WORK_WAVES, LP_WORK_N };

constexpr int LP_COEFFS = 9;

struct LightProbeIO {
    const float4* position;    // [probes] (p.xyz, ignored)
    const float4* direction;   // [directions] (d.xyz, quadrature weight)
    uint32_t probes;           // P
    uint32_t directions;       // K, 1 .. 4096; P*K <= 2^30
    uint32_t blocks;           // J = ceil(K / 64)
    uint32_t normalize;        // SRT_LIGHT_PROBE_NORMALIZE: d = float3::Normalized(d) first
    uint32_t id_base;          // ray (p, k) draws from the stream of "pixel" id_base + p*K + k (mod 2^32)
    uint32_t reserved;
    float4* coefficients;      // J == 1: [P][9] the output (NULL: not requested); J > 1: unused here
    float4* partial;           // J > 1: [P][J][9] block sums (NULL: COEFFICIENTS not requested)
    float4* radiance;          // [P*K] the running means (NULL: not requested)
    float4* rows;              // [grid waves][RAD_CHUNK][64] sample colours of the chunk in flight
    unsigned long long* work;  // COUNT: [LP_WORK_N] totals of the launch (zeroed by the host before it)
    const uint32_t* list;      // LISTED: [4 + P] SRT_PROBE_LIST's layout: n, P, 0, 0, then the probe indices
};
// (the sample range, bounces, seed and SRT_LIGHT_PROBE_RESET travel in KernelParams, as radiance_kernel's)

template <bool ON>
struct LpWork {
    __device__ __forceinline__ void add(int, unsigned long long) {}
};
template <>
struct LpWork<true> {
    unsigned long long n[LP_WORK_N] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    __device__ __forceinline__ void add(int i, unsigned long long v) { n[i] += v; }
};
// ... of a TAIL instantiation (srt_probe_tail.hip.h): both records' sums are always kept and flushed when the launch has the record
struct LpTailWork : LpWork<true> {
    ProbeTail tail;
};
// ... of a SUN instantiation (srt_sun_sampling.hip.h): the sums are always kept and flushed when the launch has the record
struct LpSunWork : LpWork<true> {
    const SunIO* sun = nullptr;
};

// one butterfly of six levels: afterwards every lane holds the sum; lane 0's association is the header's pairwise tree
__device__ __forceinline__ float lp_wave_tree(float v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

// LDS: the path-trace kernel's layout (make_lds with four waves), as radiance_kernel.
// LISTED (srt_trace_light_probes_listed): the units are (q, j) for q < n, the count in the list's header, read here: the host never
// learns it; probe p = list[q], and a word >= P skips the unit.  Everything of probe p is computed and stored as the unlisted
// launch does it, but a multi-block partial goes to the COMPACT unit q*J + j (light_probe_sum_listed_kernel scatters it).
// The kernel's text is srt_light_probes_body.inc, included by the three kernels that run it, as radiance_kernel's (see there); TAIL
// (srt_probe_tail.hip.h) runs the lookup run_sample_pool calls at this text's own path end, SUN (srt_sun_sampling.hip.h) the sun
// sample run_sample_pool makes between the bounce and its closest_hit.
template <bool SCENE_LDS, bool MESH, bool COUNT, bool LISTED = false>
__global__ void __launch_bounds__(WG_THREADS) light_probe_kernel(const KernelParams P, const LightProbeIO io) {
    constexpr bool TAIL = false, SUN = false;
    [[maybe_unused]] constexpr const ProbeTailIO* tio = nullptr;
    [[maybe_unused]] constexpr const SunIO* sio = nullptr;
#include "srt_light_probes_body.inc"
}

// srt_trace_light_probes[_listed] under srt_probe_tail: the sums of both work records are always kept and flushed when the launch
// has the record
template <bool SCENE_LDS, bool MESH, bool LISTED>
__global__ void __launch_bounds__(WG_THREADS) light_probe_tail_kernel(const KernelParams P, const LightProbeIO io, const ProbeTailIO tail_io) {
    constexpr bool TAIL = true, SUN = false, COUNT = true;
    const ProbeTailIO* const tio = &tail_io;
    [[maybe_unused]] constexpr const SunIO* sio = nullptr;
#include "srt_light_probes_body.inc"
}

// srt_trace_light_probes[_listed] with SRT_LIGHT_PROBE_SUN_SAMPLING (srt_sun_sampling.hip.h): the frame is a kernel argument of its
// own; the work sums are always kept and flushed when the launch has the record
template <bool SCENE_LDS, bool MESH, bool LISTED>
__global__ void __launch_bounds__(WG_THREADS) light_probe_sun_kernel(const KernelParams P, const LightProbeIO io, const SunIO sun_io) {
    constexpr bool TAIL = false, SUN = true, COUNT = true;
    [[maybe_unused]] constexpr const ProbeTailIO* tio = nullptr;
    const SunIO* const sio = &sun_io;
#include "srt_light_probes_body.inc"
}

// J > 1: out[p][c] = partial[p][0][c], then + partial[p][j][c] for j = 1 .. J - 1 ascending, lane by lane.  One thread per (p, c).
__global__ void __launch_bounds__(256) light_probe_sum_kernel(const float4* __restrict__ partial, float4* __restrict__ out, size_t elems, uint32_t J) {
    const size_t e = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= elems) return;
    const size_t p = e / LP_COEFFS, c = e - p * LP_COEFFS;
    const float4* src = partial + p * (size_t)J * LP_COEFFS + c;
    float4 s = src[0];
    for (uint32_t j = 1; j < J; ++j) {
        const float4 v = src[(size_t)j * LP_COEFFS];
        s = make_float4(s.x + v.x, s.y + v.y, s.z + v.z, s.w + v.w);
    }
    out[e] = s;
}

}  // namespace srt
