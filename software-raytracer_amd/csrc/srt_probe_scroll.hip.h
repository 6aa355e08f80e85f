// srt_probe_scroll.hip.h — gfx950 scrolling of a probe grid (srt_scroll_probes): the per-probe arrays of the grid moved by a whole
// number of cells.  The header block of srt_pathtrace.h is the rules (SC1 .. SC8); this file restates SC1 and SC2.
//
// probe_scroll_kernel.  ONE WAVE PER DESTINATION PROBE, dealt to persistent waves, strided, as probe_blend_kernel deals them.  ONE
// launch serves every selected array (coefficients [P][9], moments [P][R*R], records [P], float4 each), so the decision "retained
// or exposed" is made once per probe; it is wave-uniform: the destination index is made scalar, the source coordinate j = i + shift
// is formed per axis in 64 bits, and the source INDEX is formed only when all three lie inside the grid, so no load can leave an
// array whatever `shift` holds.  The lanes then stride the probe's elements with 16-byte loads and stores, both sides contiguous
// per probe; an exposed probe stores zero bits and loads nothing.  Elements move as four 32-bit words: no arithmetic touches
// them, so a NaN keeps its payload.  Source and destination are DISTINCT buffers (the host gives a spare): waves of one launch
// never read what another wrote.  A streaming kernel: per element moved one read and one write; no LDS, no scratch.  No atomic
// reaches an output.  Work counts (COUNT instantiation only): wave-uniform 64-bit sums, ONE vector atomic per wave at the end.
#pragma once

#include "srt_kernel.hip.h"

namespace srt {

enum { PSC_WORK_PROBES = 0, PSC_WORK_RETAINED, PSC_WORK_EXPOSED, PSC_WORK_WAVES, PSC_WORK_N };
constexpr int PSC_ARRAYS = 3;  // coefficients, moments, records

struct ProbeScrollIO {
    const uint4* src[PSC_ARRAYS];  // [P][elems] each; NULL with dst: the array is not moved by this launch
    uint4* dst[PSC_ARRAYS];        // never a src of the same launch
    uint32_t elems[PSC_ARRAYS];    // 16-byte elements per probe: 9, R*R, 1
    uint32_t probes;               // P = nx * ny * nz, 1 .. 2^30
    int32_t counts[3];             // nx, ny, nz
    int32_t shift[3];              // any int32
    unsigned long long* work;      // COUNT: [PSC_WORK_N] totals of the launch (zeroed by the host before it)
};

template <bool COUNT>
__global__ void __launch_bounds__(WG_THREADS) probe_scroll_kernel(const ProbeScrollIO io) {
    constexpr int WAVES = WG_TILES_X * WG_TILES_Y;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (the same in all lanes: scalar from here on)
    const uint32_t P = io.probes, nx = (uint32_t)io.counts[0], ny = (uint32_t)io.counts[1];
    unsigned long long n_probes = 0ull, n_retained = 0ull;
    for (uint32_t i = blockIdx.x * (uint32_t)WAVES + wave; i < P; i += gridDim.x * (uint32_t)WAVES) {
        // rule SC1
        const uint32_t t = i / nx;
        const long long jx = (long long)(i - t * nx) + (long long)io.shift[0];
        const long long jy = (long long)(t % ny) + (long long)io.shift[1];
        const long long jz = (long long)(t / ny) + (long long)io.shift[2];
        const bool retained = jx >= 0 && jx < (long long)io.counts[0] && jy >= 0 && jy < (long long)io.counts[1] && jz >= 0 && jz < (long long)io.counts[2];
        // (inside the grid each coordinate is below its count, so the index is below P)
        const size_t j = retained ? (size_t)jx + (size_t)nx * ((size_t)jy + (size_t)ny * (size_t)jz) : (size_t)0;
#pragma unroll
        for (int a = 0; a < PSC_ARRAYS; ++a) {  // rule SC2 / SC3
            uint4* const D = io.dst[a];
            if (!D) continue;  // (uniform for the launch)
            const uint32_t n = io.elems[a];
            uint4* const d = D + (size_t)i * n;
            if (retained) {
                const uint4* const s = io.src[a] + j * n;
                for (uint32_t e = (uint32_t)lane; e < n; e += 64u) d[e] = s[e];
            } else {
                for (uint32_t e = (uint32_t)lane; e < n; e += 64u) d[e] = make_uint4(0u, 0u, 0u, 0u);
            }
        }
        if constexpr (COUNT) n_probes += 1ull, n_retained += retained ? 1ull : 0ull;
    }
    if constexpr (COUNT) {  // the wave's sums: lane k adds counter k — one vector atomic per wave
        unsigned long long v = 0ull;
        v = lane == PSC_WORK_PROBES ? n_probes : v;
        v = lane == PSC_WORK_RETAINED ? n_retained : v;
        v = lane == PSC_WORK_EXPOSED ? n_probes - n_retained : v;
        v = lane == PSC_WORK_WAVES ? 1ull : v;
        if (lane < PSC_WORK_N) atomicAdd(&io.work[lane], v);
    }
}

}  // namespace srt
