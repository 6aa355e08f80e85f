// srt_probe_update.hip.h — gfx950 per-frame probe updates: the list of a grid's active probes (srt_list_probes) and the
// hysteresis blend of newly traced probe data into a history (srt_blend_probes).  The header block of srt_pathtrace.h is the
// rules; this file restates them.  Everything is binary32 without contraction.
//
// probe_list_kernel.  A deterministic stream compaction of the state records: the indices p with (state & skip_mask) == 0, in
// ascending order, behind a four-word header (n, P, 0, 0); the words behind the n indices are 0xFFFFFFFF.  ONE WORKGROUP walks the
// records in chunks of PL_ROUNDS x WG_THREADS with a running base, so the order is ascending by construction: per chunk every
// thread loads the state words of its PL_ROUNDS records up front (record r*WG_THREADS + thread of the chunk: coalesced 4-byte
// loads at a 16-byte stride), a ballot and mbcnt give its rank inside its wave and round, lane 0 leaves the wave's count in LDS,
// and after one barrier every thread adds the counts of the (round, wave) pairs in front of its own: broadcast LDS reads.  The
// count table is double-buffered, so a chunk costs one barrier.  No atomic reaches the output.  At 8925 records that is nine
// chunks: microseconds; a two-level scan would be more code than that is worth.  Work counts (COUNT instantiation only): ONE
// vector atomic per wave at the end.
//
// probe_blend_kernel.  ONE WAVE PER PROBE, dealt to persistent waves, strided, as probe_classify_kernel deals them; with LISTED
// the units are the q < n of the list (n is read from the list's header on the device: the host never learns it) and p = list[q],
// a word >= P skips the unit.  The two DC loads (H[p][0], N[p][0]) and, with PREV, the two records are at one address per wave:
// broadcast 16-byte loads; the restart and change decisions (rules U2, U3) are wave-uniform.  Then the lanes stride over the
// probe's 9 + R*R float4 with 16-byte loads and stores: H = N on a restart, otherwise H = N + ((H - N) * h).  A streaming kernel:
// per element moved one read of H, one read of N and one write of H.  No atomics reach an output.  Work counts (COUNT
// instantiations only): wave-uniform 64-bit sums, ONE vector atomic per wave at the end.
#pragma once

#include "srt_kernel.hip.h"
#include "srt_probe_states.hip.h"

namespace srt {

enum { PL_WORK_PROBES = 0, PL_WORK_LISTED, PL_WORK_WAVES, PL_WORK_N };
enum { PB_WORK_PROBES = 0, PB_WORK_RESTARTED, PB_WORK_CHANGED, PB_WORK_WAVES, PB_WORK_N };
constexpr int PL_ROUNDS = 4;       // records per thread and chunk
constexpr uint32_t PL_HEADER = 4;  // n, P, 0, 0
constexpr int PB_COEFFS = 9;

struct ProbeListIO {
    const float4* states;      // [P] (o.xyz, state bits): SRT_PROBE_STATE_RECORDS' layout
    uint32_t* list;            // [4 + P]
    uint32_t probes;           // P, 1 .. 2^30
    uint32_t skip_mask;        // a probe with (state & skip_mask) != 0 is not listed
    unsigned long long* work;  // COUNT: [PL_WORK_N] totals of the launch (zeroed by the host before it)
};

// Launched with ONE workgroup of WG_THREADS threads.
template <bool COUNT>
__global__ void __launch_bounds__(WG_THREADS) probe_list_kernel(const ProbeListIO io) {
    constexpr int WAVES = WG_THREADS / 64;
    constexpr uint32_t CHUNK = (uint32_t)(PL_ROUNDS * WG_THREADS);
    __shared__ uint32_t counts[2][PL_ROUNDS * WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t P = io.probes;
    const uint32_t* const words = reinterpret_cast<const uint32_t*>(io.states);  // record i's state: word 4 i + 3
    uint32_t* const out = io.list + PL_HEADER;
    uint32_t base = 0;  // indices written so far (the same in every thread)
    unsigned long long seen = 0ull;
    int buf = 0;
    for (uint32_t c0 = 0; c0 < P; c0 += CHUNK, buf ^= 1) {  // (P <= 2^30: c0 + CHUNK does not wrap)
        uint32_t idx[PL_ROUNDS];
        bool keep[PL_ROUNDS];
#pragma unroll
        for (int r = 0; r < PL_ROUNDS; ++r) {
            idx[r] = c0 + (uint32_t)(r * WG_THREADS) + threadIdx.x;
            uint32_t st = 0xFFFFFFFFu;
            if (idx[r] < P) st = words[4 * (size_t)idx[r] + 3];
            keep[r] = idx[r] < P && (st & io.skip_mask) == 0u;
        }
        uint32_t rank[PL_ROUNDS];
#pragma unroll
        for (int r = 0; r < PL_ROUNDS; ++r) {
            const unsigned long long m = __builtin_amdgcn_ballot_w64(keep[r]);
            rank[r] = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            if (lane == 0) counts[buf][r * WAVES + wave] = (uint32_t)__builtin_popcountll(m);
            if constexpr (COUNT) seen += (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(idx[r] < P));
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < PL_ROUNDS; ++r) {
            uint32_t before = base;  // the indices in front of (round r, this wave)
#pragma unroll
            for (int w = 0; w < WAVES; ++w) {
                const uint32_t n = counts[buf][r * WAVES + w];
                before += w < wave ? n : 0u;
                base += n;
            }
            if (keep[r]) out[before + rank[r]] = idx[r];  // (before + rank < the number of kept records <= P)
        }
        // (the next chunk writes the other count table; the one after it comes behind the next barrier)
    }
    for (uint32_t i = base + threadIdx.x; i < P; i += (uint32_t)WG_THREADS) out[i] = 0xFFFFFFFFu;
    if (threadIdx.x < PL_HEADER) io.list[threadIdx.x] = threadIdx.x == 0 ? base : threadIdx.x == 1 ? P : 0u;
    if constexpr (COUNT) {  // the wave's sums: lane k adds counter k — one vector atomic per wave; wave 0 reports the listed count
        unsigned long long v = 0ull;
        v = lane == PL_WORK_PROBES ? seen : v;
        v = lane == PL_WORK_LISTED ? (wave == 0 ? (unsigned long long)base : 0ull) : v;
        v = lane == PL_WORK_WAVES ? 1ull : v;
        if (lane < PL_WORK_N) atomicAdd(&io.work[lane], v);
    }
}

// The listed variant of light_probe_sum_kernel (J > 1), launched for P*9 threads: thread (q, c) with q < n adds the J partials of
// the COMPACT units q*J + j in ascending j, lane by lane, and stores to slot p = list[q].  Threads past n*9 exit, and a word >= P
// stores nothing.
__global__ void __launch_bounds__(256) light_probe_sum_listed_kernel(const float4* __restrict__ partial, float4* __restrict__ out, const uint32_t* __restrict__ list,
                                                                     uint32_t probes, uint32_t J) {
    const size_t e = (size_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t ln = list[0];
    const size_t n = ln < probes ? ln : probes;
    if (e >= n * PB_COEFFS) return;
    const size_t q = e / PB_COEFFS, c = e - q * PB_COEFFS;
    const uint32_t p = list[PL_HEADER + q];
    if (p >= probes) return;
    const float4* src = partial + q * (size_t)J * PB_COEFFS + c;
    float4 s = src[0];
    for (uint32_t j = 1; j < J; ++j) {
        const float4 v = src[(size_t)j * PB_COEFFS];
        s = make_float4(s.x + v.x, s.y + v.y, s.z + v.z, s.w + v.w);
    }
    out[(size_t)p * PB_COEFFS + c] = s;
}

struct ProbeBlendIO {
    float4* history;             // [P][9] H, updated in place
    const float4* fresh;         // [P][9] N: what the last light-probe trace wrote
    float4* depth_history;       // MOMENTS: [P][R*R]
    const float4* depth_fresh;   // MOMENTS: [P][R*R]
    const uint32_t* list;        // LISTED: [4 + P]
    const float4* states;        // PREV: [P] the current records
    const float4* previous;      // PREV: [P] the previous records
    uint32_t probes;             // P
    uint32_t texels;             // MOMENTS: R*R (otherwise 0)
    float hysteresis, fast_hysteresis, depth_hysteresis, change_threshold;
    unsigned long long* work;    // COUNT: [PB_WORK_N] totals of the launch (zeroed by the host before it)
};

// rule U3's luminance (Rec. 709 weights; no header of the project fixes others)
__device__ __forceinline__ float probe_blend_luminance(const float4 v) { return (0.2126f * v.x + 0.7152f * v.y) + 0.0722f * v.z; }

// rules U2 / U4 / U5 on one float4
__device__ __forceinline__ float4 probe_blend_mix(const float4 H, const float4 N, bool restart, float h) {
    if (restart) return N;
    return make_float4(N.x + ((H.x - N.x) * h), N.y + ((H.y - N.y) * h), N.z + ((H.z - N.z) * h), N.w + ((H.w - N.w) * h));
}

template <bool LISTED, bool PREV, bool COUNT>
__global__ void __launch_bounds__(WG_THREADS) probe_blend_kernel(const ProbeBlendIO io) {
    constexpr int WAVES = WG_TILES_X * WG_TILES_Y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t P = io.probes, R2 = io.texels;
    uint32_t units = P;
    if constexpr (LISTED) {
        const uint32_t n = io.list[0];  // (one address for the launch)
        units = n < P ? n : P;          // (a list never holds more than P indices: nothing is read past 4 + P)
    }
    unsigned long long n_probes = 0ull, n_restart = 0ull, n_changed = 0ull;
    for (uint32_t q = blockIdx.x * (uint32_t)WAVES + (uint32_t)wave; q < units; q += gridDim.x * (uint32_t)WAVES) {
        uint32_t p = q;
        if constexpr (LISTED) {
            p = io.list[PL_HEADER + q];  // (wave-uniform)
            if (p >= P) continue;        // a bad word skips the unit
        }
        float4* const H = io.history + (size_t)p * PB_COEFFS;
        const float4* const N = io.fresh + (size_t)p * PB_COEFFS;
        const float4 h0 = H[0], n0 = N[0];  // (one address for the wave: broadcast 16-byte loads)
        bool restart = __float_as_uint(h0.w) == 0u;  // rule U2
        if constexpr (PREV) {
            const float4 a = io.states[p], b = io.previous[p];
            const bool moved = __float_as_uint(a.x) != __float_as_uint(b.x) || __float_as_uint(a.y) != __float_as_uint(b.y) || __float_as_uint(a.z) != __float_as_uint(b.z);
            restart = restart || moved || ((__float_as_uint(a.w) ^ __float_as_uint(b.w)) & (PS_BURIED | PS_IDLE)) != 0u;
        }
        // rule U3
        const float yh = probe_blend_luminance(h0), yn = probe_blend_luminance(n0);
        const float d = fabsf(yn - yh);
        const float ah = fabsf(yh), an = fabsf(yn);
        const float m = ah > an ? ah : an;
        const bool changed = d > io.change_threshold * m;
        const float h = changed ? io.fast_hysteresis : io.hysteresis;
        // every lane has read H[0] before any lane writes it: the loads above are complete once their values are used, and
        // lane 0's store of element 0 depends on them.  (Within this wave; no other wave has this probe: a list's indices are
        // distinct, the header's rule L.)
        if (lane < PB_COEFFS) H[lane] = probe_blend_mix(lane == 0 ? h0 : H[lane], lane == 0 ? n0 : N[lane], restart, h);  // rule U4
        if (R2 != 0u) {  // rule U5 (wave-uniform)
            float4* const DH = io.depth_history + (size_t)p * R2;
            const float4* const DN = io.depth_fresh + (size_t)p * R2;
            for (uint32_t t = (uint32_t)lane; t < R2; t += 64u) DH[t] = probe_blend_mix(DH[t], DN[t], restart, io.depth_hysteresis);
        }
        if constexpr (COUNT) n_probes += 1ull, n_restart += restart ? 1ull : 0ull, n_changed += !restart && changed ? 1ull : 0ull;
    }
    if constexpr (COUNT) {  // the wave's sums: lane k adds counter k — one vector atomic per wave
        unsigned long long v = 0ull;
        v = lane == PB_WORK_PROBES ? n_probes : v;
        v = lane == PB_WORK_RESTARTED ? n_restart : v;
        v = lane == PB_WORK_CHANGED ? n_changed : v;
        v = lane == PB_WORK_WAVES ? 1ull : v;
        if (lane < PB_WORK_N) atomicAdd(&io.work[lane], v);
    }
}

}  // namespace srt
