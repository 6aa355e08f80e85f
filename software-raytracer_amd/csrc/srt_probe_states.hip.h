// srt_probe_states.hip.h — gfx950 probe classification and relocation (srt_classify_probes) and the probe-grid shading that obeys
// the records (srt_shade_probe_grid_states).  The header blocks of srt_pathtrace.h are the rules; this file restates them.
// Everything is binary32 without contraction.
//
// probe_classify_kernel.  Spheres and axis-aligned boxes have an exact signed distance, so the state of a probe needs no ray: S(x)
// is the smallest signed distance from x to any sphere or box of the scene (rule S1; meshes contribute nothing), a probe with
// S < 0 lies inside an object, and with SRT_PROBE_CLASSIFY_RELOCATE a probe nearer than `margin` to a surface is moved along one of
// the K shared directions to the first distance (of `steps`) at which some direction clears the margin, to the direction that
// clears it by most (rule S4).  No rays, no closest_hit, no scene image: the kernel reads a primitive table of its own (the host
// builds it from the object list; the scene image stores r*r, not r): `spheres` float4 (centre, |radius|), then `boxes` pairs
// (centre, 0), (half size, 0).
// ONE WAVE PER PROBE, dealt to persistent waves, strided, as probe_depth_kernel deals them.  s0 = S(g) is computed by every lane on
// the same values at wave-uniform addresses.  A wave whose probe needs no search is done after that.  In the search lane l takes
// direction 64 j + l and every lane loops over all primitives: the table is read at one address per wave.  WHERE THE TABLE LIVES:
// in LDS when it fits (TABLE_LDS: staged once per workgroup, read back with broadcast ds_read_b128, which are in order and need
// no waitcnt on the scalar cache in the inner loop), otherwise in memory, read through the caches at uniform addresses.  Per step
// each lane keeps its best accepted (S, k) — ascending k, so a strict > keeps the lowest k — then a butterfly over the wave takes
// the largest S and on equal S the lowest k; a ballot ends the search at the first step that accepted a candidate.  Lanes past K
// hold no candidate: they are never accepted.  The winner's offset is recomputed from its direction (the same operations on the
// same values: the same bits), so nothing but the key crosses lanes.  Nothing is culled: every candidate is measured against
// every primitive, as the numpy reference does.  No atomics reach an output.  Work counts (COUNT instantiations only):
// wave-uniform 64-bit sums, ONE vector atomic per wave at the end.
//
// probe_grid_states_kernel.  The corner-packed body of srt_probe_grid.hip.h (probe_grid_shade, described there) with the probe
// records switched on (rules 3s and 4s).  DEPTH: rule 7b as probe_grid_depth_kernel applies it; without it the call is
// srt_shade_probe_grid without SRT_PROBE_GRID_VISIBILITY (segments and open stay 0).  It traces nothing and stages no scene;
// 16 KiB of static LDS.
#pragma once

#include "srt_kernel.hip.h"
#include "srt_probe_depth.hip.h"

namespace srt {

enum { PS_WORK_PROBES = 0, PS_WORK_INSIDE, PS_WORK_MOVED, PS_WORK_BURIED, PS_WORK_IDLE, PS_WORK_CANDIDATES, PS_WORK_WAVES, PS_WORK_N };
enum : uint32_t { PS_MOVED = 1u, PS_BURIED = 2u, PS_INSIDE = 4u, PS_IDLE = 8u };
constexpr uint32_t PS_TABLE_LDS_VEC4 = 2048;  // a table of up to 32 KiB is staged into LDS

struct ProbeClassifyIO {
    const float4* table;       // [spheres] (c.xyz, |r|), then [boxes][2] (c.xyz, 0), (h.xyz, 0)
    const float4* direction;   // [directions] (d.xyz, ignored); NULL without relocate
    uint32_t spheres, boxes;
    uint32_t directions;       // K, 1 .. 4096 (0 without relocate)
    uint32_t probes;           // P = nx * ny * nz <= 2^30
    float origin[3], spacing[3];
    int32_t counts[3];
    float clearance, max_offset;
    uint32_t steps;            // 1 .. 64
    uint32_t relocate, normalize, has_mesh;
    float4* records;           // [P] (o.xyz, state bits) (NULL: not requested)
    float4* positions;         // [P] (g + o, 0) (NULL: not requested)
    unsigned long long* work;  // COUNT: [PS_WORK_N] totals of the launch (zeroed by the host before it)
};

// rule S1: the scene distance at x.  T is read at addresses every lane of the wave shares.
__device__ __forceinline__ float probe_scene_distance(const float4* T, uint32_t ns, uint32_t nb, float x, float y, float z) {
    float S = __builtin_inff();
    for (uint32_t i = 0; i < ns; ++i) {
        const float4 s = T[i];
        const float ex = x - s.x, ey = y - s.y, ez = z - s.z;
        const float D = sqrtf((ex * ex + ey * ey) + ez * ez);
        const float sd = D - s.w;
        S = sd < S ? sd : S;  // (a NaN is ignored)
    }
    const float4* B = T + ns;
    for (uint32_t i = 0; i < nb; ++i) {
        const float4 c = B[2 * i], h = B[2 * i + 1];
        const float qx = fabsf(x - c.x) - h.x, qy = fabsf(y - c.y) - h.y, qz = fabsf(z - c.z) - h.z;
        const float mx = qx > 0.0f ? qx : 0.0f, my = qy > 0.0f ? qy : 0.0f, mz = qz > 0.0f ? qz : 0.0f;
        const float outside = sqrtf((mx * mx + my * my) + mz * mz);
        const float qxy = qx > qy ? qx : qy;
        const float qm = qxy > qz ? qxy : qz;
        const float sd = outside + (qm < 0.0f ? qm : 0.0f);
        S = sd < S ? sd : S;
    }
    return S;
}

template <bool TABLE_LDS, bool COUNT>
__global__ void __launch_bounds__(WG_THREADS) probe_classify_kernel(const ProbeClassifyIO io) {
    extern __shared__ float4 lds_probe_table[];
    const uint32_t ns = io.spheres, nb = io.boxes;
    if constexpr (TABLE_LDS) {  // (ns + 2 nb <= PS_TABLE_LDS_VEC4: the host chose this instantiation)
        const uint32_t n = ns + 2u * nb;
        for (uint32_t i = threadIdx.x; i < n; i += WG_THREADS) lds_probe_table[i] = io.table[i];
        __syncthreads();
    }
    const float4* const T = TABLE_LDS ? (const float4*)lds_probe_table : io.table;
    constexpr int WAVES = WG_TILES_X * WG_TILES_Y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long n_probes = 0ull, n_inside = 0ull, n_moved = 0ull, n_buried = 0ull, n_idle = 0ull, n_cand = 0ull;
    const uint32_t nx = (uint32_t)io.counts[0], ny = (uint32_t)io.counts[1];
    const float sx = io.spacing[0], sy = io.spacing[1], sz = io.spacing[2];
    // rule S2
    const float sxy = sx < sy ? sx : sy;
    const float smin = sxy < sz ? sxy : sz;
    const float margin = io.clearance * smin;
    const float reach = sqrtf((sx * sx + sy * sy) + sz * sz);
    const float idle_from = 1.0625f * reach;
    const float dt = io.max_offset / (float)io.steps;
    const uint32_t K = io.directions, J = (K + 63u) >> 6;
    const bool relocate = io.relocate != 0u, norm = io.normalize != 0u, has_mesh = io.has_mesh != 0u;  // (kernel arguments: wave-uniform)
    for (uint32_t p = blockIdx.x * (uint32_t)WAVES + (uint32_t)wave; p < io.probes; p += gridDim.x * (uint32_t)WAVES) {
        const uint32_t ix = p % nx, rest = p / nx, iy = rest % ny, iz = rest / ny;
        const float gx = io.origin[0] + (float)ix * sx, gy = io.origin[1] + (float)iy * sy, gz = io.origin[2] + (float)iz * sz;  // probe-grid rule 4
        const float s0 = probe_scene_distance(T, ns, nb, gx, gy, gz);  // rule S3
        const bool inside = s0 < 0.0f;
        uint32_t state = inside ? (PS_BURIED | PS_INSIDE) : 0u;
        float ox = 0.0f, oy = 0.0f, oz = 0.0f;
        if (relocate && s0 < margin) {  // rule S4 (wave-uniform)
            for (uint32_t m = 1; m <= io.steps; ++m) {
                const float t = (float)m * dt;
                float best = -__builtin_inff();
                uint32_t best_k = 0xffffffffu;
                for (uint32_t j = 0; j < J; ++j) {
                    const uint32_t k = (j << 6) + (uint32_t)lane;
                    const bool active = k < K;
                    float4 d4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // (a lane past K holds no candidate)
                    if (active) d4 = io.direction[k];
                    V3 d = v3(d4.x, d4.y, d4.z);
                    if (norm) d = normalized_ieee(d);
                    const float cx = gx + (d.x * t) * sx, cy = gy + (d.y * t) * sy, cz = gz + (d.z * t) * sz;
                    const float S = probe_scene_distance(T, ns, nb, cx, cy, cz);
                    if (active && S >= margin && S > best) best = S, best_k = k;  // (ascending k: the lowest k of equal S stays)
                }
                n_cand += (unsigned long long)K;
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {  // the largest S of the wave, on equal S the lowest k: every lane ends with it
                    const float oS = __shfl_xor(best, off, 64);
                    const uint32_t oK = (uint32_t)__shfl_xor((int)best_k, off, 64);
                    if (oS > best || (oS == best && oK < best_k)) best = oS, best_k = oK;
                }
                if (__builtin_amdgcn_ballot_w64(best_k != 0xffffffffu) != 0ull) {  // the first step that accepted a candidate
                    const uint32_t kw = (uint32_t)__builtin_amdgcn_readfirstlane((int)best_k);  // (< K)
                    const float4 d4 = io.direction[kw];
                    V3 d = v3(d4.x, d4.y, d4.z);
                    if (norm) d = normalized_ieee(d);
                    ox = (d.x * t) * sx, oy = (d.y * t) * sy, oz = (d.z * t) * sz;
                    state = PS_MOVED | (inside ? PS_INSIDE : 0u);
                    break;
                }
            }
        }
        if (state == 0u && !has_mesh && s0 > idle_from) state = PS_IDLE;
        if (lane == 0) {
            if (io.records) io.records[p] = make_float4(ox, oy, oz, __uint_as_float(state));
            if (io.positions) io.positions[p] = make_float4(gx + ox, gy + oy, gz + oz, 0.0f);
        }
        if constexpr (COUNT) {
            n_probes += 1ull;
            n_inside += (state & PS_INSIDE) ? 1ull : 0ull, n_moved += (state & PS_MOVED) ? 1ull : 0ull;
            n_buried += (state & PS_BURIED) ? 1ull : 0ull, n_idle += (state & PS_IDLE) ? 1ull : 0ull;
        }
    }
    if constexpr (COUNT) {  // the wave's sums: lane k adds counter k — one vector atomic per wave
        unsigned long long v = 0ull;
        v = lane == PS_WORK_PROBES ? n_probes : v;
        v = lane == PS_WORK_INSIDE ? n_inside : v;
        v = lane == PS_WORK_MOVED ? n_moved : v;
        v = lane == PS_WORK_BURIED ? n_buried : v;
        v = lane == PS_WORK_IDLE ? n_idle : v;
        v = lane == PS_WORK_CANDIDATES ? n_cand : v;
        v = lane == PS_WORK_WAVES ? 1ull : v;
        if (lane < PS_WORK_N) atomicAdd(&io.work[lane], v);
    }
}

static_assert(PG_STATE_BURIED == PS_BURIED, "srt_probe_grid.hip.h and srt_probe_states.hip.h disagree");

// srt_shade_probe_grid_states: probe_grid_shade with the records, and rule 7b (DEPTH) or no test; 16 KiB of static LDS
template <bool DEPTH, bool COUNT>
__global__ void __launch_bounds__(WG_THREADS) probe_grid_states_kernel(const KernelParams P, const ProbeGridIO io) {
    constexpr int WAVES = WG_TILES_X * WG_TILES_Y;
    __shared__ float pix_records[WAVES][64 * PG_REC];
    __shared__ float4 result_slots[WAVES][64];
    const int wave = threadIdx.x >> 6;
    probe_grid_shade<true, DEPTH ? PgTest::MOMENTS : PgTest::NONE, COUNT>(P, io, pix_records[wave], result_slots[wave]);
}

}  // namespace srt
