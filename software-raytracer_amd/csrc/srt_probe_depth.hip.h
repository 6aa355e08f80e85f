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
// probe_grid_depth_kernel.  probe_grid_kernel's corner-packed scheme (srt_probe_grid.hip.h, which stays as it is: this is a
// sibling that reuses probe_grid_cell) with rule 7b in place of the any-hit query: the corner's probe is weighted by Chebyshev's
// bound on "the probe sees at least as far as this point", from the two moments of the texel that looks from the probe towards
// the point — one 16-byte load and a dozen operations per corner, whatever the scene holds.  It traces nothing, so it stages no
// scene and has one template axis; its LDS is the pixel records and the result slots of its four waves, 16 KiB.
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

struct ProbeGridDepthIO {
    const int32_t* object;       // SRT_GBUF_OBJECT: -1 = miss
    const float4* normal_depth;  // SRT_GBUF_NORMAL_DEPTH: xyz = normal
    const float4* position;      // SRT_GBUF_POSITION: xyz = point
    const float4* albedo;        // SRT_GBUF_ALBEDO; NULL without SRT_PROBE_GRID_ALBEDO
    const float4* coefficients;  // [nx * ny * nz][9]
    const float4* depth;         // [nx * ny * nz][R*R]: SRT_PROBE_DEPTH_MOMENTS' layout
    float4* out;                 // W * H
    float origin[3], spacing[3];
    int32_t counts[3];
    float band_weight[3];
    uint32_t normal_weight;      // SRT_PROBE_GRID_NORMAL_WEIGHT
    uint32_t resolution;         // R: 4, 8 or 16
    float bias, min_variance;
    unsigned long long* work;    // COUNT: [PG_WORK_N] totals of the launch (zeroed by the host before it)
};

// rule 7b's texel lookup on one axis: the texel index of the folded octahedral coordinate g
__device__ __forceinline__ int probe_depth_texel_axis(float g, float fr, float top) {
    float a = ((g * 0.5f) + 0.5f) * fr;
    a = !(a > 0.0f) ? 0.0f : (a > top ? top : a);  // (a NaN gives 0)
    return (int)a;
}

// One launch covers scene rows [P.y0, P.y0 + P.rows); buffers are indexed x + y * width with the SCENE row y, as the G-buffer.
// Of P only width, rows and y0 are read.
template <bool COUNT>
__global__ void __launch_bounds__(WG_THREADS) probe_grid_depth_kernel(const KernelParams P, const ProbeGridDepthIO io) {
    constexpr int WAVES = WG_TILES_X * WG_TILES_Y;
    __shared__ float pix_records[WAVES][64 * PG_REC];
    __shared__ float4 result_slots[WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* const pixrec = pix_records[wave];
    float4* const slots = result_slots[wave];  // [64] the results of a trip
    unsigned long long trips_done = 0ull, pixels = 0ull, corners = 0ull, open = 0ull;
    const int W = P.width;
    const int tiles_x = (W + TILE_W - 1) / TILE_W, tiles_y = (P.rows + TILE_H - 1) / TILE_H;
    const int tiles = tiles_x * tiles_y;
    const bool weigh = io.normal_weight != 0u;  // (a kernel argument: wave-uniform)
    const int nx = io.counts[0], ny = io.counts[1], nz = io.counts[2];
    const int cx = lane & 1, cy = (lane >> 1) & 1, cz = (lane >> 2) & 1;  // this lane's corner: c = lane & 7 in every trip
    const int R = (int)io.resolution;
    const float fr = (float)R, top = (float)(R - 1);
    for (int t = (int)blockIdx.x * WAVES + wave; t < tiles; t += (int)gridDim.x * WAVES) {
        const int tx = t % tiles_x, ty = t / tiles_x;
        const int px = tx * TILE_W + (lane & 7), py = ty * TILE_H + (lane >> 3);
        const bool in_range = px < W && py < P.rows;
        const int x = px, y = P.y0 + py;
        const size_t pix = (size_t)x + (size_t)y * (size_t)W;  // (used by lanes in range only)
        int obj = -1;
        if (in_range) obj = io.object[pix];
        const bool hit = obj != -1;
        // a miss pixel loads none of its other guide values
        float4 nd = make_float4(0.0f, 0.0f, 0.0f, 0.0f), xp = make_float4(0.0f, 0.0f, 0.0f, 0.0f), alb = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (hit) nd = io.normal_depth[pix], xp = io.position[pix];  // 16-byte loads
        if (hit && io.albedo) alb = io.albedo[pix];
        const unsigned long long hmask = __builtin_amdgcn_ballot_w64(hit);
        const int h = __builtin_popcountll(hmask);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(hmask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)hmask, 0u));
        const int trips = (h + 7) >> 3;
        if (trips > 0) {  // the pixel of rank r leaves what its corners need in record r
            const float ofs = .00001f;
            int i0, i1, i2;
            float f0, f1, f2;
            probe_grid_cell(xp.x, io.origin[0], io.spacing[0], nx, i0, f0);
            probe_grid_cell(xp.y, io.origin[1], io.spacing[1], ny, i1, f1);
            probe_grid_cell(xp.z, io.origin[2], io.spacing[2], nz, i2, f2);
            __builtin_amdgcn_wave_barrier();
            if (hit) {
                float* rec = pixrec + rank * PG_REC;
                rec[0] = xp.x + nd.x * ofs, rec[1] = xp.y + nd.y * ofs, rec[2] = xp.z + nd.z * ofs;  // :177
                rec[3] = nd.x, rec[4] = nd.y, rec[5] = nd.z;
                rec[6] = __int_as_float(i0), rec[7] = __int_as_float(i1), rec[8] = __int_as_float(i2);
                rec[9] = f0, rec[10] = f1, rec[11] = f2;
            }
            __builtin_amdgcn_wave_barrier();
        }
        if constexpr (COUNT) pixels += (unsigned long long)h;
        float E0 = 0.0f, E1 = 0.0f, E2 = 0.0f, T = 0.0f;
        for (int trip = 0; trip < trips; ++trip) {
            const int r = (trip << 3) + (lane >> 3);  // item 64 trip + lane = 8 r + c
            const bool item = r < h;
            const float* rec = pixrec + (item ? r : 0) * PG_REC;
            const V3 o = v3(rec[0], rec[1], rec[2]);
            const V3 pn = v3(rec[3], rec[4], rec[5]);
            const int i0 = __float_as_int(rec[6]), i1 = __float_as_int(rec[7]), i2 = __float_as_int(rec[8]);
            const float f0 = rec[9], f1 = rec[10], f2 = rec[11];
            // rule 3: the trilinear weight
            const float w0 = cx ? f0 : (1.0f - f0), w1 = cy ? f1 : (1.0f - f1), w2 = cz ? f2 : (1.0f - f2);
            float tw = (w0 * w1) * w2;
            bool live = item && tw > 0.0f;  // (a NaN fails)
            // rule 4: the probe; rule 5: the segment to it
            const V3 p = v3(io.origin[0] + (float)(i0 + cx) * io.spacing[0], io.origin[1] + (float)(i1 + cy) * io.spacing[1],
                            io.origin[2] + (float)(i2 + cz) * io.spacing[2]);
            const V3 v = v3(p.x - o.x, p.y - o.y, p.z - o.z);
            const float q = (v.x * v.x + v.y * v.y) + v.z * v.z;
            const float L = sqrtf(q);
            live = live && L > 0.0f;
            const V3 d = v3(v.x / L, v.y / L, v.z / L);
            if (weigh) {  // rule 6
                const float hh = (((d.x * pn.x + d.y * pn.y) + d.z * pn.z) + 1.0f) * 0.5f;
                tw = tw * ((hh * hh) + 0.2f);
            }
            // clamped per axis: in [0, n_a - 1] whatever the record holds
            const int k0 = min(max(i0 + cx, 0), nx - 1), k1 = min(max(i1 + cy, 0), ny - 1), k2 = min(max(i2 + cz, 0), nz - 1);
            const size_t probe = (size_t)k0 + (size_t)nx * ((size_t)k1 + (size_t)ny * (size_t)k2);
            bool ok = false;
            if (live) {  // rule 7b: the texel that looks from the probe towards the point
                const float qx = -d.x, qy = -d.y, qz = -d.z;
                const float s = (fabsf(qx) + fabsf(qy)) + fabsf(qz);
                float u = qx / s, vv = qy / s;
                if (qz < 0.0f) {
                    const float u2 = (1.0f - fabsf(vv)) * (u >= 0.0f ? 1.0f : -1.0f), v2 = (1.0f - fabsf(u)) * (vv >= 0.0f ? 1.0f : -1.0f);
                    u = u2, vv = v2;
                }
                const int ti = probe_depth_texel_axis(u, fr, top), tj = probe_depth_texel_axis(vv, fr, top);  // in [0, R - 1]
                const float4 mo = io.depth[probe * (size_t)(R * R) + (size_t)(tj * R + ti)];  // 16-byte load
                const float m1 = mo.x, m2 = mo.y;
                if (L > m1 + io.bias) {
                    float var = fabsf(m2 - m1 * m1);
                    var = var > io.min_variance ? var : io.min_variance;
                    const float dl = L - m1;
                    const float ch = var / (var + dl * dl);
                    tw = tw * ((ch * ch) * ch);
                }
                ok = tw > 0.0f;
            }
            if constexpr (COUNT) {
                corners += (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(live));
                open += (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(ok));
                trips_done += 1ull;
            }
            // rule 8: the corner's irradiance at the normal
            float4 res = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (ok) {
                const float4* co = io.coefficients + probe * (size_t)PG_COEFFS;
                const float bx = pn.x, by = pn.y, bz = pn.z;
                float b[PG_COEFFS];
                b[0] = 0.282095f;
                b[1] = 0.488603f * by;
                b[2] = 0.488603f * bz;
                b[3] = 0.488603f * bx;
                b[4] = 1.092548f * (bx * by);
                b[5] = 1.092548f * (by * bz);
                b[6] = 0.315392f * ((3.0f * (bz * bz)) - 1.0f);
                b[7] = 1.092548f * (bx * bz);
                b[8] = 0.546274f * ((bx * bx) - (by * by));
                float e0 = 0.0f, e1 = 0.0f, e2 = 0.0f;
#pragma unroll
                for (int c = 0; c < PG_COEFFS; ++c) {
                    const float a = c == 0 ? io.band_weight[0] : c < 4 ? io.band_weight[1] : io.band_weight[2];
                    const float4 k = co[c];  // 16-byte load
                    const float t0 = (a * k.x) * b[c], t1 = (a * k.y) * b[c], t2 = (a * k.z) * b[c];
                    e0 = c == 0 ? t0 : e0 + t0, e1 = c == 0 ? t1 : e1 + t1, e2 = c == 0 ? t2 : e2 + t2;
                }
                res = make_float4(tw * e0, tw * e1, tw * e2, tw);
            }
            // rule 9: the owner adds its eight corners in ascending c
            slots[lane] = res;
            __builtin_amdgcn_wave_barrier();
            if (hit && (rank >> 3) == trip) {
                const float4* mine = slots + ((rank & 7) << 3);
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float4 s = mine[c];
                    E0 = E0 + s.x, E1 = E1 + s.y, E2 = E2 + s.z, T = T + s.w;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (in_range) {
            float4 o4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (hit && T > 0.0f) {
                o4 = make_float4(E0 / T, E1 / T, E2 / T, T);
                if (io.albedo) o4.x = o4.x * alb.x, o4.y = o4.y * alb.y, o4.z = o4.z * alb.z;
            }
            io.out[pix] = o4;
        }
    }
    if constexpr (COUNT) {  // the wave's sums: lane k adds counter k — one vector atomic per wave; the three test counters stay 0
        unsigned long long v = 0ull;
        v = lane == PG_WORK_PIXELS ? pixels : v;
        v = lane == PG_WORK_CORNERS ? corners : v;
        v = lane == PG_WORK_SEGMENTS ? corners : v;
        v = lane == PG_WORK_OPEN ? open : v;
        v = lane == PG_WORK_TRIPS ? trips_done : v;
        v = lane == PG_WORK_WAVES ? 1ull : v;
        if (lane < PG_WORK_N) atomicAdd(&io.work[lane], v);
    }
}

}  // namespace srt
