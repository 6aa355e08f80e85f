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
// probe_grid_states_kernel.  probe_grid_depth_kernel's corner-packed scheme (srt_probe_depth.hip.h, which stays as it is: this is a
// sibling that reuses probe_grid_cell and probe_depth_texel_axis) with rules 3s and 4s: one 16-byte load of the corner probe's
// record; a BURIED probe is skipped before rule 5 and enters no counter, and every other probe stands at its grid position plus
// the record's offset.  DEPTH: rule 7b as probe_grid_depth_kernel applies it; without it the call is srt_shade_probe_grid without
// SRT_PROBE_GRID_VISIBILITY (segments and open stay 0).  It traces nothing and stages no scene; 16 KiB of static LDS.
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

struct ProbeGridStatesIO {
    const int32_t* object;       // SRT_GBUF_OBJECT: -1 = miss
    const float4* normal_depth;  // SRT_GBUF_NORMAL_DEPTH: xyz = normal
    const float4* position;      // SRT_GBUF_POSITION: xyz = point
    const float4* albedo;        // SRT_GBUF_ALBEDO; NULL without SRT_PROBE_GRID_ALBEDO
    const float4* coefficients;  // [nx * ny * nz][9]
    const float4* depth;         // DEPTH: [nx * ny * nz][R*R]: SRT_PROBE_DEPTH_MOMENTS' layout
    const float4* states;        // [nx * ny * nz] (o.xyz, state bits): SRT_PROBE_STATE_RECORDS' layout
    float4* out;                 // W * H
    float origin[3], spacing[3];
    int32_t counts[3];
    float band_weight[3];
    uint32_t normal_weight;      // SRT_PROBE_GRID_NORMAL_WEIGHT
    uint32_t resolution;         // DEPTH: R: 4, 8 or 16
    float bias, min_variance;    // DEPTH
    unsigned long long* work;    // COUNT: [PG_WORK_N] totals of the launch (zeroed by the host before it)
};

// One launch covers scene rows [P.y0, P.y0 + P.rows); buffers are indexed x + y * width with the SCENE row y, as the G-buffer.
// Of P only width, rows and y0 are read.
template <bool DEPTH, bool COUNT>
__global__ void __launch_bounds__(WG_THREADS) probe_grid_states_kernel(const KernelParams P, const ProbeGridStatesIO io) {
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
    const int R = DEPTH ? (int)io.resolution : 1;
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
            // clamped per axis: in [0, n_a - 1] whatever the record holds
            const int k0 = min(max(i0 + cx, 0), nx - 1), k1 = min(max(i1 + cy, 0), ny - 1), k2 = min(max(i2 + cz, 0), nz - 1);
            const size_t probe = (size_t)k0 + (size_t)nx * ((size_t)k1 + (size_t)ny * (size_t)k2);
            // rule 3s: the probe's record; a buried probe is skipped and enters no counter
            float4 st = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (live) st = io.states[probe];  // 16-byte load
            live = live && !(__float_as_uint(st.w) & PS_BURIED);
            // rule 4s: the probe where it was moved to; rule 5: the segment to it
            const V3 p = v3((io.origin[0] + (float)(i0 + cx) * io.spacing[0]) + st.x, (io.origin[1] + (float)(i1 + cy) * io.spacing[1]) + st.y,
                            (io.origin[2] + (float)(i2 + cz) * io.spacing[2]) + st.z);
            const V3 v = v3(p.x - o.x, p.y - o.y, p.z - o.z);
            const float q = (v.x * v.x + v.y * v.y) + v.z * v.z;
            const float L = sqrtf(q);
            live = live && L > 0.0f;
            const V3 d = v3(v.x / L, v.y / L, v.z / L);
            if (weigh) {  // rule 6
                const float hh = (((d.x * pn.x + d.y * pn.y) + d.z * pn.z) + 1.0f) * 0.5f;
                tw = tw * ((hh * hh) + 0.2f);
            }
            bool ok = live;
            if constexpr (DEPTH) {
                ok = false;
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
            }
            if constexpr (COUNT) {
                corners += (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(live));
                if constexpr (DEPTH) open += (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(ok));
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
        v = lane == PG_WORK_SEGMENTS ? (DEPTH ? corners : 0ull) : v;
        v = lane == PG_WORK_OPEN ? open : v;
        v = lane == PG_WORK_TRIPS ? trips_done : v;
        v = lane == PG_WORK_WAVES ? 1ull : v;
        if (lane < PG_WORK_N) atomicAdd(&io.work[lane], v);
    }
}

}  // namespace srt
