// srt_probe_cascade.hip.h — gfx950 probe-cascade shading (srt_shade_probe_cascade): per-pixel irradiance from up to four nested
// probe grids, the finest level that holds the pixel's first hit blended into the next coarser one across a border band.  The
// header block of srt_pathtrace.h (rules C1 - C5) is the contract; this file restates it.  Everything is binary32 without
// contraction.
//
// Per level the pass computes what probe_grid_shade (srt_probe_grid.hip.h) computes on that level's grid and arrays — rules 1 - 9
// of the probe-grid block with 3s / 4s (STATES) and 7b (DEPTH), through the same device functions probe_grid_cell,
// probe_depth_weigh and probe_grid_irradiance — so one level gives the single-grid call's bits.  It is a body of its own:
// probe_grid_shade is not touched.
//
// Shape: persistent workgroups of four waves, each wave strides over 8 x 8 tiles of the band, as probe_grid_states_kernel.  The
// hit pixels are ranked in lane order (ballot + mbcnt).  VARIABLE ITEMS PER PIXEL: each hit pixel finds its first level f, its
// weight beta and its evaluation count k in {1, 2} (rule C2); the exclusive scan of k over the ranks — rank plus the number of
// two-evaluation hit pixels in lower lanes, one more mbcnt — is the pixel's first evaluation index q, and Q = h + (pixels with two)
// is the tile's evaluation count.  The pixel leaves origin and normal in pixel record `rank` (6 floats) and per evaluation a record
// of 7 words (level and owner rank in one word, three cell indices, three fractions) at q and q + 1.  Items are numbered
// j = 8 q' + c: trip t gives lane l corner l & 7 of evaluation 8 t + (l >> 3), so a trip serves eight evaluations and a tile
// takes ceil(Q / 8) trips.  Results come back through 64 float4 LDS slots per wave; the owner adds the eight slots of each of its
// evaluations in ascending c, separately per evaluation (rule C1), then combines (rule C3).  No atomics on outputs, no order left
// to the hardware.
// LEVEL TABLE: lanes of one trip belong to different levels, so grid and array pointers are read per lane from a 4 x 64-byte table
// in LDS that thread 0 fills once per workgroup from the kernel argument (static indices: no select chains, no scratch).
// LDS per wave: 64 x 6 + 128 x 7 words + 64 float4 = 6144 bytes; per workgroup 24576 + 256 of table = 24832 bytes, static.
// SAFETY (rule C4): every coefficient, moment and record index is built from cell indices clamped to [0, n_a - 1] per axis and a
// level in [0, levels - 1]; a record's level and rank words are written by this wave only.
// Work counts (COUNT instantiations only): per-wave scalar sums and ONE vector atomic per wave at the end.
#pragma once

#include "srt_probe_grid.hip.h"

namespace srt {

enum {
    PC_WORK_PIXELS = 0,
    PC_WORK_EVALUATIONS,
    PC_WORK_BLENDED,
    PC_WORK_FIRST0,  // .. PC_WORK_FIRST0 + 3
    PC_WORK_CORNERS = PC_WORK_FIRST0 + 4,
    PC_WORK_OPEN,
    PC_WORK_TRIPS,
    PC_WORK_WAVES,
    PC_WORK_N
};
constexpr int PC_LEVELS = 4;      // SRT_PROBE_CASCADE_MAX_LEVELS
constexpr int PC_PIX_REC = 6;     // floats per pixel record: origin 0..2, normal 3..5
constexpr int PC_EVAL_REC = 7;    // words per evaluation record: level | rank << 8, cell index 1..3 (int bits), fraction 4..6
constexpr int PC_EVALS = 128;     // evaluation records per wave: two per pixel of a tile

// one level: 64 bytes, as it lies in the kernel argument and in LDS
struct ProbeCascadeLevel {
    float origin[3], spacing[3];
    int32_t counts[3];
    uint32_t pad;
    const float4* coefficients;  // [P][9]
    const float4* depth;         // DEPTH: [P][R*R]
    const float4* states;        // STATES: [P]
};

struct ProbeCascadeIO {
    const int32_t* object;       // SRT_GBUF_OBJECT: -1 = miss
    const float4* normal_depth;  // SRT_GBUF_NORMAL_DEPTH: xyz = normal
    const float4* position;      // SRT_GBUF_POSITION: xyz = point
    const float4* albedo;        // SRT_GBUF_ALBEDO; NULL without SRT_PROBE_CASCADE_ALBEDO
    float4* out;                 // W * H
    ProbeCascadeLevel level[PC_LEVELS];  // entries >= levels are zero and never read
    uint32_t levels;             // 1 .. 4
    uint32_t resolution;         // DEPTH: R: 4, 8 or 16
    float blend_cells;
    float band_weight[3];
    uint32_t normal_weight;      // SRT_PROBE_CASCADE_NORMAL_WEIGHT
    float bias, min_variance;    // DEPTH
    unsigned long long* work;    // COUNT: [PC_WORK_N] totals of the launch (zeroed by the host before it)
};

// rule C2 on one axis of one level: false when the point is outside (or NaN); otherwise e takes the distance to the nearer face
__device__ __forceinline__ bool probe_cascade_axis(float x, float origin, float spacing, int n, float& e) {
    if (n < 2) return true;
    const float m = (float)(n - 1);
    const float u = (x - origin) / spacing;  // rule 2's expression before its clamp
    if (!(u >= 0.0f && u <= m)) return false;
    const float g = m - u;
    const float ea = u < g ? u : g;
    e = ea < e ? ea : e;
    return true;
}

template <bool DEPTH, bool STATES, bool COUNT>
__global__ void __launch_bounds__(WG_THREADS) probe_cascade_kernel(const KernelParams P, const ProbeCascadeIO io) {
    constexpr int WAVES = WG_TILES_X * WG_TILES_Y;
    __shared__ ProbeCascadeLevel table[PC_LEVELS];
    __shared__ float pix_records[WAVES][64 * PC_PIX_REC];
    __shared__ float eval_records[WAVES][PC_EVALS * PC_EVAL_REC];
    __shared__ float4 result_slots[WAVES][64];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int l = 0; l < PC_LEVELS; ++l) table[l] = io.level[l];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* const pixrec = pix_records[wave];
    float* const evrec = eval_records[wave];
    float4* const slots = result_slots[wave];
    unsigned long long trips_done = 0ull, pixels = 0ull, evaluations = 0ull, blended = 0ull, corners = 0ull, open = 0ull;
    unsigned long long first0 = 0ull, first1 = 0ull, first2 = 0ull, first3 = 0ull;
    const int W = P.width;
    const int tiles_x = (W + TILE_W - 1) / TILE_W, tiles_y = (P.rows + TILE_H - 1) / TILE_H;
    const int tiles = tiles_x * tiles_y;
    const bool weigh = io.normal_weight != 0u;  // (a kernel argument: wave-uniform)
    const int levels = (int)io.levels;
    const float blend = io.blend_cells;
    const int cx = lane & 1, cy = (lane >> 1) & 1, cz = (lane >> 2) & 1;  // this lane's corner: c = lane & 7 in every trip
    const int R = DEPTH ? (int)io.resolution : 1;
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
        // rule C2: the first level f, its weight beta, one or two evaluations (the level loop is wave-uniform: broadcast LDS reads)
        int f = -1;
        float beta = 0.0f;
        for (int l = 0; l < levels; ++l) {
            const ProbeCascadeLevel& g = table[l];
            float e = __builtin_inff();
            bool inside = probe_cascade_axis(xp.x, g.origin[0], g.spacing[0], g.counts[0], e);
            inside = probe_cascade_axis(xp.y, g.origin[1], g.spacing[1], g.counts[1], e) && inside;
            inside = probe_cascade_axis(xp.z, g.origin[2], g.spacing[2], g.counts[2], e) && inside;
            const float b = !inside ? 0.0f : (e >= blend ? 1.0f : e / blend);
            if (f < 0 && b > 0.0f) f = l, beta = b;
        }
        if (f < 0) f = levels - 1;
        const bool two = hit && f != levels - 1 && !(beta >= 1.0f);
        const unsigned long long tmask = __builtin_amdgcn_ballot_w64(two);
        const int q = rank + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(tmask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)tmask, 0u));  // the exclusive scan of k
        const int Q = h + __builtin_popcountll(tmask);
        const int trips = (Q + 7) >> 3;
        if (trips > 0) {  // the pixel of rank r leaves what its corners need: one pixel record, one or two evaluation records
            const float ofs = .00001f;
            __builtin_amdgcn_wave_barrier();
            if (hit) {
                float* rec = pixrec + rank * PC_PIX_REC;
                rec[0] = xp.x + nd.x * ofs, rec[1] = xp.y + nd.y * ofs, rec[2] = xp.z + nd.z * ofs;
                rec[3] = nd.x, rec[4] = nd.y, rec[5] = nd.z;
                for (int k = 0; k < (two ? 2 : 1); ++k) {
                    const int l = f + k;  // (<= levels - 1: two only when f != levels - 1)
                    const ProbeCascadeLevel& g = table[l];
                    int i0, i1, i2;
                    float f0, f1, f2;
                    probe_grid_cell(xp.x, g.origin[0], g.spacing[0], g.counts[0], i0, f0);
                    probe_grid_cell(xp.y, g.origin[1], g.spacing[1], g.counts[1], i1, f1);
                    probe_grid_cell(xp.z, g.origin[2], g.spacing[2], g.counts[2], i2, f2);
                    float* ev = evrec + (q + k) * PC_EVAL_REC;
                    ev[0] = __int_as_float(l | (rank << 8));
                    ev[1] = __int_as_float(i0), ev[2] = __int_as_float(i1), ev[3] = __int_as_float(i2);
                    ev[4] = f0, ev[5] = f1, ev[6] = f2;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        if constexpr (COUNT) {
            pixels += (unsigned long long)h, evaluations += (unsigned long long)Q, blended += (unsigned long long)__builtin_popcountll(tmask);
            first0 += (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(hit && f == 0));
            first1 += (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(hit && f == 1));
            first2 += (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(hit && f == 2));
            first3 += (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(hit && f == 3));
        }
        float A0 = 0.0f, A1 = 0.0f, A2 = 0.0f, AT = 0.0f;  // evaluation q: level f
        float B0 = 0.0f, B1 = 0.0f, B2 = 0.0f, BT = 0.0f;  // evaluation q + 1: level f + 1
        for (int trip = 0; trip < trips; ++trip) {
            const int ei = (trip << 3) + (lane >> 3);  // item 64 trip + lane = 8 ei + c
            const bool item = ei < Q;
            const float* ev = evrec + (item ? ei : 0) * PC_EVAL_REC;
            const int lr = __float_as_int(ev[0]);
            const int l = min(max(lr & 0xff, 0), levels - 1), r = (lr >> 8) & 63;
            const int i0 = __float_as_int(ev[1]), i1 = __float_as_int(ev[2]), i2 = __float_as_int(ev[3]);
            const float f0 = ev[4], f1 = ev[5], f2 = ev[6];
            const float* rec = pixrec + r * PC_PIX_REC;
            const V3 o = v3(rec[0], rec[1], rec[2]);
            const V3 pn = v3(rec[3], rec[4], rec[5]);
            const ProbeCascadeLevel& g = table[l];
            const int nx = g.counts[0], ny = g.counts[1], nz = g.counts[2];
            // rule 3: the trilinear weight
            const float w0 = cx ? f0 : (1.0f - f0), w1 = cy ? f1 : (1.0f - f1), w2 = cz ? f2 : (1.0f - f2);
            float tw = (w0 * w1) * w2;
            bool live = item && tw > 0.0f;  // (a NaN fails)
            // the corner's probe, clamped per axis: in [0, n_a - 1] whatever the record holds
            const int k0 = min(max(i0 + cx, 0), nx - 1), k1 = min(max(i1 + cy, 0), ny - 1), k2 = min(max(i2 + cz, 0), nz - 1);
            const size_t probe = (size_t)k0 + (size_t)nx * ((size_t)k1 + (size_t)ny * (size_t)k2);
            // rule 4: the probe; rule 5: the segment to it
            V3 p = v3(g.origin[0] + (float)(i0 + cx) * g.spacing[0], g.origin[1] + (float)(i1 + cy) * g.spacing[1], g.origin[2] + (float)(i2 + cz) * g.spacing[2]);
            if constexpr (STATES) {  // rule 3s: a buried probe is skipped and enters no counter; rule 4s: the others stand where they were moved to
                float4 st = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (live) st = g.states[probe];  // 16-byte load
                live = live && !(__float_as_uint(st.w) & PG_STATE_BURIED);
                p = v3(p.x + st.x, p.y + st.y, p.z + st.z);
            }
            const V3 v = v3(p.x - o.x, p.y - o.y, p.z - o.z);
            const float qq = (v.x * v.x + v.y * v.y) + v.z * v.z;
            const float L = sqrtf(qq);
            live = live && L > 0.0f;
            const V3 d = v3(v.x / L, v.y / L, v.z / L);
            if (weigh) {  // rule 6
                const float hh = (((d.x * pn.x + d.y * pn.y) + d.z * pn.z) + 1.0f) * 0.5f;
                tw = tw * ((hh * hh) + 0.2f);
            }
            bool ok = live;
            if constexpr (DEPTH) {
                ok = false;
                if (live) {  // rule 7b
                    tw = probe_depth_weigh(g.depth + probe * (size_t)(R * R), R, d, L, io.bias, io.min_variance, tw);
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
                const V3 e = probe_grid_irradiance(g.coefficients + probe * (size_t)PG_COEFFS, pn, io.band_weight);
                res = make_float4(tw * e.x, tw * e.y, tw * e.z, tw);
            }
            // rule 9 per evaluation: the owner adds the eight corners of each of its evaluations in ascending c
            slots[lane] = res;
            __builtin_amdgcn_wave_barrier();
            if (hit && (q >> 3) == trip) {
                const float4* mine = slots + ((q & 7) << 3);
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float4 s = mine[c];
                    A0 = A0 + s.x, A1 = A1 + s.y, A2 = A2 + s.z, AT = AT + s.w;
                }
            }
            if (two && ((q + 1) >> 3) == trip) {
                const float4* mine = slots + (((q + 1) & 7) << 3);
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float4 s = mine[c];
                    B0 = B0 + s.x, B1 = B1 + s.y, B2 = B2 + s.z, BT = BT + s.w;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (in_range) {  // rule C3
            float4 o4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (hit) {
                const bool ua = AT > 0.0f, ub = two && BT > 0.0f;
                float4 ia = make_float4(0.0f, 0.0f, 0.0f, 0.0f), ib = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (ua) ia = make_float4(A0 / AT, A1 / AT, A2 / AT, AT);
                if (ub) ib = make_float4(B0 / BT, B1 / BT, B2 / BT, BT);
                if (ua && ub) {
                    const float gb = 1.0f - beta;
                    o4 = make_float4((beta * ia.x) + (gb * ib.x), (beta * ia.y) + (gb * ib.y), (beta * ia.z) + (gb * ib.z), (beta * ia.w) + (gb * ib.w));
                } else if (ua) {
                    o4 = ia;
                } else if (ub) {
                    o4 = ib;
                }
                if (io.albedo && (ua || ub)) o4.x = o4.x * alb.x, o4.y = o4.y * alb.y, o4.z = o4.z * alb.z;
            }
            io.out[pix] = o4;
        }
    }
    if constexpr (COUNT) {  // the wave's sums: lane k adds counter k — one vector atomic per wave
        unsigned long long v = 0ull;
        v = lane == PC_WORK_PIXELS ? pixels : v;
        v = lane == PC_WORK_EVALUATIONS ? evaluations : v;
        v = lane == PC_WORK_BLENDED ? blended : v;
        v = lane == PC_WORK_FIRST0 ? first0 : v;
        v = lane == PC_WORK_FIRST0 + 1 ? first1 : v;
        v = lane == PC_WORK_FIRST0 + 2 ? first2 : v;
        v = lane == PC_WORK_FIRST0 + 3 ? first3 : v;
        v = lane == PC_WORK_CORNERS ? corners : v;
        v = lane == PC_WORK_OPEN ? open : v;
        v = lane == PC_WORK_TRIPS ? trips_done : v;
        v = lane == PC_WORK_WAVES ? 1ull : v;
        if (lane < PC_WORK_N) atomicAdd(&io.work[lane], v);
    }
}

}  // namespace srt
