// srt_probe_grid.hip.h — gfx950 probe-grid shading: per-pixel irradiance from a regular grid of light probes, read from the first-hit
// buffers.  ONE device body, probe_grid_shade, serves the three calls; their kernels differ in where the LDS comes from and in two
// compile-time choices:
//   probe_grid_kernel         srt_shade_probe_grid, here                           PgTest::QUERY, no records; LDS from make_lds
//   probe_grid_depth_kernel   srt_shade_probe_grid_depth, srt_probe_depth.hip.h    PgTest::MOMENTS, no records; 16 KiB of static LDS
//   probe_grid_states_kernel  srt_shade_probe_grid_states, srt_probe_states.hip.h  PgTest::MOMENTS or NONE, RECORDS; 16 KiB of static LDS
// Per pixel with a hit (OBJECT != -1) the body finds the cell of the point x, and for each of the cell's eight corner probes a
// trilinear weight t.  RECORDS (rules 3s, 4s): one 16-byte load of the corner probe's record; a BURIED probe is skipped before rule
// 5 and enters no counter, and every other probe stands at its grid position plus the record's offset.  The weight is optionally
// scaled by how far the probe lies in front of the surface (SRT_PROBE_GRID_NORMAL_WEIGHT), then the corner test: PgTest::QUERY drops
// the corner when the segment from the bounce origin x + n * .00001f to the probe is occluded (SRT_PROBE_GRID_VISIBILITY: any_hit,
// srt_occlusion.hip.h, unchanged; without the flag the same trips run with no query — a kernel argument, wave-uniform — so any_hit
// is inlined once); PgTest::MOMENTS scales the weight by rule 7b's bound from the probe's depth map; PgTest::NONE does nothing.
// Each surviving corner's nine SH coefficients are evaluated at the normal (srt_light_probe_irradiance's rule with the caller's band
// weights) and the pixel gets sum(t e) / sum(t) with sum(t) in the fourth lane.  A miss pixel gets (0, 0, 0, 0) and loads no other
// guide value.  Everything is binary32 without contraction; the header blocks of srt_pathtrace.h are the rules, this file restates
// them.
//
// Launched and sized like visibility_kernel: persistent workgroups of four waves, each wave strides over 8 x 8 pixel tiles of the
// band.  CORNER PACKING: the hot part is the eight corner items of a hit pixel — a test, 144 bytes of coefficients and 27
// multiply-adds each.  Eight times down one lane would leave the wave as empty as the tile is at a silhouette and serialise the
// loads.  Instead the hit pixels are ranked in lane order (ballot + mbcnt), the pixel of rank r leaves origin, normal, cell and
// fractions in record r of the wave's pixel records in LDS, and the items are numbered j = 8 r + c: trip t gives lane l item
// 64 t + l, so a trip serves eight pixels with one corner per lane, and a tile with h hit pixels takes ceil(h / 8) trips.  RESULTS
// come back through LDS: every lane of a trip stores its (t e.r, t e.g, t e.b, t), or zeros for a skipped corner, into slot `lane`
// of the wave's 64 x float4 result slots, and the lane that owns a pixel of ranks [8 t, 8 t + 8) adds its eight slots in ascending
// c.  No atomics, no order left to the hardware.  probe_grid_kernel takes records and slots from what make_lds already lays out
// (the pixel records and the colour ring: no LDS beyond visibility_kernel's, so the same workgroups per CU).
// Every coefficient, record and moment index is built from cell indices clamped to [0, n_a - 1] per axis: no load can leave the
// arrays whatever the guides hold.
// Work counts (COUNT instantiations only): per-wave scalar sums and ONE vector atomic per wave at the end into a handle-owned record.
#pragma once

#include "srt_occlusion.hip.h"

namespace srt {

enum {
    PG_WORK_PIXELS = 0,
    PG_WORK_CORNERS,
    PG_WORK_SEGMENTS,
    PG_WORK_OPEN,
    PG_WORK_TRIPS,
    PG_WORK_ANALYTIC,
    PG_WORK_NODES,
    PG_WORK_TRIANGLES,
    PG_WORK_WAVES,
    PG_WORK_N
};
constexpr int PG_REC = 12;     // floats per pixel record (Lds::pix): origin 0..2, normal 3..5, cell index 6..8 (int bits), fraction 9..11
constexpr int PG_COEFFS = 9;   // float4 per probe: SRT_LIGHT_PROBE_COEFFICIENTS' layout

struct ProbeGridIO {
    const int32_t* object;       // SRT_GBUF_OBJECT: -1 = miss
    const float4* normal_depth;  // SRT_GBUF_NORMAL_DEPTH: xyz = normal
    const float4* position;      // SRT_GBUF_POSITION: xyz = point
    const float4* albedo;        // SRT_GBUF_ALBEDO; NULL without SRT_PROBE_GRID_ALBEDO
    const float4* coefficients;  // [nx * ny * nz][9]
    float4* out;                 // W * H
    float origin[3], spacing[3];
    int32_t counts[3];
    float band_weight[3];
    uint32_t visibility;         // PgTest::QUERY: SRT_PROBE_GRID_VISIBILITY
    uint32_t normal_weight;      // SRT_PROBE_GRID_NORMAL_WEIGHT
    // what srt_shade_probe_grid does not read (NULL / 0 there) stands behind what it does, and the work record last, where all three
    // kernels had it: with the record in front of these fields the two counting rule-7b kernels took 71 and 73 VGPRs for 52 and 50
    const float4* depth;         // PgTest::MOMENTS: [nx * ny * nz][R*R]: SRT_PROBE_DEPTH_MOMENTS' layout
    const float4* states;        // RECORDS: [nx * ny * nz] (o.xyz, state bits): SRT_PROBE_STATE_RECORDS' layout
    uint32_t resolution;         // PgTest::MOMENTS: R: 4, 8 or 16
    float bias, min_variance;    // PgTest::MOMENTS
    unsigned long long* work;    // COUNT: [PG_WORK_N] totals of the launch (zeroed by the host before it)
};

// what decides, after rule 6, whether a live corner enters the sum
enum class PgTest {
    NONE,     // nothing: every live corner does (segments and open stay 0)
    QUERY,    // rule 7: any_hit on the segment to the probe, behind io.visibility (a kernel argument: wave-uniform); OccWork counts
    MOMENTS,  // rule 7b: Chebyshev's bound from the probe's depth map scales the weight
};
constexpr uint32_t PG_STATE_BURIED = 2u;  // SRT_PROBE_BURIED, the bit of a record's w lane that rule 3s reads

// rule 2 on one axis: the cell index and the fraction of x_a
__device__ __forceinline__ void probe_grid_cell(float x, float origin, float spacing, int n, int& i, float& f) {
    const float m = (float)(n - 1);
    float u = (x - origin) / spacing;
    u = !(u > 0.0f) ? 0.0f : (u > m ? m : u);  // (a NaN gives 0)
    i = (int)u;
    if (n >= 2 && i > n - 2) i = n - 2;
    f = u - (float)i;
}

// rule 7b's texel lookup on one axis: the texel index of the folded octahedral coordinate g
__device__ __forceinline__ int probe_depth_texel_axis(float g, float fr, float top) {
    float a = ((g * 0.5f) + 0.5f) * fr;
    a = !(a > 0.0f) ? 0.0f : (a > top ? top : a);  // (a NaN gives 0)
    return (int)a;
}

// rule 7b: the weight tw of a corner whose probe lies at distance L in direction d, scaled by Chebyshev's bound on "the probe sees
// at least as far as this point" from the two moments of the texel of `map` (the probe's R x R octahedral map) that looks from the
// probe towards the point — one 16-byte load and a dozen operations, whatever the scene holds
__device__ __forceinline__ float probe_depth_weigh(const float4* map, int R, V3 d, float L, float bias, float min_variance, float tw) {
    const float fr = (float)R, top = (float)(R - 1);
    const float qx = -d.x, qy = -d.y, qz = -d.z;
    const float s = (fabsf(qx) + fabsf(qy)) + fabsf(qz);
    float u = qx / s, vv = qy / s;
    if (qz < 0.0f) {
        const float u2 = (1.0f - fabsf(vv)) * (u >= 0.0f ? 1.0f : -1.0f), v2 = (1.0f - fabsf(u)) * (vv >= 0.0f ? 1.0f : -1.0f);
        u = u2, vv = v2;
    }
    const int ti = probe_depth_texel_axis(u, fr, top), tj = probe_depth_texel_axis(vv, fr, top);  // in [0, R - 1]
    const float4 mo = map[(size_t)(tj * R + ti)];  // 16-byte load
    const float m1 = mo.x, m2 = mo.y;
    if (L > m1 + bias) {
        float var = fabsf(m2 - m1 * m1);
        var = var > min_variance ? var : min_variance;
        const float dl = L - m1;
        const float ch = var / (var + dl * dl);
        tw = tw * ((ch * ch) * ch);
    }
    return tw;
}

// rule 8: the irradiance of one probe's nine coefficients `co` at the normal n (srt_light_probe_irradiance's rule with the caller's
// band weights)
__device__ __forceinline__ V3 probe_grid_irradiance(const float4* co, V3 n, const float (&band_weight)[3]) {
    const float bx = n.x, by = n.y, bz = n.z;
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
        const float a = c == 0 ? band_weight[0] : c < 4 ? band_weight[1] : band_weight[2];
        const float4 k = co[c];  // 16-byte load
        const float t0 = (a * k.x) * b[c], t1 = (a * k.y) * b[c], t2 = (a * k.z) * b[c];
        e0 = c == 0 ? t0 : e0 + t0, e1 = c == 0 ? t1 : e1 + t1, e2 = c == 0 ? t2 : e2 + t2;
    }
    return v3(e0, e1, e2);
}

// The body of the three kernels: this wave's tiles of scene rows [P.y0, P.y0 + P.rows); buffers are indexed x + y * width with the
// SCENE row y, as the G-buffer.  `pixrec` ([64][PG_REC]) and `slots` ([64]) are this wave's LDS, wherever the caller has it.  Of P
// only width, rows and y0 are read here; S, SCENE_LDS and MESH are any_hit's (PgTest::QUERY only).
template <bool RECORDS, PgTest TEST, bool COUNT, bool SCENE_LDS = false, bool MESH = false>
__device__ __forceinline__ void probe_grid_shade(const KernelParams& P, const ProbeGridIO& io, float* const pixrec, float4* const slots, const Lds* S = nullptr) {
    constexpr int WAVES = WG_TILES_X * WG_TILES_Y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    OccWork<COUNT && TEST == PgTest::QUERY> Wk;  // any_hit's counts; its RAYS / OCCLUDED words carry the segments / open segments
    unsigned long long trips_done = 0ull, pixels = 0ull, corners = 0ull, open = 0ull;
    const int W = P.width;
    const int tiles_x = (W + TILE_W - 1) / TILE_W, tiles_y = (P.rows + TILE_H - 1) / TILE_H;
    const int tiles = tiles_x * tiles_y;
    const bool query = TEST == PgTest::QUERY && io.visibility != 0u, weigh = io.normal_weight != 0u;  // (kernel arguments: wave-uniform)
    const int nx = io.counts[0], ny = io.counts[1], nz = io.counts[2];
    const int cx = lane & 1, cy = (lane >> 1) & 1, cz = (lane >> 2) & 1;  // this lane's corner: c = lane & 7 in every trip
    const int R = TEST == PgTest::MOMENTS ? (int)io.resolution : 1;
    // wave-uniform loop: every lane of a wave runs the same trips, so any_hit sees all 64 lanes in each call
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
            // the corner's probe, clamped per axis: in [0, n_a - 1] whatever the record holds
            const int k0 = min(max(i0 + cx, 0), nx - 1), k1 = min(max(i1 + cy, 0), ny - 1), k2 = min(max(i2 + cz, 0), nz - 1);
            const size_t probe = (size_t)k0 + (size_t)nx * ((size_t)k1 + (size_t)ny * (size_t)k2);
            // rule 4: the probe; rule 5: the segment to it
            V3 p = v3(io.origin[0] + (float)(i0 + cx) * io.spacing[0], io.origin[1] + (float)(i1 + cy) * io.spacing[1],
                      io.origin[2] + (float)(i2 + cz) * io.spacing[2]);
            if constexpr (RECORDS) {  // rule 3s: a buried probe is skipped and enters no counter; rule 4s: the others stand where they were moved to
                float4 st = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (live) st = io.states[probe];  // 16-byte load
                live = live && !(__float_as_uint(st.w) & PG_STATE_BURIED);
                p = v3(p.x + st.x, p.y + st.y, p.z + st.z);
            }
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
            if constexpr (TEST == PgTest::QUERY) {
                if (query) {  // rule 7 (wave-uniform)
                    const bool occ = any_hit<MESH, COUNT, SCENE_LDS>(*S, P, o, d, L, live, Wk);
                    ok = live && !occ;
                    if constexpr (COUNT) {
                        Wk.add(OCC_WORK_RAYS, __builtin_amdgcn_ballot_w64(live));
                        Wk.add(OCC_WORK_OCCLUDED, __builtin_amdgcn_ballot_w64(ok));
                    }
                }
            } else if constexpr (TEST == PgTest::MOMENTS) {
                ok = false;
                if (live) {  // rule 7b
                    tw = probe_depth_weigh(io.depth + probe * (size_t)(R * R), R, d, L, io.bias, io.min_variance, tw);
                    ok = tw > 0.0f;
                }
            }
            if constexpr (COUNT) {
                corners += (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(live));
                if constexpr (TEST == PgTest::MOMENTS) open += (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(ok));
                trips_done += 1ull;
            }
            // rule 8: the corner's irradiance at the normal
            float4 res = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (ok) {
                const V3 e = probe_grid_irradiance(io.coefficients + probe * (size_t)PG_COEFFS, pn, io.band_weight);
                res = make_float4(tw * e.x, tw * e.y, tw * e.z, tw);
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
    if constexpr (COUNT) {  // the wave's sums: lane k adds counter k — one vector atomic per wave; without a query its three counters stay 0
        unsigned long long v = 0ull;
        v = lane == PG_WORK_PIXELS ? pixels : v;
        v = lane == PG_WORK_CORNERS ? corners : v;
        v = lane == PG_WORK_SEGMENTS ? (TEST == PgTest::MOMENTS ? corners : 0ull) : v;
        v = lane == PG_WORK_OPEN ? open : v;
        v = lane == PG_WORK_TRIPS ? trips_done : v;
        if constexpr (TEST == PgTest::QUERY) {
            v = lane == PG_WORK_SEGMENTS ? Wk.n[OCC_WORK_RAYS] : v;
            v = lane == PG_WORK_OPEN ? Wk.n[OCC_WORK_OCCLUDED] : v;
            v = lane == PG_WORK_ANALYTIC ? Wk.n[OCC_WORK_ANALYTIC] : v;
            v = lane == PG_WORK_NODES ? Wk.n[OCC_WORK_NODES] : v;
            v = lane == PG_WORK_TRIANGLES ? Wk.n[OCC_WORK_TRIANGLES] : v;
        }
        v = lane == PG_WORK_WAVES ? 1ull : v;
        if (lane < PG_WORK_N) atomicAdd(&io.work[lane], v);
    }
}

// srt_shade_probe_grid: the scene image staged and the LDS laid out as visibility_kernel does
template <bool SCENE_LDS, bool MESH, bool COUNT>
__global__ void __launch_bounds__(WG_THREADS) probe_grid_kernel(const KernelParams P, const ProbeGridIO io) {
    extern __shared__ float4 lds_scene[];
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
    const Lds S = make_lds<SCENE_LDS>(P, lds_scene, WG_TILES_X * WG_TILES_Y, threadIdx.x >> 6);
    probe_grid_shade<false, PgTest::QUERY, COUNT, SCENE_LDS, MESH>(P, io, S.pix, S.ring, &S);
}

}  // namespace srt
