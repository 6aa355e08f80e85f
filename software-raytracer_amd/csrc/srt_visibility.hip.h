// srt_visibility.hip.h — gfx950 per-pixel visibility (srt_render_visibility): ambient occlusion and sun visibility from the
// first-hit buffers.  Per pixel with a hit (OBJECT != -1) the kernel starts at the bounce origin of Raytracer.cpp:177,
// x + n * .00001f, and asks any_hit (srt_occlusion.hip.h, unchanged)
//   AO:  for samples f = f0 .. f0 + n - 1, is the segment along the hemisphere direction that srt_render's sample f draws before
//        its first bounce (draws 1..3 of srt_rng_key(seed, pixel, f): GetRandomNormalOrientedHemisphere, :90-105, through
//        normalized_in_window as the path tracer) free up to ao_radius?  ao = (float)open / (float)n.
//   SUN: with s = -sun_direction and c = n . s > 0, is the ray towards the sun free?  sun = free ? c : 0.
// A miss pixel gets (1, 0) and loads no other guide value.  Everything is binary32 without contraction; the AO result is an
// integer count and one IEEE division, so it depends on no order of evaluation.
//
// Launched, sized and staged like gbuffer_kernel: persistent workgroups, make_lds with four waves, each wave strides over 8 x 8
// pixel tiles of the band.  What is new is SEGMENT PACKING.  A tile with h hit pixels has h * n AO segments; n trips with h of 64
// lanes busy would waste most of the wave at silhouettes and in sparse scenes.  Instead the hit pixels are ranked in lane order
// (ballot + mbcnt), the pixel of rank r leaves its origin, normal and RNG key prefix in record r of the wave's pixel records in
// LDS, and the segments are numbered j = r * n + (f - f0): trip t gives lane l segment 64 t + l, whatever pixel it belongs to.
// After a trip ONE ballot of `open` reduces it: the lane that owns rank r adds the population of that ballot masked to lanes
// [r n - 64 t, (r + 1) n - 64 t) ∩ [0, 64).  No atomics, no LDS reduction, deterministic.  The sun segments of a tile are one more
// trip of the same loop — lanes are their own pixels — so any_hit is inlined once.  A tile without hit pixels stores its
// constants and calls nothing.
// Work counts (COUNT instantiations only): as occlusion_kernel, per-wave scalar sums and ONE vector atomic per wave at the end
// into a handle-owned record; segments = n * hits + #{c > 0}, wave_trips = sum over tiles of ceil(h n / 64) + (any c > 0).
#pragma once

#include "srt_occlusion.hip.h"

namespace srt {

enum { VIS_WORK_SEGMENTS = 0, VIS_WORK_OPEN, VIS_WORK_TRIPS, VIS_WORK_ANALYTIC, VIS_WORK_NODES, VIS_WORK_TRIANGLES, VIS_WORK_N };
constexpr int VIS_REC = 12;  // floats per pixel record (Lds::pix): origin 0..2, normal 3..5, key prefix 6

struct VisibilityIO {
    const int32_t* object;       // SRT_GBUF_OBJECT: -1 = miss
    const float4* normal_depth;  // SRT_GBUF_NORMAL_DEPTH: xyz = normal
    const float4* position;      // SRT_GBUF_POSITION: xyz = point
    float* ao;                   // NULL: not asked for
    float* sun;                  // NULL: not asked for
    uint32_t n;                  // AO samples per pixel, 1 .. 4096
    uint32_t first_sample;       // f0
    uint32_t seed;
    float radius;                // t_max of the AO segments
    unsigned long long* work;    // COUNT: [VIS_WORK_N] totals of the launch (zeroed by the host before it)
};

// One launch covers scene rows [P.y0, P.y0 + P.rows); buffers are indexed x + y * width with the SCENE row y, as the G-buffer.
template <bool SCENE_LDS, bool MESH, bool COUNT>
__global__ void __launch_bounds__(WG_THREADS) visibility_kernel(const KernelParams P, const VisibilityIO io) {
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
    constexpr int WAVES = WG_TILES_X * WG_TILES_Y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Lds S = make_lds<SCENE_LDS>(P, lds_scene, WAVES, wave);
    OccWork<COUNT> Wk;  // any_hit's counts; its RAYS / OCCLUDED words carry this kernel's segments / open segments
    unsigned long long trips_done = 0ull;
    const int W = P.width;
    const int tiles_x = (W + TILE_W - 1) / TILE_W, tiles_y = (P.rows + TILE_H - 1) / TILE_H;
    const int tiles = tiles_x * tiles_y;
    const float4 e3 = S.c[CONST_ENV_ROW + 3];
    const V3 sdir = v3(-e3.x, -e3.y, -e3.z);  // s = -sun_direction
    const bool want_ao = io.ao != nullptr, want_sun = io.sun != nullptr;  // (kernel arguments: wave-uniform)
    const int n = (int)io.n;
    const int step_r = 64 / n, step_s = 64 % n;  // a lane's segment number grows by 64 per trip
    const uint32_t key0 = srt_mix32(io.seed ^ 0xA511E9B3U);  // srt_rng_key's first round
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
        float4 nd = make_float4(0.0f, 0.0f, 0.0f, 0.0f), xp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (hit) nd = io.normal_depth[pix], xp = io.position[pix];  // 16-byte loads
        const V3 nrm = v3(nd.x, nd.y, nd.z);
        const float ofs = .00001f;
        const V3 org = v3(xp.x + nrm.x * ofs, xp.y + nrm.y * ofs, xp.z + nrm.z * ofs);  // :177
        const float c = dot3(nrm, sdir);
        const bool lit = hit && c > 0.0f;  // (a NaN fails)
        const unsigned long long hmask = __builtin_amdgcn_ballot_w64(hit);
        const int h = __builtin_popcountll(hmask);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(hmask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)hmask, 0u));
        const int total = want_ao ? h * n : 0;  // <= 64 * 4096
        const int ao_trips = (total + 63) >> 6;
        const int sun_trips = want_sun && __builtin_amdgcn_ballot_w64(lit) != 0ull ? 1 : 0;
        if (ao_trips > 0) {  // the pixel of rank r leaves what its segments need in record r
            __builtin_amdgcn_wave_barrier();
            if (hit) {
                float* rec = S.pix + rank * VIS_REC;
                rec[0] = org.x, rec[1] = org.y, rec[2] = org.z;
                rec[3] = nrm.x, rec[4] = nrm.y, rec[5] = nrm.z;
                rec[6] = __uint_as_float(srt_mix32(key0 + (uint32_t)pix));  // srt_rng_key's second round: pixel = x + y * W, scene coordinates
            }
            __builtin_amdgcn_wave_barrier();
        }
        int open_count = 0;
        bool sun_free = false;
        int seg_r = lane / n, seg_s = lane - seg_r * n;  // segment `lane` of trip 0: rank and sample offset
        for (int trip = 0; trip < ao_trips + sun_trips; ++trip) {
            const bool sun_trip = trip == ao_trips;  // (wave-uniform)
            V3 o = org, d = sdir;
            float t_max = __builtin_inff();
            bool active = lit;
            if (!sun_trip) {
                active = (trip << 6) + lane < total;
                const float* rec = S.pix + (active ? seg_r : 0) * VIS_REC;
                o = v3(rec[0], rec[1], rec[2]);
                const V3 pn = v3(rec[3], rec[4], rec[5]);
                const uint32_t key = srt_mix32(__float_as_uint(rec[6]) + (io.first_sample + (uint32_t)seg_s));  // = srt_rng_key(seed, pixel, f)
                // GetRandomNormalOrientedHemisphere (:90-105): draws 1, 2, 3 of the sample (draw 0 is its specular lottery)
                const uint32_t r1 = srt_mix32(key + 0x9E3779B9U) >> 17;
                const uint32_t r2 = srt_mix32(key + 2u * 0x9E3779B9U) >> 17;
                const uint32_t r3 = srt_mix32(key + 3u * 0x9E3779B9U) >> 17;
                V3 sr = v3((rand_unit(r1) - 0.5f) * 2, (rand_unit(r2) - 0.5f) * 2, (rand_unit(r3) - 0.5f) * 2);
                sr = normalized_in_window(sr);  // (inside normalized()'s window by construction: see there)
                if (dot3(sr, pn) < 0) sr = v3(sr.x * -1, sr.y * -1, sr.z * -1);
                d = sr;
                t_max = io.radius;
            }
            const bool occ = any_hit<MESH, COUNT, SCENE_LDS>(S, P, o, d, t_max, active, Wk);
            const unsigned long long open = __builtin_amdgcn_ballot_w64(active && !occ);
            if constexpr (COUNT) {
                Wk.add(OCC_WORK_RAYS, __builtin_amdgcn_ballot_w64(active));
                Wk.add(OCC_WORK_OCCLUDED, open);
                trips_done += 1ull;
            }
            if (sun_trip) {
                sun_free = active && !occ;
            } else {
                // this pixel's segments in this trip: lanes [rank n - 64 trip, (rank + 1) n - 64 trip) ∩ [0, 64)
                const int lo = rank * n - (trip << 6), hi = lo + n;
                const int a = lo < 0 ? 0 : lo, b = hi > 64 ? 64 : hi;
                if (hit && a < b) {
                    const unsigned long long upto_b = b >= 64 ? ~0ull : ((1ull << b) - 1ull);
                    open_count += __builtin_popcountll(open & upto_b & ~((1ull << a) - 1ull));  // (a <= 63 here)
                }
                seg_r += step_r, seg_s += step_s;
                if (seg_s >= n) seg_s -= n, ++seg_r;
            }
        }
        if (in_range) {
            if (want_ao) io.ao[pix] = hit ? (float)open_count / (float)n : 1.0f;
            if (want_sun) io.sun[pix] = sun_free ? c : 0.0f;
        }
    }
    if constexpr (COUNT) {  // the wave's sums: lane k adds counter k — one vector atomic per wave
        unsigned long long v = 0ull;
        v = lane == VIS_WORK_SEGMENTS ? Wk.n[OCC_WORK_RAYS] : v;
        v = lane == VIS_WORK_OPEN ? Wk.n[OCC_WORK_OCCLUDED] : v;
        v = lane == VIS_WORK_TRIPS ? trips_done : v;
        v = lane == VIS_WORK_ANALYTIC ? Wk.n[OCC_WORK_ANALYTIC] : v;
        v = lane == VIS_WORK_NODES ? Wk.n[OCC_WORK_NODES] : v;
        v = lane == VIS_WORK_TRIANGLES ? Wk.n[OCC_WORK_TRIANGLES] : v;
        if (lane < VIS_WORK_N) atomicAdd(&io.work[lane], v);
    }
}

}  // namespace srt
