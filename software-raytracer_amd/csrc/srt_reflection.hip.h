// srt_reflection.hip.h — gfx950 reflection guides (srt_render_reflection_gbuffer): per pixel, the camera ray followed through
// the chain of mirror-like surfaces it meets, and the first hit that is NOT one written out as the first-hit buffers write theirs
// — object index, normal + path length, point, albedo — plus the number of reflections J.
//
// Ray 0 is gbuffer_kernel's (GetRayDirection, no jitter); ray j + 1 leaves hit j as srt_render's bounce ray leaves it when the
// material's Lerp weight is 1: float3::Reflect (Common.hpp:163-165), float3::Normalized (:176), origin p + n * .00001f (:177).
// Same closest_hit, scene image, staging and tie rule as gbuffer_kernel; launched and sized like it (persistent workgroups,
// make_lds with four waves, defer_min = 1).
//
// What is new is the REFILLING LANE POOL.  A wave owns the pixel slots of its tiles — the tiles gbuffer_kernel's static stride
// gives it, 64 slots per tile in lane order (x = slot & 7, y = slot >> 3 inside the tile) — as one stream with a wave-uniform
// cursor.  Before every closest_hit call each FREE lane takes the next slot of the stream (ballot + mbcnt: its rank among the
// free lanes); a slot outside the frame or band retires at once without a ray, its lane stays free for this call.  Busy lanes
// carry their chain ray.  All 64 lanes go through ONE closest_hit call with active = has a ray; a lane whose chain stops stores
// its pixel's outputs and is free again.  The loop ends when the stream is empty and no lane is busy.  So while the stream is
// not empty every call has 64 occupied lanes, whatever mix of primaries and chain rays they hold; a plain "trace the tile, then
// loop while any lane is on a mirror" would run every chain step of a tile with only its mirror pixels busy.  Per-lane state
// on top of closest_hit's: pixel index, origin, direction, D, T, J.  Nothing is added to LDS, no atomics reach the outputs, and a
// pixel's value does not depend on which call or lane traced it.
// Work counts (COUNT instantiations only): per-wave scalar sums and ONE vector atomic per wave at the end into a handle-owned
// record, as visibility_kernel.
#pragma once

#include "srt_kernel.hip.h"

namespace srt {

enum { REFL_WORK_PIXELS = 0, REFL_WORK_REFLECTIONS, REFL_WORK_CALLS, REFL_WORK_WAVES, REFL_WORK_N };

// Where the launch writes (NULL: that output was not asked for), indexed x + y * width with the SCENE row y, and the chain's rule.
struct ReflectionIO {
    int32_t* object;           // list index of the terminal object, -1 when the chain leaves the scene
    float4* normal_depth;      // (terminal normal, D = ((t_0 + t_1) + ...) + t_J); left: (0, 0, 0, +inf)
    float4* position;          // (terminal point, 1); left: 0
    float4* albedo;            // (throughput x terminal base colour, 0); left: 0
    int32_t* bounces;          // J
    int32_t max_bounces;       // 0 .. 64
    float min_smoothness;      // follow a hit whose material has smoothness >= this ...
    float min_specular;        // ... and specular_amount >= this (a NaN comparison fails)
    unsigned long long* work;  // COUNT: [REFL_WORK_N] totals of the launch (zeroed by the host before it)
};

// One launch covers scene rows [P.y0, P.y0 + P.rows).
template <bool SCENE_LDS, bool MESH, bool COUNT>
__global__ void __launch_bounds__(WG_THREADS) reflection_kernel(const KernelParams P, const ReflectionIO io) {
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
#if defined(SRT_STATS) && SRT_STATS == 3
    Prof prof{};
#endif
    Tally<false> no_tally;
    const int W = P.width, H = P.height;
    const int tiles_x = (W + TILE_W - 1) / TILE_W, tiles_y = (P.rows + TILE_H - 1) / TILE_H;
    const int tiles = tiles_x * tiles_y;
    const V3 cam = v3(P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]);
    // this wave's stream: tiles first, first + stride, ... (gbuffer_kernel's order), 64 slots each
    const int first = (int)blockIdx.x * WAVES + wave, stride = (int)gridDim.x * WAVES;
    const int my_tiles = first < tiles ? (tiles - first + stride - 1) / stride : 0;
    const long long slots = (long long)my_tiles << 6;  // (64-bit: a frame one pixel wide has eight slots a pixel)
    long long cursor = 0;                              // wave-uniform: slots handed out so far
    // per-lane chain state
    bool busy = false;
    int pix = 0, J = 0;
    V3 o = v3(0.0f, 0.0f, 0.0f), d = v3(0.0f, 0.0f, 1.0f);
    float D = 0.0f, Tr = 0.0f, Tg = 0.0f, Tb = 0.0f;
    unsigned long long n_pixels = 0ull, n_refl = 0ull, n_calls = 0ull;
    // wave-uniform loop: every lane of a wave runs the same trips, so closest_hit sees all 64 lanes in each call
    while (true) {
        const unsigned long long free_mask = __builtin_amdgcn_ballot_w64(!busy);
        if (cursor < slots && free_mask != 0ull) {  // ---- refill: free lane of rank r takes slot cursor + r
            const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(free_mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)free_mask, 0u));
            const long long s = cursor + rank;
            const bool take = !busy && s < slots;
            const int t = first + (take ? (int)(s >> 6) : 0) * stride, l = (int)(s & 63);
            const int tx = t % tiles_x, ty = t / tiles_x;
            const int px = tx * TILE_W + (l & 7), py = ty * TILE_H + (l >> 3);
            const bool start = take && px < W && py < P.rows;  // a slot outside the frame or band retires here, without a ray
            // lanes that start nothing make the nearest pixel's ray with the others (normalized()'s window test is wave-level) and drop it
            const int x = px < W ? px : W - 1, y = P.y0 + (py < P.rows ? py : P.rows - 1);
            // ---- GetRayDirection (Raytracer.cpp:106-122), as gbuffer_kernel ----
            float nX = ((float)x / (float)W) * 2 - 1;
            float nY = ((float)y / (float)H) * 2 - 1;
            V3 u = v3(P.right_rd[0] * nX, P.right_rd[1] * nX, P.right_rd[2] * nX);
            V3 vv = v3(P.up_ld[0] * nY, P.up_ld[1] * nY, P.up_ld[2] * nY);
            const V3 dir = normalized(v3((u.x + vv.x) + P.fwd_clip[0], (u.y + vv.y) + P.fwd_clip[1], (u.z + vv.z) + P.fwd_clip[2]));
            if (start) {
                busy = true;
                pix = x + y * W;  // (W * H < 2^31: srt_create's limit)
                J = 0;
                o = cam, d = dir;
            }
            const int freed = __builtin_popcountll(free_mask);
            cursor = cursor + freed < slots ? cursor + freed : slots;
            if constexpr (COUNT) n_pixels += (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(start));
        }
        const unsigned long long busy_mask = __builtin_amdgcn_ballot_w64(busy);
        if (busy_mask == 0ull) {
            if (cursor >= slots) break;
            continue;  // 64 slots outside the band: nothing to trace, take the next ones
        }
        bool deferred = false;  // (defer_min = 1: every call resolves its mesh rays itself)
        // lanes without a ray carry a harmless unit ray through the wave's rounds
        const Hit h = closest_hit<MESH, false, SCENE_LDS>(S, P, busy ? o : v3(0.0f, 0.0f, 0.0f), busy ? d : v3(0.0f, 0.0f, 1.0f), busy, 1, deferred,
                                                          no_tally SRT_PROF_ARG);
        if constexpr (COUNT) n_calls += 1ull;
        const bool hit = busy && h.prim >= 0;
        float4 m0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), m1 = m0, m2 = m0;
        if (hit) m0 = S.mat(h.prim, 0), m1 = S.mat(h.prim, 1), m2 = S.mat(h.prim, 2);  // (smoothness, specular_amount, base r, g) (base b, ..) (specular rgb, ..)
        if (hit) {
            D = J == 0 ? h.t : D + h.t;
            if (J >= 2) Tr = Tr * 0.8f, Tg = Tg * 0.8f, Tb = Tb * 0.8f;  // the dissipation from the second bounce on (Raytracer.cpp:169-171)
        }
        const bool follow = hit && J < io.max_bounces && m0.x >= io.min_smoothness && m0.y >= io.min_specular;  // (a NaN fails)
        const unsigned long long follow_mask = __builtin_amdgcn_ballot_w64(follow);
        if (busy && !follow) {  // ---- the chain stops here: on h (hit) or by leaving the scene
            if (io.object) io.object[pix] = hit ? S.order(h.prim) : -1;
            if (io.normal_depth) io.normal_depth[pix] = hit ? make_float4(h.n.x, h.n.y, h.n.z, D) : make_float4(0.0f, 0.0f, 0.0f, __builtin_inff());
            if (io.position) io.position[pix] = hit ? make_float4(h.p.x, h.p.y, h.p.z, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (io.albedo) {
                float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (hit) a = J == 0 ? make_float4(m0.z, m0.w, m1.x, 0.0f) : make_float4(Tr * m0.z, Tg * m0.w, Tb * m1.x, 0.0f);
                io.albedo[pix] = a;
            }
            if (io.bounces) io.bounces[pix] = J;
            busy = false;
        }
        if (follow_mask != 0ull) {  // ---- the next ray of the chain
            if (follow) {           // T = base_0, then the mirror's Lerp(base, specular, 1) = specular of every later one
                if (J == 0) Tr = m0.z, Tg = m0.w, Tb = m1.x;
                else Tr = Tr * m2.x, Tg = Tg * m2.y, Tb = Tb * m2.z;
            }
            // float3::Reflect (Common.hpp:163-165); lanes that follow nothing reflect a harmless vector with the others
            const V3 dd = follow ? d : v3(1.0f, 1.0f, 1.0f), nn = follow ? h.n : v3(0.0f, 0.0f, 0.0f);
            const float k = 2 * dot3(dd, nn);
            const V3 r = normalized(v3(dd.x - nn.x * k, dd.y - nn.y * k, dd.z - nn.z * k));  // :176
            const float ofs = .00001f;
            if (follow) {
                d = r;
                o = v3(h.p.x + h.n.x * ofs, h.p.y + h.n.y * ofs, h.p.z + h.n.z * ofs);  // :177
                ++J;
            }
            if constexpr (COUNT) n_refl += (unsigned long long)__builtin_popcountll(follow_mask);
        }
    }
    if constexpr (COUNT) {  // the wave's sums: lane k adds counter k — one vector atomic per wave
        unsigned long long v = 0ull;
        v = lane == REFL_WORK_PIXELS ? n_pixels : v;
        v = lane == REFL_WORK_REFLECTIONS ? n_refl : v;
        v = lane == REFL_WORK_CALLS ? n_calls : v;
        v = lane == REFL_WORK_WAVES ? (n_calls != 0ull ? 1ull : 0ull) : v;
        if (lane < REFL_WORK_N) atomicAdd(&io.work[lane], v);
    }
}

}  // namespace srt
