// srt_gbuffer.hip.h — gfx950 first-hit buffers (srt_render_gbuffer): per pixel, the camera ray's closest hit
// (GetClosestObject, Raytracer.cpp:123-140) written out as object index, normal + distance, point and albedo.
//
// The ray, its generation and the tie rule are those of the path-trace kernel's primary ray and of pick_kernel
// (GetRayDirection, Raytracer.cpp:106-122, no jitter): the same closest_hit, on the same scene image, staged the
// same way.  What differs is the shape of the work: one ray per pixel and a few stores, so the cost of staging a
// scene of up to ~2000 primitives into LDS would dwarf the 256 rays of a workgroup.  The workgroups are therefore
// persistent — about CUs x resident workgroups, sized by the host — and each wave strides over 8 x 8 pixel tiles
// (lane -> x = lane & 7, y = lane >> 3: coherent rays for closest_hit's wave-level cluster culling, and every float4
// output row segment of a tile is one 128-byte line).  No workgroup talks to another.
#pragma once

#include "srt_kernel.hip.h"

namespace srt {

// Where the launch writes (NULL: that output was not asked for).  Indexed x + y * width with the SCENE row y,
// like the float4 accumulator.
struct GBufferOut {
    int32_t* object;       // list index of the hit object, -1 on a miss
    float4* normal_depth;  // (rayHit.normal, rayHit.distance); miss: (0, 0, 0, +inf)
    float4* position;      // (rayHit.point, 1); miss: 0
    float4* albedo;        // (material.BaseColor rgb, 0); miss: 0
};

// One launch covers scene rows [P.y0, P.y0 + P.rows).  LDS: the path-trace kernel's layout (make_lds with four waves), so
// the host's scene_in_lds decision and byte count carry over unchanged.  SCENE_LDS also selects closest_hit's short square
// root, exactly as in pathtrace_kernel (the host only stages scenes whose radii lie in its window).
template <bool SCENE_LDS, bool MESH>
__global__ void __launch_bounds__(WG_THREADS) gbuffer_kernel(const KernelParams P, const GBufferOut out) {
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
    // wave-uniform loop: every lane of a wave runs the same trips, so closest_hit sees all 64 lanes in each call
    for (int t = (int)blockIdx.x * WAVES + wave; t < tiles; t += (int)gridDim.x * WAVES) {
        const int tx = t % tiles_x, ty = t / tiles_x;
        const int px = tx * TILE_W + (lane & 7), py = ty * TILE_H + (lane >> 3);
        const bool in_range = px < W && py < P.rows;
        // lanes outside the frame or band trace the nearest pixel's ray (take part in the wave's rounds) and store nothing
        const int x = px < W ? px : W - 1, y = P.y0 + (py < P.rows ? py : P.rows - 1);
        // ---- GetRayDirection (Raytracer.cpp:106-122), as pick_kernel / pathtrace_kernel ----
        float nX = ((float)x / (float)W) * 2 - 1;
        float nY = ((float)y / (float)H) * 2 - 1;
        V3 u = v3(P.right_rd[0] * nX, P.right_rd[1] * nX, P.right_rd[2] * nX);
        V3 vv = v3(P.up_ld[0] * nY, P.up_ld[1] * nY, P.up_ld[2] * nY);
        const V3 dir = normalized(v3((u.x + vv.x) + P.fwd_clip[0], (u.y + vv.y) + P.fwd_clip[1], (u.z + vv.z) + P.fwd_clip[2]));
        bool deferred = false;  // (defer_min = 1: every call resolves its mesh rays itself)
        const Hit h = closest_hit<MESH, false, SCENE_LDS>(S, P, cam, dir, true, 1, deferred, no_tally SRT_PROF_ARG);
        if (!in_range) continue;
        const bool hit = h.prim >= 0;
        const size_t pix = (size_t)x + (size_t)y * (size_t)W;
        if (out.object) out.object[pix] = hit ? S.order(h.prim) : -1;
        if (out.normal_depth)
            out.normal_depth[pix] = hit ? make_float4(h.n.x, h.n.y, h.n.z, h.t) : make_float4(0.0f, 0.0f, 0.0f, __builtin_inff());
        if (out.position) out.position[pix] = hit ? make_float4(h.p.x, h.p.y, h.p.z, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (out.albedo) {
            float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (hit) {  // material rows 0 / 1 of the primitive (srt_scene_image.h): base_color r, g | b
                const float4 m0 = S.mat(h.prim, 0), m1 = S.mat(h.prim, 1);
                a = make_float4(m0.z, m0.w, m1.x, 0.0f);
            }
            out.albedo[pix] = a;
        }
    }
}

}  // namespace srt
