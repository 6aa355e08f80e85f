// srt_rays.hip.h — gfx950 closest-hit queries for caller-supplied rays (srt_trace_rays): for ray i of a batch,
// GetClosestObject(origin[i], direction[i]) (Raytracer.cpp:123-140) written out as the first-hit buffers write it — object
// index, normal + distance, point, albedo — plus OCCLUDED, the closest hit held against the ray's own t_max.
//
// The same closest_hit, on the same scene image, staged the same way and under the same tie rule as gbuffer_kernel and
// pick_kernel; what differs is where the ray comes from: two float4 arrays instead of GetRayDirection.  The workgroups are
// persistent, sized by the host as the G-buffer pass sizes them (a workgroup stages the scene once), and each wave strides over
// blocks of 64 consecutive rays: lane l of a block takes ray 64 * block + l, so a wave reads one contiguous KiB of each input
// array and writes one contiguous KiB (256 B for the int32 outputs) of each output.  Nothing is said about how coherent the
// rays of a block are: closest_hit's wave-level phases are correct for any 64 rays (the path pool's bounce rays are no more
// coherent).  No workgroup talks to another, no atomics reach the outputs.
#pragma once

#include "srt_kernel.hip.h"

namespace srt {

// The batch and where the launch writes (NULL: that output was not asked for).  All arrays are indexed by ray.
struct RaysIO {
    const float4* origin;     // (o.xyz, ignored)
    const float4* direction;  // (d.xyz, t_max)
    uint32_t count;           // rays, 1 .. 2^30
    uint32_t normalize;       // SRT_RAYS_NORMALIZE: d = float3::Normalized(d) first
    int32_t* object;          // list index of the hit object, -1 on a miss
    float4* normal_depth;     // (rayHit.normal, rayHit.distance); miss: (0, 0, 0, +inf)
    float4* position;         // (rayHit.point, 1); miss: 0
    float4* albedo;           // (material.BaseColor rgb, 0); miss: 0
    int32_t* occluded;        // 1: a closest hit with rayHit.distance < t_max; else 0
};

// LDS: the path-trace kernel's layout (make_lds with four waves), so the host's scene_in_lds decision and byte count carry over
// unchanged.  SCENE_LDS also selects closest_hit's short square root, exactly as in pathtrace_kernel / gbuffer_kernel.
template <bool SCENE_LDS, bool MESH>
__global__ void __launch_bounds__(WG_THREADS) rays_kernel(const KernelParams P, const RaysIO io) {
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
    const uint32_t blocks = (io.count + 63u) >> 6;  // count <= 2^30: at most 2^24 blocks
    const bool norm = io.normalize != 0u;           // (a kernel argument: wave-uniform)
    // wave-uniform loop: every lane of a wave runs the same trips, so closest_hit sees all 64 lanes in each call
    for (uint32_t b = blockIdx.x * (uint32_t)WAVES + (uint32_t)wave; b < blocks; b += gridDim.x * (uint32_t)WAVES) {
        const uint32_t i = (b << 6) + (uint32_t)lane;
        const bool active = i < io.count;
        // lanes past the batch load nothing: they carry a harmless unit ray through the wave's rounds and store nothing
        float4 o4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), d4 = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
        if (active) o4 = io.origin[i], d4 = io.direction[i];  // 16-byte loads
        V3 dir = v3(d4.x, d4.y, d4.z);
        if (norm) dir = normalized(dir);  // float3::Normalized (Common.hpp:159-162); its window test is wave-level: called by all lanes
        bool deferred = false;            // (defer_min = 1: every call resolves its mesh rays itself)
        const Hit h = closest_hit<MESH, false, SCENE_LDS>(S, P, v3(o4.x, o4.y, o4.z), dir, active, 1, deferred, no_tally SRT_PROF_ARG);
        if (!active) continue;
        const bool hit = h.prim >= 0;
        if (io.object) io.object[i] = hit ? S.order(h.prim) : -1;
        if (io.normal_depth)
            io.normal_depth[i] = hit ? make_float4(h.n.x, h.n.y, h.n.z, h.t) : make_float4(0.0f, 0.0f, 0.0f, __builtin_inff());
        if (io.position) io.position[i] = hit ? make_float4(h.p.x, h.p.y, h.p.z, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (io.albedo) {
            float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (hit) {  // material rows 0 / 1 of the primitive (srt_scene_image.h): base_color r, g | b
                const float4 m0 = S.mat(h.prim, 0), m1 = S.mat(h.prim, 1);
                a = make_float4(m0.z, m0.w, m1.x, 0.0f);
            }
            io.albedo[i] = a;
        }
        if (io.occluded) io.occluded[i] = (hit && h.t < d4.w) ? 1 : 0;  // binary32 <: a NaN t_max gives 0
    }
}

}  // namespace srt
