// srt_antialias.hip.h — gfx950 geometry-supersampled anti-aliasing (srt_render_subsamples, srt_antialias): subpixel
// reconstruction anti-aliasing (Chajdas, McGuire and Luebke 2011) on the first hit, which is the cheap thing here.
//
// The reference has no sub-pixel jitter (GetRayDirection, Raytracer.cpp:106-122), so a pixel's colour converges and its
// coverage never does.  subsample_kernel traces the object index at k x k sub-pixel positions of every pixel; antialias_kernel
// rebuilds each pixel as the mix of its own colour and the colours of the neighbouring pixels whose object its sub-samples
// see.  Shading stays one estimate per pixel, and a pixel all of whose sub-samples see its own object keeps its bits.
//
// subsample_kernel is gbuffer_kernel with an inner loop: persistent workgroups that stage the scene image once, waves that
// stride over 8 x 8 pixel tiles and, within a tile, over the K planes.  One trip is one wave-wide closest_hit on the 64 rays
// of one plane — as coherent as the G-buffer's, the whole tile shifted by a fraction of a pixel — and one 4-byte store per
// lane (every 8-pixel row segment is a contiguous 32 bytes).  No LDS beyond make_lds's layout, no atomics.
//
// antialias_kernel has the work shape of upsample_kernel: a wave per 8 x 8 tile, four waves per workgroup, no LDS, no atomics,
// no scratch (the K plane values live in registers: the kernel is instantiated per k and its loops over s are unrolled).
#pragma once

#include "srt_denoise.hip.h"
#include "srt_gbuffer.hip.h"

namespace srt {

// The sub-sample planes: K*W*H int32, plane-major, index s*W*H + x + y*W with the SCENE row y.
struct SubsampleOut {
    int32_t* sub;
    int k;  // 1..4
};

// One launch covers scene rows [P.y0, P.y0 + P.rows) of every plane.  LDS, staging and closest_hit as gbuffer_kernel.
template <bool SCENE_LDS, bool MESH>
__global__ void __launch_bounds__(WG_THREADS) subsample_kernel(const KernelParams P, const SubsampleOut out) {
    extern __shared__ float4 lds_scene[];
    if constexpr (SCENE_LDS) {  // staged as gbuffer_kernel stages it: every load issued before the first LDS store
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
    const int W = P.width, H = P.height, k = out.k, K = k * k;
    // the virtual frame of 2k W x 2k H pixels (both below 2^24: exact in binary32)
    const float VW = (float)(2 * k * W), VH = (float)(2 * k * H);
    const size_t plane = (size_t)W * (size_t)H;
    const int tiles_x = (W + TILE_W - 1) / TILE_W, tiles_y = (P.rows + TILE_H - 1) / TILE_H;
    const int tiles = tiles_x * tiles_y;
    const V3 cam = v3(P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]);
    // wave-uniform loops: every lane of a wave runs the same trips, so closest_hit sees all 64 lanes in each call
    for (int t = (int)blockIdx.x * WAVES + wave; t < tiles; t += (int)gridDim.x * WAVES) {
        const int tx = t % tiles_x, ty = t / tiles_x;
        const int px = tx * TILE_W + (lane & 7), py = ty * TILE_H + (lane >> 3);
        const bool in_range = px < W && py < P.rows;
        // lanes outside the frame or band trace the nearest pixel's rays (take part in the wave's rounds) and store nothing
        const int x = px < W ? px : W - 1, y = P.y0 + (py < P.rows ? py : P.rows - 1);
        const size_t pix = (size_t)x + (size_t)y * (size_t)W;
        int i = 0, j = 0;  // s = j * k + i
        for (int s = 0; s < K; ++s) {
            // ---- GetRayDirection (Raytracer.cpp:106-122) for pixel (X, Y) of the virtual frame; X, Y may be negative ----
            const int X = 2 * k * x + 2 * i - (k - 1), Y = 2 * k * y + 2 * j - (k - 1);
            float nX = ((float)X / VW) * 2 - 1;
            float nY = ((float)Y / VH) * 2 - 1;
            V3 u = v3(P.right_rd[0] * nX, P.right_rd[1] * nX, P.right_rd[2] * nX);
            V3 vv = v3(P.up_ld[0] * nY, P.up_ld[1] * nY, P.up_ld[2] * nY);
            const V3 dir = normalized(v3((u.x + vv.x) + P.fwd_clip[0], (u.y + vv.y) + P.fwd_clip[1], (u.z + vv.z) + P.fwd_clip[2]));
            bool deferred = false;  // (defer_min = 1: every call resolves its mesh rays itself)
            const Hit h = closest_hit<MESH, false, SCENE_LDS>(S, P, cam, dir, true, 1, deferred, no_tally SRT_PROF_ARG);
            if (in_range) out.sub[(size_t)s * plane + pix] = h.prim >= 0 ? S.order(h.prim) : -1;
            if (++i == k) i = 0, ++j;
        }
    }
}

// All buffers W*H (sub: K planes of W*H), index x + y * width, SCENE rows (the accumulator's layout).
struct AntialiasLaunch {
    const float4* src;      // the colour c: the accumulator or the denoised buffer
    float4* dst;            // the result buffer, never src
    const int32_t* object;  // SRT_GBUF_OBJECT
    const int32_t* sub;     // the sub-sample planes
    uint32_t* framebuffer;  // SRT_AA_FRAMEBUFFER, else NULL (memory row H - 1 - y)
    int width, height;
};

template <int KK>  // k
__global__ void __launch_bounds__(WG_THREADS) antialias_kernel(const AntialiasLaunch A) {
    constexpr int K = KK * KK;
    const TilePixel tp = tile_pixel();
    const int x = tp.x, y = tp.y;
    const int W = A.width, H = A.height;
    if (x >= W || y >= H) return;
    const size_t plane = (size_t)W * (size_t)H;
    const size_t p = (size_t)x + (size_t)y * (size_t)W;
    // the K plane values (coalesced 4-byte loads), the pixel's own object and colour: all issued together
    int32_t sv[K];
#pragma unroll
    for (int s = 0; s < K; ++s) sv[s] = A.sub[(size_t)s * plane + p];
    const int32_t op = A.object[p];
    const float4 c = A.src[p];
    bool foreign = false;
#pragma unroll
    for (int s = 0; s < K; ++s) foreign |= sv[s] != op;
    float4 out = c;
    // a wave of interior pixels (most of a frame) leaves through the copy below without touching a neighbour
    if (__ballot(foreign) != 0ull && foreign) {
        float sr = 0.0f, sg = 0.0f, sb = 0.0f;
        bool changed = false;  // some C_s came from taps: else the pixel keeps its bits
#pragma unroll
        for (int s = 0; s < K; ++s) {
            float cr = c.x, cg = c.y, cb = c.z;  // rule 2, and the fallback of rule 3
            if (sv[s] != op) {
                const float dx = (float)(2 * (s % KK) - (KK - 1)) / (float)(2 * KK);
                const float dy = (float)(2 * (s / KK) - (KK - 1)) / (float)(2 * KK);
                float sw = 0.0f, tr = 0.0f, tg = 0.0f, tb = 0.0f;
                for (int ay = -1; ay <= 1; ++ay) {
                    const float wy = fmaxf(0.0f, 1.0f - fabsf((float)ay - dy));
                    const int qy = y + ay;
                    if (wy == 0.0f || qy < 0 || qy >= H) continue;
                    for (int ax = -1; ax <= 1; ++ax) {
                        const float w = fmaxf(0.0f, 1.0f - fabsf((float)ax - dx)) * wy;
                        const int qx = x + ax;
                        if (w == 0.0f || qx < 0 || qx >= W) continue;
                        const size_t q = (size_t)qx + (size_t)qy * (size_t)W;
                        if (A.object[q] != sv[s]) continue;  // another object: skipped before its colour is read
                        const float4 cq = A.src[q];
                        sw = sw + w;
                        tr = tr + w * cq.x;
                        tg = tg + w * cq.y;
                        tb = tb + w * cq.z;
                    }
                }
                if (sw != 0.0f) {  // (the weights that count are positive: 0 means no tap counted)
                    cr = tr / sw, cg = tg / sw, cb = tb / sw;
                    changed = true;
                }
            }
            sr = sr + cr;
            sg = sg + cg;
            sb = sb + cb;
        }
        if (changed) out = make_float4(sr / (float)K, sg / (float)K, sb / (float)K, c.w);
    }
    store_result(A.dst, p, A.framebuffer, x, y, W, H, out);
}

}  // namespace srt
