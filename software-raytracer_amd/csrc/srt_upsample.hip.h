// srt_upsample.hip.h — gfx950 guided upsampler (srt_upsample): the progressive-resolution blocks of srt_render (one ray per
// steps x steps block, Raytracer.cpp:233-248) reconstructed at full resolution by a joint-bilateral interpolation of the
// blocks' anchor pixels, guided by the first-hit buffers of srt_render_gbuffer (joint bilateral upsampling, Kopf et al. 2007,
// with the denoiser's object, normal and plane-distance weights in place of a colour range term).
//
// The block's ray is the camera ray through its anchor pixel and there is no sub-pixel jitter, so the full-resolution
// guides hold, at the anchor, exactly the first hit the block's colour belongs to.  Every pixel takes the up to four anchors
// around it (its own block's, the next block's to the right, above, and diagonally), weighs them bilinearly and by how well
// their first hit agrees with its own, and never looks at a non-anchor pixel of the colour buffer.
//
// One launch.  Work shape as atrous_kernel and temporal_kernel: a wave per 8 x 8 tile (lane -> x = lane & 7, y = lane >> 3),
// four waves per workgroup (16 x 16 pixels), so every float4 row segment a wave touches is one 128-byte line.  No LDS, no
// atomics, no scratch.  The weights are the denoiser's (EdgeStop).
// In place (SRT_UPSAMPLE_IN_PLACE) the launch reads anchors only and writes non-anchors only: no pixel reads what another
// writes, so one launch needs no second buffer and no grid-wide barrier.
#pragma once

#include "srt_denoise.hip.h"

namespace srt {

// All buffers W*H, index x + y * width, SCENE rows (the accumulator's layout).
struct UpsampleLaunch {
    const float4* acc;           // the accumulator: anchors are the taps; p's own pixel gives the alpha and the fallback
    float4* dst;                 // the result buffer; NULL with in_place
    float* acc_rgb;              // in_place: the accumulator again, for the three-float stores into non-anchor pixels
    const int32_t* object;       // SRT_GBUF_OBJECT
    const float4* normal_depth;  // SRT_GBUF_NORMAL_DEPTH: n xyz, d w
    const float4* position;      // SRT_GBUF_POSITION: x xyz
    uint32_t* framebuffer;       // SRT_UPSAMPLE_FRAMEBUFFER, else NULL (memory row H - 1 - y)
    int width, height;
    int steps;                   // >= 1
    int stripe;                  // S: stripe_width, or the width when that is 0 or larger (1..width)
    float sigma_normal;          // exponent of the normal term (at most FLT_MAX), 0 = off
    float sigma_plane;           // 0 = off
};

// The anchors around coordinate v on an axis whose anchors are origin + j * steps below `end` (the stripe's end on columns,
// the frame's on rows) and, on columns, the next stripe's first column `end` when that lies inside the frame: a0 = the
// largest anchor <= v, a1 = the smallest anchor > v or -1, f = (v - a0) / (a1 - a0) in binary32 (0 without a1).
__device__ __forceinline__ void upsample_axis(int v, int origin, int end, int limit, int steps, int& a0, int& a1, float& f) {
    a0 = origin + ((v - origin) / steps) * steps;
    a1 = a0 + steps;
    if (a1 >= end) a1 = end;  // the next stripe starts here (columns); rows: end == limit
    if (a1 >= limit) a1 = -1;
    f = a1 < 0 ? 0.0f : (float)(v - a0) / (float)(a1 - a0);
}

__global__ void __launch_bounds__(WG_THREADS) upsample_kernel(const UpsampleLaunch U) {
    const TilePixel tp = tile_pixel();
    const int x = tp.x, y = tp.y;
    const int W = U.width, H = U.height;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)x + (size_t)y * (size_t)W;
    const float4 c = U.acc[p];
    int x0, x1, y0, y1;
    float fx, fy;
    const int s0 = (x / U.stripe) * U.stripe;
    upsample_axis(x, s0, s0 + U.stripe, W, U.steps, x0, x1, fx);
    upsample_axis(y, 0, H, H, U.steps, y0, y1, fy);
    float4 out = c;
    const bool anchor = x == x0 && y == y0;  // its one tap is itself, weight 1: the input bits
    if (!anchor) {
        const int op = U.object[p];
        EdgeStop geo;  // a miss has no first hit to compare with: its taps (other misses) are weighed bilinearly alone
        geo.load(U.normal_depth, U.position, p, U.sigma_normal, U.sigma_plane, op >= 0);
        float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int qx = (k & 1) ? x1 : x0, qy = (k >> 1) ? y1 : y0;
            float w = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
            if (qx < 0 || qy < 0 || w == 0.0f) continue;
            const size_t q = (size_t)qx + (size_t)qy * (size_t)W;
            if (U.object[q] != op) continue;  // another object: skipped before anything else of it is read
            w = geo.weight(U.normal_depth, U.position, q, w);
            const float4 cq = U.acc[q];
            sw = sw + w;
            sr = sr + w * cq.x;
            sg = sg + w * cq.y;
            sb = sb + w * cq.z;
        }
        if (sw != 0.0f) {  // else no tap counted, or they weigh nothing: the pixel keeps its input
            out = make_float4(sr / sw, sg / sw, sb / sw, c.w);
            if (U.acc_rgb) {
                float* const a = U.acc_rgb + 4 * p;
                a[0] = out.x, a[1] = out.y, a[2] = out.z;
            }
        }
    }
    if (U.dst) U.dst[p] = out;
    store_framebuffer(U.framebuffer, x, y, W, H, out);
}

}  // namespace srt
