// srt_variance.hip.h — gfx950 variance estimate (srt_variance) and the luminance edge-stop of the variance-guided à-trous filter
// (srt_denoise_variance): the spatial stage of SVGF (Schied et al. 2017, §4.2–4.4) on a dual-buffer variance (Rousselle et al.
// 2012).  The filter itself is srt_denoise.hip.h's atrous_kernel.
//
// variance_kernel streams over the frame once: per pixel it reads the two half renders (2 x 16 B; the object index and, when
// demodulating, the albedo next to them), writes the squared half-difference of their luminances (4 B) and, when merging,
// the mean of the halves into the accumulator's rgb (12 B; the alpha is not stored).  One thread per pixel in memory order, so
// a wave reads and writes whole lines; no LDS, no atomics, no scratch.
//
// The luminance stop (include/srt_pathtrace.h is the contract the tests check) is exp(-|lum c_p - lum c_q| / (sigma_l sqrt(g_p) +
// 1e-10)), g_p being the 3 x 3 prefiltered variance of the level.  The working variance travels in the .w of the working float4,
// so a tap stays one 16-byte load.  The prefilter reads an LDS tile of the workgroup's 16 x 16 pixels plus a one-pixel apron,
// (variance, object) pairs, filled with one pass of coalesced loads: nine ds_read_b64 per pixel instead of nine more scattered
// global loads.  A row of the tile is 24 pairs wide: the four 8-lane rows of a half-wave then start 48 banks apart (0, 48, 32, 16
// of 64) and do not conflict.
#pragma once

#include <cfloat>

#include "srt_kernel.hip.h"

namespace srt {

// demodulation factor of one channel: the albedo where it is at least 1e-3, else 1
__device__ __forceinline__ float demod_factor(float a) { return a >= 1e-3f ? a : 1.0f; }

// Rec. 709 luminance in the contract's order: (0.2126 r + 0.7152 g) + 0.0722 b
__device__ __forceinline__ float luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// All buffers W*H, index x + y * width, SCENE rows (the accumulator's layout).
struct VarianceLaunch {
    float4* acc;            // half A: read, and with `merge` its rgb replaced by the mean of the halves (alpha never stored)
    const float4* half;     // half B
    const int32_t* object;  // SRT_GBUF_OBJECT
    const float4* albedo;   // SRT_GBUF_ALBEDO, NULL without demodulation
    float* variance;        // the output
    size_t pixels;          // W*H
    int merge;              // SRT_VARIANCE_MERGE
};

constexpr int VARIANCE_THREADS = 256;

__global__ void __launch_bounds__(VARIANCE_THREADS) variance_kernel(const VarianceLaunch V) {
    const size_t p = (size_t)blockIdx.x * VARIANCE_THREADS + threadIdx.x;
    if (p >= V.pixels) return;
    const float4 a = V.acc[p], b = V.half[p];
    float v = 0.0f;  // a miss
    if (V.object[p] >= 0) {
        float la, lb;
        if (V.albedo) {
            const float4 m4 = V.albedo[p];
            const float mr = demod_factor(m4.x), mg = demod_factor(m4.y), mb = demod_factor(m4.z);
            la = luminance(a.x / mr, a.y / mg, a.z / mb);
            lb = luminance(b.x / mr, b.y / mg, b.z / mb);
        } else {
            la = luminance(a.x, a.y, a.z);
            lb = luminance(b.x, b.y, b.z);
        }
        const float d = 0.5f * la - 0.5f * lb;
        v = d * d;
    }
    V.variance[p] = v;
    if (V.merge) {
        float* const rgb = (float*)(V.acc + p);
        rgb[0] = 0.5f * a.x + 0.5f * b.x;
        rgb[1] = 0.5f * a.y + 0.5f * b.y;
        rgb[2] = 0.5f * a.z + 0.5f * b.z;
    }
}

// the LDS tile of the 3 x 3 prefilter: the workgroup's pixels and a one-pixel apron, rows VT_PITCH pairs apart
constexpr int VT_W = WG_W + 2, VT_H = WG_H + 2, VT_PITCH = 24;
static_assert(VT_W <= VT_PITCH, "a tile row must fit its pitch");

// Fills the tile with (working variance, object as bits) of level input `src`; object -2 outside the frame.  Every thread of the
// workgroup calls it, before any returns.
__device__ __forceinline__ void stage_variance_tile(float2* tile, const int32_t* object, const float4* src, int W, int H) {
    const int x0 = (int)blockIdx.x * WG_W - 1, y0 = (int)blockIdx.y * WG_H - 1;
    for (int i = (int)threadIdx.x; i < VT_W * VT_H; i += WG_THREADS) {
        const int ty = i / VT_W, tx = i - ty * VT_W;
        const int gx = x0 + tx, gy = y0 + ty;
        int o = -2;
        float v = 0.0f;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t g = (size_t)gx + (size_t)gy * (size_t)W;
            o = object[g];
            if (o >= 0) v = src[g].w;  // (a miss has no working pixel)
        }
        tile[ty * VT_PITCH + tx] = make_float2(v, __int_as_float(o));
    }
    __syncthreads();
}

// g_p: the (1 2 1)^2 / 16 mean of the tile's variances around workgroup pixel (lx, ly) over the taps of its object `op`
__device__ __forceinline__ float prefiltered_variance(const float2* tile, int lx, int ly, int op) {
    const float k[3] = {1.0f / 4, 2.0f / 4, 1.0f / 4};
    const int tc = (ly + 1) * VT_PITCH + lx + 1;
    float ks = 0.0f, gs = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const float2 t = tile[tc + dy * VT_PITCH + dx];
            if ((dx != 0 || dy != 0) && __float_as_int(t.y) != op) continue;  // outside the frame or another object
            const float kw = k[dx + 1] * k[dy + 1];
            ks = ks + kw;
            gs = gs + kw * t.x;
        }
    }
    return gs / ks;  // ks >= 4/16: the centre
}

// The luminance edge-stop of one centre pixel.
struct LuminanceStop {
    float lp = 0.0f;     // lum(c_p)
    float scale = 0.0f;  // 1 / (sigma_luminance * sqrt(g_p) + 1e-10), at most FLT_MAX in size

    __device__ __forceinline__ void load(float g, float3 cp, float sigma_luminance) {
        scale = 1.0f / (sigma_luminance * sqrtf(g) + 1e-10f);
        if (__builtin_isinf(scale)) scale = copysignf(FLT_MAX, scale);
        lp = luminance(cp.x, cp.y, cp.z);
    }
    // w times the stop's factor for a tap of colour cq
    __device__ __forceinline__ float weight(float3 cq, float w) const { return w * __expf(-fabsf(lp - luminance(cq.x, cq.y, cq.z)) * scale); }
};

}  // namespace srt
