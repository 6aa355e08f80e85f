// srt_variance.hip.h — gfx950 variance estimate (srt_variance) and variance-guided à-trous filter (srt_denoise_variance):
// the spatial stage of SVGF (Schied et al. 2017, §4.2–4.4) on a dual-buffer variance (Rousselle et al. 2012).
//
// variance_kernel streams over the frame once: per pixel it reads the two half renders (2 x 16 B; the object index and, when
// demodulating, the albedo next to them), writes the squared half-difference of their luminances (4 B) and, when merging,
// the mean of the halves into the accumulator's rgb (12 B; the alpha is not stored).  One thread per pixel in memory order, so
// a wave reads and writes whole lines; no LDS, no atomics, no scratch.
//
// The filter is srt_denoise.hip.h's with two changes (include/srt_pathtrace.h is the contract the tests check): the colour
// edge-stop is exp(-|lum c_p - lum c_q| / (sigma_l sqrt(g_p) + 1e-10)), g_p being the 3 x 3 prefiltered variance of the level,
// and the variance is filtered with the colour by the squared weights.  The working variance travels in the .w of the working
// float4, so a tap stays one 16-byte load; the input alpha is re-attached after the last level as denoise_kernel<LAST> does.
// The 3 x 3 prefilter reads an LDS tile of the workgroup's 16 x 16 pixels plus a one-pixel apron, (variance, object) pairs,
// filled with one pass of coalesced loads: nine ds_read_b64 per pixel instead of nine more scattered global loads.  A row of the
// tile is 24 pairs wide: the four 8-lane rows of a half-wave then start 48 banks apart (0, 48, 32, 16 of 64) and do not conflict.
// The normal and plane terms, the tap order, the skipping rules and the sums are denoise_kernel's, operation for operation
// (same helpers, same expressions, -ffp-contract=off), so that with sigma_luminance = 0 the colour equals srt_denoise's with
// sigma_color = 0 bit for bit.  Work shape as denoise_kernel: a wave per 8 x 8 tile, four waves per workgroup.  No atomics, no
// scratch.
#pragma once

#include <cfloat>

#include "srt_denoise.hip.h"

namespace srt {

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

// One launch of the filter: DenoiseLevel with the luminance term in place of the colour term.
struct VarianceLevel {
    const float4* acc;           // the accumulator: the last level copies miss pixels and alpha from it
    const float4* src;           // this level's working colour (rgb) and variance (w)
    float4* dst;                 // this level's output (the result buffer on the last level, where w is the input alpha)
    const int32_t* object;       // SRT_GBUF_OBJECT
    const float4* normal_depth;  // SRT_GBUF_NORMAL_DEPTH: n xyz, d w
    const float4* position;      // SRT_GBUF_POSITION: x xyz
    const float4* albedo;        // SRT_GBUF_ALBEDO, NULL without demodulation
    const float* variance;       // the variance buffer: read by the preparation pass only
    uint32_t* framebuffer;       // last level with SRT_DENOISE_FRAMEBUFFER, else NULL (memory row H - 1 - y)
    int width, height, step;     // step = 2^i
    float sigma_normal;          // exponent of the normal term (at most FLT_MAX), 0 = off
    float sigma_plane;           // 0 = off
    float sigma_luminance;       // at most FLT_MAX; the LUM instantiations only
};

// Level 0's working pixel, once per pixel: denoise_prep_kernel's colour with the variance estimate in w.  Hit pixels only.
__global__ void __launch_bounds__(WG_THREADS) denoise_variance_prep_kernel(const VarianceLevel L) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = (int)blockIdx.x * WG_W + (wave % WG_TILES_X) * TILE_W + (lane & 7);
    const int y = (int)blockIdx.y * WG_H + (wave / WG_TILES_X) * TILE_H + (lane >> 3);
    if (x >= L.width || y >= L.height) return;
    const size_t p = (size_t)x + (size_t)y * (size_t)L.width;
    if (L.object[p] < 0) return;
    float4 c = L.acc[p];
    if (L.albedo) {
        const float4 a = L.albedo[p];
        c = make_float4(c.x / demod_factor(a.x), c.y / demod_factor(a.y), c.z / demod_factor(a.z), 0.0f);
    }
    L.dst[p] = make_float4(c.x, c.y, c.z, L.variance[p]);
}

// the LDS tile of the 3 x 3 prefilter: the workgroup's pixels and a one-pixel apron, rows VT_PITCH pairs apart
constexpr int VT_W = WG_W + 2, VT_H = WG_H + 2, VT_PITCH = 24;
static_assert(VT_W <= VT_PITCH, "a tile row must fit its pitch");

// LUM: the luminance term is on (sigma_luminance > 0); without it no tile is staged and the weights are denoise_kernel's with
// its colour term off.
template <bool LAST, bool LUM>
__global__ void __launch_bounds__(WG_THREADS) denoise_variance_kernel(const VarianceLevel L) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = (int)blockIdx.x * WG_W + (wave % WG_TILES_X) * TILE_W + (lane & 7);
    const int y = (int)blockIdx.y * WG_H + (wave / WG_TILES_X) * TILE_H + (lane >> 3);
    const int W = L.width, H = L.height;
    __shared__ float2 tile[LUM ? VT_H * VT_PITCH : 1];  // (working variance, object as bits); object -2 outside the frame
    if constexpr (LUM) {
        const int x0 = (int)blockIdx.x * WG_W - 1, y0 = (int)blockIdx.y * WG_H - 1;
        for (int i = (int)threadIdx.x; i < VT_W * VT_H; i += WG_THREADS) {
            const int ty = i / VT_W, tx = i - ty * VT_W;
            const int gx = x0 + tx, gy = y0 + ty;
            int o = -2;
            float v = 0.0f;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const size_t g = (size_t)gx + (size_t)gy * (size_t)W;
                o = L.object[g];
                if (o >= 0) v = L.src[g].w;  // (a miss has no working pixel)
            }
            tile[ty * VT_PITCH + tx] = make_float2(v, __int_as_float(o));
        }
        __syncthreads();  // every thread of the workgroup arrives: nothing has returned yet
    }
    if (x >= W || y >= H) return;
    const size_t p = (size_t)x + (size_t)y * (size_t)W;
    const int op = L.object[p];
    if (op < 0) {  // miss: the input, bit for bit, and never a tap
        if constexpr (LAST) {
            const float4 c = L.acc[p];
            L.dst[p] = c;
            if (L.framebuffer) L.framebuffer[(size_t)(H - 1 - y) * W + x] = tone_map(c);
        }
        return;
    }
    const float4 cp4 = L.src[p];
    const float3 cp = make_float3(cp4.x, cp4.y, cp4.z);
    const bool use_n = L.sigma_normal > 0.0f, use_x = L.sigma_plane > 0.0f;
    float3 np = make_float3(0.0f, 0.0f, 0.0f), xp = np;
    float plane_scale = 0.0f;  // 1 / (sigma_plane * d_p)
    if (use_n || use_x) {
        const float4 nd = L.normal_depth[p];
        np = make_float3(nd.x, nd.y, nd.z);
        if (use_x) {
            plane_scale = 1.0f / (L.sigma_plane * nd.w);
            if (__builtin_isinf(plane_scale)) plane_scale = copysignf(FLT_MAX, plane_scale);  // as denoise_kernel
        }
    }
    if (use_x) {
        const float4 xx = L.position[p];
        xp = make_float3(xx.x, xx.y, xx.z);
    }
    float lp = 0.0f, lum_scale = 0.0f;  // lum(c_p) and 1 / (sigma_luminance * sqrt(g_p) + 1e-10)
    if constexpr (LUM) {
        const float k[3] = {1.0f / 4, 2.0f / 4, 1.0f / 4};
        const int tc = ((wave / WG_TILES_X) * TILE_H + (lane >> 3) + 1) * VT_PITCH + (wave % WG_TILES_X) * TILE_W + (lane & 7) + 1;
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
        const float g = gs / ks;  // ks >= 4/16: the centre
        lum_scale = 1.0f / (L.sigma_luminance * sqrtf(g) + 1e-10f);
        if (__builtin_isinf(lum_scale)) lum_scale = copysignf(FLT_MAX, lum_scale);
        lp = luminance(cp.x, cp.y, cp.z);
    }
    const float h[5] = {1.0f / 16, 4.0f / 16, 6.0f / 16, 4.0f / 16, 1.0f / 16};
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
    const int s = L.step;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + s * dy;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + s * dx;
            if (qx < 0 || qx >= W) continue;
            const size_t q = (size_t)qx + (size_t)qy * (size_t)W;
            float w = h[dx + 2] * h[dy + 2];
            float3 cq = cp;
            float vq = cp4.w;
            if (dx != 0 || dy != 0) {
                if (L.object[q] != op) continue;  // another object (or a miss): skipped before anything of it is read
                const float4 c4 = L.src[q];
                cq = make_float3(c4.x, c4.y, c4.z);
                vq = c4.w;
                if (use_n) {
                    const float4 nq = L.normal_depth[q];
                    w = w * pow_pos(np.x * nq.x + np.y * nq.y + np.z * nq.z, L.sigma_normal);
                }
                if (use_x) {
                    const float4 xq = L.position[q];
                    const float d = np.x * (xq.x - xp.x) + np.y * (xq.y - xp.y) + np.z * (xq.z - xp.z);
                    w = w * __expf(-fabsf(d) * plane_scale);
                }
                if constexpr (LUM) w = w * __expf(-fabsf(lp - luminance(cq.x, cq.y, cq.z)) * lum_scale);
            }
            sw = sw + w;
            sr = sr + w * cq.x;
            sg = sg + w * cq.y;
            sb = sb + w * cq.z;
            if constexpr (!LAST) sv = sv + (w * w) * vq;  // (the last level's variance has no reader)
        }
    }
    float3 o = make_float3(sr / sw, sg / sw, sb / sw);  // sw >= 36/256: the centre tap
    if constexpr (LAST) {
        const float4 in = L.acc[p];
        if (L.albedo) {
            const float4 a = L.albedo[p];
            o = make_float3(o.x * demod_factor(a.x), o.y * demod_factor(a.y), o.z * demod_factor(a.z));
        }
        const float4 r = make_float4(o.x, o.y, o.z, in.w);
        L.dst[p] = r;
        if (L.framebuffer) L.framebuffer[(size_t)(H - 1 - y) * W + x] = tone_map(r);
    } else {
        L.dst[p] = make_float4(o.x, o.y, o.z, sv / (sw * sw));
    }
}

}  // namespace srt
