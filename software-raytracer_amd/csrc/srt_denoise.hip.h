// srt_denoise.hip.h — gfx950 denoisers (srt_denoise, srt_denoise_variance): an edge-avoiding à-trous wavelet filter (Dammertz et
// al. 2010) with SVGF-style normal and plane-distance weights, guided by the first-hit buffers of srt_render_gbuffer, and either
// a colour edge-stop or SVGF's variance-guided luminance stop (srt_variance.hip.h) with the variance filtered alongside.
//
// One launch per level: level i reads what level i - 1 wrote (taps up to 2 * 2^i pixels away), so the levels need a
// grid-wide barrier between them and a launch boundary is the cheapest one.  A preparation launch first writes level 0's
// working colour (the accumulator, demodulated by the albedo guide) once per pixel, so that no tap divides; the last level
// remodulates, writes the result and, when asked, the framebuffer pixel.  The weights use the hardware exp2 / log2
// (__expf, and max(0, d)^sn as exp2(sn log2 d)) and per-pixel reciprocals; that keeps the kernel off the
// correctly-rounded library paths at a relative error far inside the tests' tolerance.
// Work shape as gbuffer_kernel: a wave per 8 x 8 tile, four waves per workgroup (tile_pixel), so every float4 row segment a
// wave touches is one 128-byte line.  No atomics, no scratch; LDS only for the luminance stop's prefilter tile.
//
// The filter (include/srt_pathtrace.h is the contract the tests check):
//   w(p,q) = h(dx) h(dy) [o_q == o_p] max(0, n_p.n_q)^sn exp(-|n_p.(x_q - x_p)| / (sx d_p)) stop(p,q)
//   stop(p,q) = exp(-|c_p - c_q|^2 / (sc 2^-i)^2)  or  exp(-|lum c_p - lum c_q| / (sl sqrt(g_p) + 1e-10))
// with a term left out when its sigma is 0.  A tap of another object (or outside the frame) is skipped before any of its
// values is loaded, so non-finite colours or guides there cannot reach the sums; the centre tap weighs exactly 36/256.
// Every stop shares one tap loop, in one order of operations (-ffp-contract=off): with sigma_luminance = 0 the colour of
// srt_denoise_variance equals srt_denoise's with sigma_color = 0 bit for bit.
#pragma once

#include <cfloat>

#include "srt_kernel.hip.h"
#include "srt_variance.hip.h"  // demod_factor, the luminance stop

namespace srt {

// One level's launch.  All buffers W*H, index x + y * width, SCENE rows (the accumulator's layout).
struct AtrousLevel {
    const float4* acc;           // the accumulator: the last level copies miss pixels and alpha from it
    const float4* src;           // this level's working colour (rgb) and variance (w): atrous_prep_kernel's output, then the previous level's
    float4* dst;                 // this level's output (the result buffer on the last level, where w is the input alpha)
    const int32_t* object;       // SRT_GBUF_OBJECT
    const float4* normal_depth;  // SRT_GBUF_NORMAL_DEPTH: n xyz, d w
    const float4* position;      // SRT_GBUF_POSITION: x xyz
    const float4* albedo;        // SRT_GBUF_ALBEDO, NULL without demodulation
    const float* variance;       // srt_denoise_variance's variance buffer, read by the preparation pass only; NULL for srt_denoise
    uint32_t* framebuffer;       // last level with SRT_DENOISE_FRAMEBUFFER, else NULL (memory row H - 1 - y)
    int width, height, step;     // step = 2^i
    float sigma_normal;          // exponent of the normal term (at most FLT_MAX), 0 = off
    float sigma_plane;           // 0 = off
    float color_scale;           // STOP_COLOR: 1 / (sigma_color * 2^-i)^2 (at most FLT_MAX), 0 = off
    float sigma_luminance;       // STOP_LUMINANCE: at most FLT_MAX
};

// The working pixel of level 0, once per pixel instead of once per tap: the accumulator's rgb, divided by the albedo
// factors when demodulating, and the variance estimate (0 without one) in w.  Hit pixels only (miss pixels are never taps).
// Whether there is a variance buffer is a branch on a kernel argument, uniform over the launch: one load in a pass that is a
// tenth of a level's time does not pay for a second instantiation.
__global__ void __launch_bounds__(WG_THREADS) atrous_prep_kernel(const AtrousLevel L) {
    const TilePixel tp = tile_pixel();
    if (tp.x >= L.width || tp.y >= L.height) return;
    const size_t p = (size_t)tp.x + (size_t)tp.y * (size_t)L.width;
    if (L.object[p] < 0) return;
    float4 c = L.acc[p];
    if (L.albedo) {
        const float4 a = L.albedo[p];
        c = make_float4(c.x / demod_factor(a.x), c.y / demod_factor(a.y), c.z / demod_factor(a.z), 0.0f);
    }
    L.dst[p] = make_float4(c.x, c.y, c.z, L.variance ? L.variance[p] : 0.0f);
}

// max(0, d)^e for e > 0 through the hardware log2 / exp2 (v_log_f32, v_exp_f32): 0 for d <= 0
__device__ __forceinline__ float pow_pos(float d, float e) {
    return d > 0.0f ? __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(d)) : 0.0f;
}

// The geometric edge-stop of one centre pixel p: the normal and plane-distance terms of the denoisers and the upsampler.
struct EdgeStop {
    float3 np, xp;
    float plane_scale;   // 1 / (sigma_plane * d_p)
    float sigma_normal;  // (at most FLT_MAX)
    bool use_n, use_x;

    // `on`: whether p has a first hit to compare with (false: both terms off, nothing loaded)
    __device__ __forceinline__ void load(const float4* normal_depth, const float4* position, size_t p, float sn, float sigma_plane, bool on = true) {
        sigma_normal = sn;
        use_n = on && sn > 0.0f, use_x = on && sigma_plane > 0.0f;
        np = make_float3(0.0f, 0.0f, 0.0f), xp = np;
        plane_scale = 0.0f;
        if (use_n || use_x) {
            const float4 nd = normal_depth[p];
            np = make_float3(nd.x, nd.y, nd.z);
            if (use_x) {
                plane_scale = 1.0f / (sigma_plane * nd.w);
                // sigma_plane * d_p below about 2.9e-39 in magnitude: +-FLT_MAX instead of +-inf, so that an exact tie
                // n_p.(x_q - x_p) == 0 keeps its weight 1 (0 * inf would be NaN)
                if (__builtin_isinf(plane_scale)) plane_scale = copysignf(FLT_MAX, plane_scale);
            }
        }
        if (use_x) {
            const float4 xx = position[p];
            xp = make_float3(xx.x, xx.y, xx.z);
        }
    }
    // w times the normal term, then the plane term, of tap q (a pixel of p's object): each loads its guide only when it is on
    __device__ __forceinline__ float weight(const float4* normal_depth, const float4* position, size_t q, float w) const {
        if (use_n) {
            const float4 nq = normal_depth[q];
            w = w * pow_pos(np.x * nq.x + np.y * nq.y + np.z * nq.z, sigma_normal);
        }
        if (use_x) {
            const float4 xq = position[q];
            const float d = np.x * (xq.x - xp.x) + np.y * (xq.y - xp.y) + np.z * (xq.z - xp.z);
            w = w * __expf(-fabsf(d) * plane_scale);
        }
        return w;
    }
};

// The third factor of a tap's weight, and with it whether the working variance is filtered alongside the colour.
enum AtrousStop {
    STOP_COLOR,      // srt_denoise: the squared colour distance when color_scale > 0; no variance
    STOP_LUMINANCE,  // srt_denoise_variance with sigma_luminance > 0: the luminance stop over the prefiltered variance
    STOP_NONE,       // srt_denoise_variance with sigma_luminance = 0: no third factor, the variance still carried
};

template <bool LAST, AtrousStop STOP>
__global__ void __launch_bounds__(WG_THREADS) atrous_kernel(const AtrousLevel L) {
    constexpr bool LUM = STOP == STOP_LUMINANCE;
    constexpr bool VAR = STOP != STOP_COLOR && !LAST;  // (the last level's variance has no reader)
    const TilePixel tp = tile_pixel();
    const int x = tp.x, y = tp.y;
    const int W = L.width, H = L.height;
    __shared__ float2 tile[LUM ? VT_H * VT_PITCH : 1];
    if constexpr (LUM) stage_variance_tile(tile, L.object, L.src, W, H);  // every thread of the workgroup arrives: nothing has returned yet
    if (x >= W || y >= H) return;
    const size_t p = (size_t)x + (size_t)y * (size_t)W;
    const int op = L.object[p];
    if (op < 0) {  // miss: the input, bit for bit, and never a tap
        if constexpr (LAST) store_result(L.dst, p, L.framebuffer, x, y, W, H, L.acc[p]);
        return;
    }
    const float4 cp4 = L.src[p];
    const float3 cp = make_float3(cp4.x, cp4.y, cp4.z);
    const bool use_c = STOP == STOP_COLOR && L.color_scale > 0.0f;
    EdgeStop geo;
    geo.load(L.normal_depth, L.position, p, L.sigma_normal, L.sigma_plane);
    LuminanceStop lum;
    if constexpr (LUM) lum.load(prefiltered_variance(tile, tp.lx, tp.ly, op), cp, L.sigma_luminance);
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
                w = geo.weight(L.normal_depth, L.position, q, w);
                if (use_c) {
                    const float er = cp.x - cq.x, eg = cp.y - cq.y, eb = cp.z - cq.z;
                    w = w * __expf(-(er * er + eg * eg + eb * eb) * L.color_scale);
                }
                if constexpr (LUM) w = lum.weight(cq, w);
            }
            sw = sw + w;
            sr = sr + w * cq.x;
            sg = sg + w * cq.y;
            sb = sb + w * cq.z;
            if constexpr (VAR) sv = sv + (w * w) * vq;
        }
    }
    float3 o = make_float3(sr / sw, sg / sw, sb / sw);  // sw >= 36/256: the centre tap
    if constexpr (LAST) {
        const float4 in = L.acc[p];
        if (L.albedo) {
            const float4 a = L.albedo[p];
            o = make_float3(o.x * demod_factor(a.x), o.y * demod_factor(a.y), o.z * demod_factor(a.z));
        }
        store_result(L.dst, p, L.framebuffer, x, y, W, H, make_float4(o.x, o.y, o.z, in.w));
    } else {
        L.dst[p] = make_float4(o.x, o.y, o.z, VAR ? sv / (sw * sw) : 0.0f);
    }
}

}  // namespace srt
