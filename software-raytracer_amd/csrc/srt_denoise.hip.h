// srt_denoise.hip.h — gfx950 denoiser (srt_denoise): an edge-avoiding à-trous wavelet filter (Dammertz et al. 2010) with
// SVGF-style normal and plane-distance weights, guided by the first-hit buffers of srt_render_gbuffer.
//
// One launch per level: level i reads what level i - 1 wrote (taps up to 2 * 2^i pixels away), so the levels need a
// grid-wide barrier between them and a launch boundary is the cheapest one.  A preparation launch first writes level 0's
// working colour (the accumulator, demodulated by the albedo guide) once per pixel, so that no tap divides; the last level
// remodulates, writes the result and, when asked, the framebuffer pixel.  The weights use the hardware exp2 / log2
// (__expf, and max(0, d)^sn as exp2(sn log2 d)) and per-pixel reciprocals; that keeps the kernel off the
// correctly-rounded library paths at a relative error far inside the tests' tolerance.
// Work shape as gbuffer_kernel: a wave per 8 x 8 tile (lane -> x = lane & 7, y = lane >> 3), four waves per workgroup
// (16 x 16 pixels), so every float4 row segment a wave touches is one 128-byte line.  No LDS, no atomics, no scratch.
//
// The filter (include/srt_pathtrace.h is the contract the tests check):
//   w(p,q) = h(dx) h(dy) [o_q == o_p] max(0, n_p.n_q)^sn exp(-|n_p.(x_q - x_p)| / (sx d_p)) exp(-|c_p - c_q|^2 / (sc 2^-i)^2)
// with a term left out when its sigma is 0.  A tap of another object (or outside the frame) is skipped before any of its
// values is loaded, so non-finite colours or guides there cannot reach the sums; the centre tap weighs exactly 36/256.
#pragma once

#include <cfloat>

#include "srt_kernel.hip.h"

namespace srt {

// One level's launch.  All buffers W*H, index x + y * width, SCENE rows (the accumulator's layout).
struct DenoiseLevel {
    const float4* acc;         // the accumulator: the last level copies miss pixels and alpha from it
    const float4* src;         // this level's working colour (rgb): denoise_prep_kernel's output, then the previous level's
    float4* dst;               // this level's output (the result buffer on the last level)
    const int32_t* object;     // SRT_GBUF_OBJECT
    const float4* normal_depth;  // SRT_GBUF_NORMAL_DEPTH: n xyz, d w
    const float4* position;    // SRT_GBUF_POSITION: x xyz
    const float4* albedo;      // SRT_GBUF_ALBEDO, NULL without demodulation
    uint32_t* framebuffer;     // last level with SRT_DENOISE_FRAMEBUFFER, else NULL (memory row H - 1 - y)
    int width, height, step;   // step = 2^i
    float sigma_normal;        // exponent of the normal term (at most FLT_MAX), 0 = off
    float sigma_plane;         // 0 = off
    float color_scale;         // 1 / (sigma_color * 2^-i)^2 (at most FLT_MAX), 0 = off
};

// demodulation factor of one channel: the albedo where it is at least 1e-3, else 1
__device__ __forceinline__ float demod_factor(float a) { return a >= 1e-3f ? a : 1.0f; }

// The working colour of level 0, once per pixel instead of once per tap: the accumulator's rgb, divided by the albedo
// factors when demodulating.  Hit pixels only (miss pixels are never taps).
__global__ void __launch_bounds__(WG_THREADS) denoise_prep_kernel(const DenoiseLevel L) {
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
    L.dst[p] = make_float4(c.x, c.y, c.z, 0.0f);
}

// max(0, d)^e for e > 0 through the hardware log2 / exp2 (v_log_f32, v_exp_f32): 0 for d <= 0
__device__ __forceinline__ float pow_pos(float d, float e) {
    return d > 0.0f ? __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(d)) : 0.0f;
}

template <bool LAST>
__global__ void __launch_bounds__(WG_THREADS) denoise_kernel(const DenoiseLevel L) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = (int)blockIdx.x * WG_W + (wave % WG_TILES_X) * TILE_W + (lane & 7);
    const int y = (int)blockIdx.y * WG_H + (wave / WG_TILES_X) * TILE_H + (lane >> 3);
    const int W = L.width, H = L.height;
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
    const bool use_n = L.sigma_normal > 0.0f, use_x = L.sigma_plane > 0.0f, use_c = L.color_scale > 0.0f;
    float3 np = make_float3(0.0f, 0.0f, 0.0f), xp = np;
    float plane_scale = 0.0f;  // 1 / (sigma_plane * d_p)
    if (use_n || use_x) {
        const float4 nd = L.normal_depth[p];
        np = make_float3(nd.x, nd.y, nd.z);
        if (use_x) {
            plane_scale = 1.0f / (L.sigma_plane * nd.w);
            // sigma_plane * d_p below about 2.9e-39 in magnitude: +-FLT_MAX instead of +-inf, so that an exact tie
            // n_p.(x_q - x_p) == 0 keeps its weight 1 (0 * inf would be NaN)
            if (__builtin_isinf(plane_scale)) plane_scale = copysignf(FLT_MAX, plane_scale);
        }
    }
    if (use_x) {
        const float4 xx = L.position[p];
        xp = make_float3(xx.x, xx.y, xx.z);
    }
    const float h[5] = {1.0f / 16, 4.0f / 16, 6.0f / 16, 4.0f / 16, 1.0f / 16};
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
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
            if (dx != 0 || dy != 0) {
                if (L.object[q] != op) continue;  // another object (or a miss): skipped before anything of it is read
                const float4 c4 = L.src[q];
                cq = make_float3(c4.x, c4.y, c4.z);
                if (use_n) {
                    const float4 nq = L.normal_depth[q];
                    w = w * pow_pos(np.x * nq.x + np.y * nq.y + np.z * nq.z, L.sigma_normal);
                }
                if (use_x) {
                    const float4 xq = L.position[q];
                    const float d = np.x * (xq.x - xp.x) + np.y * (xq.y - xp.y) + np.z * (xq.z - xp.z);
                    w = w * __expf(-fabsf(d) * plane_scale);
                }
                if (use_c) {
                    const float er = cp.x - cq.x, eg = cp.y - cq.y, eb = cp.z - cq.z;
                    w = w * __expf(-(er * er + eg * eg + eb * eb) * L.color_scale);
                }
            }
            sw = sw + w;
            sr = sr + w * cq.x;
            sg = sg + w * cq.y;
            sb = sb + w * cq.z;
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
        L.dst[p] = make_float4(o.x, o.y, o.z, 0.0f);
    }
}

}  // namespace srt
