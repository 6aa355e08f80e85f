// srt_moments.hip.h — gfx950 variance from the temporal history (srt_temporal_variance): the moments stage of SVGF (Schied et
// al. 2017, §4.2).  srt_temporal_accumulate with srt_moments_output keeps per pixel the running moments (M1, M2) of the frames'
// luminance and their length Lm (srt_temporal.hip.h); this pass turns one slot of those records into the variance buffer
// srt_denoise_variance reads.
//
// A pixel whose moments are old enough (Lm >= min_frames * n) takes M2 - M1^2 of its own record.  A young one (a disocclusion,
// the first frames of a sequence) has too few frames for that and takes the same expression of the moments averaged over the
// (2R+1)^2 window around it, taps of its own object only.  Either is scaled by n / Lm: the variance of the estimate the
// accumulator holds, not of one frame.
//
// Work shape as the other passes: a wave per 8 x 8 tile, four waves per 16 x 16 workgroup.  In steady state no pixel is young and
// the pass is a stream: 16 B of record and 4 B of object index in, 4 B out.  So the workgroup first votes (__syncthreads_or), and
// only when some pixel of it is young stages its tile plus an R-pixel apron in LDS, one float4 (M1, M2, object as bits, 1) per
// entry, filled with one pass of coalesced loads.  The window is then (2R+1)^2 ds_read_b128 per young pixel instead of as many
// scattered 16-byte global loads; a wave without a young lane branches over the loop.  A tile row is MT_PITCH = 24 entries wide:
// ds_read_b128 is served in groups of 16 lanes, each lane taking one 16-byte slot of the 16 in a 256-byte bank row, and a group
// holds four 4-lane pieces of four different pixel rows (lanes 0-3, 12-15, 20-27: columns 0-3 of row 0, 4-7 of rows 1 and 2, 0-3
// of row 3).  Their first slots are 0, 24 + 4, 48 + 4 and 72, that is 0, 12, 4 and 8 modulo 16: four disjoint runs of four, so a
// tap of a full wave is conflict-free at every window offset (an offset shifts all lanes alike).  The other three groups are the
// same pattern shifted.  22 rows x 24 entries x 16 B = 8448 B per workgroup at R = 3.
// Every thread reaches both barriers before it leaves.  No atomics, no scratch; the result depends on nothing but the inputs.
#pragma once

#include "srt_kernel.hip.h"

namespace srt {

// All buffers W*H, index x + y * width, SCENE rows (the accumulator's layout).
struct MomentsLaunch {
    const float4* moments;  // (M1, M2, Lm, 0), (0, 0, 0, 0) on a miss
    const int32_t* object;  // SRT_GBUF_OBJECT
    float* variance;        // the output
    int width, height;
    float samples;          // n of the temporal call that wrote the records
    float old_length;       // min_frames * n: a record at least this long is used alone
};

constexpr int MT_MAX_RADIUS = 3;
constexpr int MT_PITCH = 24;  // entries per tile row
static_assert(WG_W + 2 * MT_MAX_RADIUS <= MT_PITCH, "a tile row must fit its pitch");

template <int R>
__global__ void __launch_bounds__(WG_THREADS) temporal_variance_kernel(const MomentsLaunch M) {
    constexpr int TW = WG_W + 2 * R, TH = WG_H + 2 * R;
    // (M1, M2, object as bits, 1); object -2 outside the frame.  The 1 is the tap's count: with all four components in use the
    // read stays one ds_read_b128
    __shared__ float4 tile[TH * MT_PITCH];
    const TilePixel tp = tile_pixel();
    const int lx = tp.lx, ly = tp.ly, x = tp.x, y = tp.y;
    const int W = M.width, H = M.height;
    const bool inside = x < W && y < H;
    const size_t p = (size_t)x + (size_t)y * (size_t)W;
    int op = -1;
    float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (inside) {
        op = M.object[p];
        if (op >= 0) m = M.moments[p];
    }
    const bool young = op >= 0 && !(m.z >= M.old_length);
    float s = fmaxf(0.0f, m.y - m.x * m.x);  // the temporal estimate
    if (__syncthreads_or(young)) {  // (uniform over the workgroup: every thread takes the same side)
        const int x0 = (int)blockIdx.x * WG_W - R, y0 = (int)blockIdx.y * WG_H - R;
        for (int i = (int)threadIdx.x; i < TW * TH; i += WG_THREADS) {
            const int ty = i / TW, tx = i - ty * TW;
            const int gx = x0 + tx, gy = y0 + ty;
            int o = -2;
            float m1 = 0.0f, m2 = 0.0f;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const size_t g = (size_t)gx + (size_t)gy * (size_t)W;
                o = M.object[g];
                if (o >= 0) {  // (a miss is no tap: its record is not needed)
                    const float4 r = M.moments[g];
                    m1 = r.x, m2 = r.y;
                }
            }
            tile[ty * MT_PITCH + tx] = make_float4(m1, m2, __int_as_float(o), 1.0f);
        }
        __syncthreads();
        if (young) {  // a wave without a young lane skips the loop
            const int tc = (ly + R) * MT_PITCH + lx + R;
            float a1 = 0.0f, a2 = 0.0f, cnt = 0.0f;
#pragma unroll
            for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
                for (int dx = -R; dx <= R; ++dx) {
                    const float4 t = tile[tc + dy * MT_PITCH + dx];
                    if (__float_as_int(t.z) != op) continue;  // outside the frame or another object (the centre always counts)
                    a1 = a1 + t.x;
                    a2 = a2 + t.y;
                    cnt = cnt + t.w;
                }
            }
            a1 = a1 / cnt;
            a2 = a2 / cnt;
            s = fmaxf(0.0f, a2 - a1 * a1);
        }
    }
    if (inside) M.variance[p] = op >= 0 ? s * (M.samples / m.z) : 0.0f;
}

}  // namespace srt
