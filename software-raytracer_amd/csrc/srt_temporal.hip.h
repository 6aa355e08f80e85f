// srt_temporal.hip.h — gfx950 temporal reprojection (srt_temporal_accumulate): the accumulator of the current camera is
// blended with the history of the previous call, reprojected through the previous camera, so that a moving camera keeps
// the samples it has already taken (the temporal stage of SVGF, Schied et al. 2017, without the variance estimate).
//
// One launch per call.  Each pixel projects its own first-hit point x_p into the previous camera (the host passes B'^-1,
// the inverse of the previous frame's ray basis, see include/srt_pathtrace.h), takes the 2 x 2 bilinear footprint there,
// tests every tap against the stored guides of the previous call (object, plane distance, normal) and blends the counted
// taps' colour and history length.  The history lives in two slots: the launch reads slot A and writes slot B, so no pixel
// reads what another writes and no grid-wide barrier is needed.
// Work shape as atrous_kernel: a wave per 8 x 8 tile (lane -> x = lane & 7, y = lane >> 3), four waves per workgroup
// (16 x 16 pixels), so every float4 row segment a wave touches is one 128-byte line.  No LDS, no atomics, no scratch.
// Moving objects (srt_update_scene) add a per-object table (displacement since the previous call, keep flag), a per-lane
// 16-byte gather keyed by the pixel's object index; srt_motion_output adds one float4 store per pixel.  Both are template
// options of the one pixel routine, and the call that uses neither runs temporal_kernel as it always was.
// srt_moments_output adds a second history that rides the same reprojection: one float4 (M1, M2, Lm, 0) per pixel, the running
// first and second moments of the frames' luminance and their own length, blended over the taps the colour blend counts with
// the same weights (up to four more 16-byte loads and one more 16-byte store per pixel, and the albedo when demodulating).  It
// is a third template option; srt_moments.hip.h turns the records into a variance.
#pragma once

#include "srt_kernel.hip.h"
#include "srt_variance.hip.h"  // luminance, demod_factor

namespace srt {

// One history slot: three W*H float4 arrays, index x + y * width, SCENE rows.
struct TemporalSlot {
    float4* color;       // result rgb, history length L in w (0 on a miss)
    float4* pos_object;  // x_p xyz, object index o_p in w (as int bits; -1 on a miss)
    float4* normal;      // n_p xyz, 0
};

struct TemporalLaunch {
    float4* acc;                 // the accumulator: read, and its rgb replaced in place (alpha rewritten with its own bits)
    const int32_t* object;       // SRT_GBUF_OBJECT
    const float4* normal_depth;  // SRT_GBUF_NORMAL_DEPTH: n xyz, d w
    const float4* position;      // SRT_GBUF_POSITION: x xyz
    TemporalSlot prev;           // the previous call's history (read only when valid)
    TemporalSlot next;           // this call's history (written for every pixel)
    uint32_t* framebuffer;       // SRT_TEMPORAL_FRAMEBUFFER, else NULL (memory row H - 1 - y)
    int width, height;
    int valid;                   // the previous slot holds a history for this scene
    float inv[9];                // B'^-1, row-major
    float cam_pos[3];            // C'.position
    float samples;               // n
    float max_samples;           // L_max
    float plane_tolerance;       // sigma_t
    float normal_threshold;      // <= -1: term off
    // object motion and the motion-vector output (srt_update_scene, srt_motion_output); appended behind the fields above so
    // that the plain instantiation reads its arguments where it always did
    const float4* table;         // MOTION: table_count rows (position now - position at the previous call, keep), else unused
    int table_count;             // rows of the table; an object index beyond it (bound guides) has moved by 0 and is kept
    float4* motion;              // MV: W*H rows (u - x, v - y, sum of the counted taps' weights, 0), else unused
    // the moments history (srt_moments_output), appended in the same way
    const float4* mom_prev;      // MOM: the previous call's records (M1, M2, Lm, 0), read only when mom_valid; else unused
    float4* mom_next;            // MOM: this call's records, written for every pixel
    const float4* albedo;        // MOM: SRT_GBUF_ALBEDO when the luminance is demodulated, else NULL
    int mom_valid;               // MOM: mom_prev belongs to the history `prev` and was written with the same flags
};

// MOTION: the hit object's row of T.table moves x_p back to where the object was at the previous call (x~_p = x_p - delta),
// and a row with keep == 0 (the object was reshaped or recoloured) leaves the pixel without history.  MV: T.motion is written.
// MOM: T.mom_next is written (include/srt_pathtrace.h, "moments"); no other value depends on it.
template <bool MOTION, bool MV, bool MOM = false>
__device__ __forceinline__ void temporal_pixel(const TemporalLaunch& T) {
    const TilePixel tp = tile_pixel();
    const int x = tp.x, y = tp.y;
    const int W = T.width, H = T.height;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)x + (size_t)y * (size_t)W;
    const int op = T.object[p];
    if (op < 0) {  // miss: the accumulator untouched, L = 0, never a tap
        T.next.color[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        T.next.pos_object[p] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
        T.next.normal[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (T.framebuffer) T.framebuffer[(size_t)(H - 1 - y) * W + x] = tone_map(T.acc[p]);
        if (MV) T.motion[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (MOM) T.mom_next[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 c = T.acc[p];
    const float4 nd = T.normal_depth[p];
    const float4 xx = T.position[p];
    float4 xt = xx;  // x~_p
    bool keep = true;
    if (MOTION && op < T.table_count) {
        const float4 row = T.table[op];
        xt = make_float4(xx.x - row.x, xx.y - row.y, xx.z - row.z, 0.0f);
        keep = row.w != 0.0f;
    }
    float mu = 0.0f, mv = 0.0f;
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sl = 0.0f;
    float s1 = 0.0f, s2 = 0.0f, sm = 0.0f;  // MOM: the counted taps' M1', M2' and Lm' under the colour blend's weights
    if (T.valid && keep) {
        const float rx = xt.x - T.cam_pos[0], ry = xt.y - T.cam_pos[1], rz = xt.z - T.cam_pos[2];
        const float a = T.inv[0] * rx + T.inv[1] * ry + T.inv[2] * rz;
        const float b = T.inv[3] * rx + T.inv[4] * ry + T.inv[5] * rz;
        const float g = T.inv[6] * rx + T.inv[7] * ry + T.inv[8] * rz;
        if (g > 0.0f) {
            const float u = (a / g + 1.0f) * ((float)W * 0.5f);
            const float v = (b / g + 1.0f) * ((float)H * 0.5f);
            // some tap of positive weight lies inside the frame only for u in (-1, W) and v in (-1, H) (also keeps NaN and
            // huge values away from the integer conversion)
            if (u > -1.0f && u < (float)W && v > -1.0f && v < (float)H) {
                if (MV) mu = u - (float)x, mv = v - (float)y;
                const float fu = floorf(u), fv = floorf(v);
                const int x0 = (int)fu, y0 = (int)fv;
                const float fx = u - fu, fy = v - fv;
                const float tol = T.plane_tolerance * nd.w;
                const bool use_n = T.normal_threshold > -1.0f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
                    const float w = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
                    if (w <= 0.0f || qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const size_t q = (size_t)qx + (size_t)qy * (size_t)W;
                    const float4 po = T.prev.pos_object[q];
                    if (__float_as_int(po.w) != op) continue;  // another object or a miss
                    const float d = nd.x * (po.x - xt.x) + nd.y * (po.y - xt.y) + nd.z * (po.z - xt.z);
                    if (!(fabsf(d) <= tol)) continue;
                    if (use_n) {
                        const float4 nq = T.prev.normal[q];
                        if (!(nd.x * nq.x + nd.y * nq.y + nd.z * nq.z >= T.normal_threshold)) continue;
                    }
                    const float4 h = T.prev.color[q];
                    sw = sw + w;
                    sr = sr + w * h.x;
                    sg = sg + w * h.y;
                    sb = sb + w * h.z;
                    sl = sl + w * h.w;
                    if (MOM && T.mom_valid) {
                        const float4 m = T.mom_prev[q];
                        s1 = s1 + w * m.x;
                        s2 = s2 + w * m.y;
                        sm = sm + w * m.z;
                    }
                }
            }
        }
    }
    if (MOM) {
        // this frame's luminance: the accumulator as the call finds it, demodulated like srt_variance's halves
        float lum;
        if (T.albedo) {
            const float4 a4 = T.albedo[p];
            lum = luminance(c.x / demod_factor(a4.x), c.y / demod_factor(a4.y), c.z / demod_factor(a4.z));
        } else {
            lum = luminance(c.x, c.y, c.z);
        }
        float m1 = lum, m2 = lum * lum, lm = T.samples;
        if (T.mom_valid && sw > 0.0f) {
            lm = fminf(sm / sw + T.samples, T.max_samples);
            const float al = T.samples / lm, bl = 1.0f - al;
            m1 = bl * (s1 / sw) + al * lum;
            m2 = bl * (s2 / sw) + al * (lum * lum);
        }
        T.mom_next[p] = make_float4(m1, m2, lm, 0.0f);
    }
    float4 out = c;
    float L = T.samples;
    if (sw > 0.0f) {
        const float inv_w = 1.0f / sw;
        L = fminf(sl * inv_w + T.samples, T.max_samples);
        const float al = T.samples / L, bl = 1.0f - al;
        out = make_float4(bl * (sr * inv_w) + al * c.x, bl * (sg * inv_w) + al * c.y, bl * (sb * inv_w) + al * c.z, c.w);
        T.acc[p] = out;
    }
    T.next.color[p] = make_float4(out.x, out.y, out.z, L);
    T.next.pos_object[p] = make_float4(xx.x, xx.y, xx.z, __int_as_float(op));
    T.next.normal[p] = make_float4(nd.x, nd.y, nd.z, 0.0f);
    if (T.framebuffer) T.framebuffer[(size_t)(H - 1 - y) * W + x] = tone_map(out);
    if (MV) T.motion[p] = make_float4(mu, mv, sw, 0.0f);
}

// the call without object motion and without the motion output
__global__ void __launch_bounds__(WG_THREADS) temporal_kernel(const TemporalLaunch T) { temporal_pixel<false, false>(T); }

// ... and with either or both
template <bool MOTION, bool MV>
__global__ void __launch_bounds__(WG_THREADS) temporal_motion_kernel(const TemporalLaunch T) {
    temporal_pixel<MOTION, MV>(T);
}

// ... and any of the four with the moments history (srt_moments_output)
template <bool MOTION, bool MV>
__global__ void __launch_bounds__(WG_THREADS) temporal_moments_kernel(const TemporalLaunch T) {
    temporal_pixel<MOTION, MV, true>(T);
}

}  // namespace srt
