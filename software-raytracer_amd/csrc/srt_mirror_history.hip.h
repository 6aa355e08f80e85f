// srt_mirror_history.hip.h — gfx950 temporal reprojection with the mirror history on (srt_mirror_history): the pixel routine of
// srt_temporal.hip.h, told by the reflection guides (srt_reflection.hip.h) which pixels look through a chain of J >= 1 mirrors.
//
// Such a pixel shows the surface at the END of its chain, so its history is where that surface's virtual image was: the point
// y = C + (x0 - C) * (D / t0) on the pixel's own camera ray at the chain's path length D (exact for a flat mirror).  If that
// footprint counts no tap the mirror's own surface point x0 is tried (a strongly curved mirror keeps its image near its
// surface).  A tap of a mirror pixel counts only when it looked through the same mirror over a chain of the same length (the
// tag kept in the history's normal.w, a word that is 0 without the mode), ended on the same object, and its terminal point
// lies within r = rho * D of the pixel's: so a mirror pixel either finds the history of what it shows or restarts, and never
// carries the history of the mirror's surface across a reflected edge.  Pixels without a mirror run srt_temporal.hip.h's
// arithmetic operation for operation, plus the test tag' == 0.
//
// A routine of its own and a launch struct of its own: temporal_pixel, TemporalLaunch and the kernels made from them are not
// touched, and a context with the mode off launches exactly those.  Work shape as theirs: a wave per 8 x 8 tile, four waves
// per workgroup, one launch, no LDS, no atomics, no scratch.  A mirror pixel adds 4 + 16 + 16 + 4 bytes of guide loads (every
// pixel the 4 of BOUNCES) and up to four more taps; every tap that passes the object test now loads its normal row, for the tag.
#pragma once

#include "srt_mirror_history_host.h"  // MIRROR_TAG_SHIFT
#include "srt_temporal.hip.h"

namespace srt {

struct MirrorLaunch {
    TemporalLaunch T;              // as srt_temporal_accumulate fills it for the plain kernels
    const int32_t* r_object;       // SRT_REFL_OBJECT: terminal object o_p, -1 when the chain leaves the scene
    const float4* r_normal_depth;  // SRT_REFL_NORMAL_DEPTH: terminal normal, w = path length D_p
    const float4* r_position;      // SRT_REFL_POSITION: terminal point x_p
    const int32_t* r_bounces;      // SRT_REFL_BOUNCES: J_p
    float cam[3];                  // C: the current camera's position
    float rho;                     // the angle of radius_pixels pixels
};

// the counted taps of one footprint under the bilinear weights
struct MirrorTaps {
    float sw, sr, sg, sb, sl;
    float s1, s2, sm;  // MOM
};

// Steps 2 and 3 for the point y: project it into the previous camera, test the window, walk the 2 x 2 footprint.  A tap counts
// when its stored object is `obj`, its stored tag is `tag`, its stored point passes the distance test against `ref` (ball:
// within sqrt(bound) of it; else: within bound of the plane through it with normal n) and its stored normal the normal test
// against n.  in_window and (u, v) report step 2 for the motion output.
template <bool MOM>
__device__ __forceinline__ MirrorTaps mirror_footprint(const TemporalLaunch& T, const float yx, const float yy, const float yz, const bool ball,
                                                       const int obj, const int tag, const float4 n, const float4 ref, const float bound,
                                                       bool& in_window, float& u_out, float& v_out) {
    MirrorTaps s{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    in_window = false;
    const int W = T.width, H = T.height;
    const float rx = yx - T.cam_pos[0], ry = yy - T.cam_pos[1], rz = yz - T.cam_pos[2];
    const float a = T.inv[0] * rx + T.inv[1] * ry + T.inv[2] * rz;
    const float b = T.inv[3] * rx + T.inv[4] * ry + T.inv[5] * rz;
    const float g = T.inv[6] * rx + T.inv[7] * ry + T.inv[8] * rz;
    if (!(g > 0.0f)) return s;
    const float u = (a / g + 1.0f) * ((float)W * 0.5f);
    const float v = (b / g + 1.0f) * ((float)H * 0.5f);
    // (as temporal_pixel: keeps NaN and huge values away from the integer conversion)
    if (!(u > -1.0f && u < (float)W && v > -1.0f && v < (float)H)) return s;
    in_window = true;
    u_out = u, v_out = v;
    const float fu = floorf(u), fv = floorf(v);
    const int x0 = (int)fu, y0 = (int)fv;
    const float fx = u - fu, fy = v - fv;
    const bool use_n = T.normal_threshold > -1.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
        const float w = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
        if (w <= 0.0f || qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        const size_t q = (size_t)qx + (size_t)qy * (size_t)W;
        const float4 po = T.prev.pos_object[q];
        if (__float_as_int(po.w) != obj) continue;  // another object, a miss or a chain that left the scene
        const float4 nq = T.prev.normal[q];
        if (__float_as_int(nq.w) != tag) continue;  // seen directly / through another mirror / over a chain of another length
        const float dx = po.x - ref.x, dy = po.y - ref.y, dz = po.z - ref.z;
        if (ball) {
            if (!(((dx * dx + dy * dy) + dz * dz) <= bound)) continue;
        } else {
            const float d = n.x * dx + n.y * dy + n.z * dz;
            if (!(fabsf(d) <= bound)) continue;
        }
        if (use_n && !(n.x * nq.x + n.y * nq.y + n.z * nq.z >= T.normal_threshold)) continue;
        const float4 h = T.prev.color[q];
        s.sw = s.sw + w;
        s.sr = s.sr + w * h.x;
        s.sg = s.sg + w * h.y;
        s.sb = s.sb + w * h.z;
        s.sl = s.sl + w * h.w;
        if (MOM && T.mom_valid) {
            const float4 m = T.mom_prev[q];
            s.s1 = s.s1 + w * m.x;
            s.s2 = s.s2 + w * m.y;
            s.sm = s.sm + w * m.z;
        }
    }
    return s;
}

// MOTION, MV, MOM: temporal_pixel's options (include/srt_pathtrace.h, "mirror history", for what they mean to a mirror pixel).
template <bool MOTION, bool MV, bool MOM>
__device__ __forceinline__ void mirror_temporal_pixel(const MirrorLaunch& M) {
    const TemporalLaunch& T = M.T;
    const TilePixel tp = tile_pixel();
    const int x = tp.x, y = tp.y;
    const int W = T.width, H = T.height;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)x + (size_t)y * (size_t)W;
    const int op = T.object[p];  // m_p: the first hit
    if (op < 0) {  // first-hit miss (J = 0): as temporal_pixel
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
    const bool mirror = M.r_bounces[p] >= 1;
    // what the history stores: the first hit, or the end of the chain under the pixel's tag
    int so = op, tag = 0;
    float4 sn = nd, sx = xx;
    if (mirror) {
        so = M.r_object[p];
        sn = M.r_normal_depth[p];
        sx = M.r_position[p];
        tag = (int)((unsigned)M.r_bounces[p] * (unsigned)MIRROR_TAG_SHIFT + (unsigned)op);
    }
    float mu = 0.0f, mv = 0.0f;
    MirrorTaps s{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (T.valid && !mirror) {  // M2: today's rule and tag' == 0
        float4 xt = xx;  // x~_p
        bool keep = true;
        if (MOTION && op < T.table_count) {
            const float4 row = T.table[op];
            xt = make_float4(xx.x - row.x, xx.y - row.y, xx.z - row.z, 0.0f);
            keep = row.w != 0.0f;
        }
        if (keep) {
            bool in_window;
            float u, v;
            s = mirror_footprint<MOM>(T, xt.x, xt.y, xt.z, false, op, 0, nd, xt, T.plane_tolerance * nd.w, in_window, u, v);
            if (MV && in_window) mu = u - (float)x, mv = v - (float)y;
        }
    } else if (T.valid && !MOTION && so >= 0) {  // M4 (M5: no history under a displacement table; M3: none for reflected sky)
        const float r = M.rho * sn.w;
        const float scale = sn.w / nd.w;
        bool in1, in2;
        float u1, v1, u2, v2;
        // candidate 1: the virtual point on the pixel's own ray at the path length
        s = mirror_footprint<MOM>(T, M.cam[0] + (xx.x - M.cam[0]) * scale, M.cam[1] + (xx.y - M.cam[1]) * scale,
                                  M.cam[2] + (xx.z - M.cam[2]) * scale, true, so, tag, sn, sx, r * r, in1, u1, v1);
        if (MV && in1) mu = u1 - (float)x, mv = v1 - (float)y;
        if (!(s.sw > 0.0f)) {
            // candidate 2: the mirror's own surface
            const MirrorTaps s2 = mirror_footprint<MOM>(T, xx.x, xx.y, xx.z, true, so, tag, sn, sx, r * r, in2, u2, v2);
            if (s2.sw > 0.0f) {
                s = s2;
                if (MV) mu = u2 - (float)x, mv = v2 - (float)y;
            }
        }
    }
    const float sw = s.sw;
    if (MOM) {
        // this frame's luminance, as temporal_pixel takes it
        float lum;
        if (T.albedo) {
            const float4 a4 = T.albedo[p];
            lum = luminance(c.x / demod_factor(a4.x), c.y / demod_factor(a4.y), c.z / demod_factor(a4.z));
        } else {
            lum = luminance(c.x, c.y, c.z);
        }
        float m1 = lum, m2 = lum * lum, lm = T.samples;
        if (T.mom_valid && sw > 0.0f) {
            lm = fminf(s.sm / sw + T.samples, T.max_samples);
            const float al = T.samples / lm, bl = 1.0f - al;
            m1 = bl * (s.s1 / sw) + al * lum;
            m2 = bl * (s.s2 / sw) + al * (lum * lum);
        }
        T.mom_next[p] = make_float4(m1, m2, lm, 0.0f);
    }
    float4 out = c;
    float L = T.samples;
    if (sw > 0.0f) {
        const float inv_w = 1.0f / sw;
        L = fminf(s.sl * inv_w + T.samples, T.max_samples);
        const float al = T.samples / L, bl = 1.0f - al;
        out = make_float4(bl * (s.sr * inv_w) + al * c.x, bl * (s.sg * inv_w) + al * c.y, bl * (s.sb * inv_w) + al * c.z, c.w);
        T.acc[p] = out;
    }
    T.next.color[p] = make_float4(out.x, out.y, out.z, L);
    T.next.pos_object[p] = make_float4(sx.x, sx.y, sx.z, __int_as_float(so));
    T.next.normal[p] = make_float4(sn.x, sn.y, sn.z, __int_as_float(tag));
    if (T.framebuffer) T.framebuffer[(size_t)(H - 1 - y) * W + x] = tone_map(out);
    if (MV) T.motion[p] = make_float4(mu, mv, sw, 0.0f);
}

// srt_temporal_accumulate with the mirror history on, over temporal_pixel's options
template <bool MOTION, bool MV, bool MOM>
__global__ void __launch_bounds__(WG_THREADS) temporal_mirror_kernel(const MirrorLaunch M) {
    mirror_temporal_pixel<MOTION, MV, MOM>(M);
}

}  // namespace srt
