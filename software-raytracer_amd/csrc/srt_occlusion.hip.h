// srt_occlusion.hip.h — gfx950 any-hit queries for caller-supplied segments (srt_trace_occlusion): for ray i of a batch, is there
// an object whose Raytrace(origin[i], direction[i]) reports a valid hit with distance < t_max[i]?  That predicate equals
// "GetClosestObject's distance < t_max" — the minimum of the valid distances is below t_max exactly when one of them is — so the
// output is, bit for bit, what rays_kernel writes for SRT_RAYS_OCCLUDED.  What differs is the work: a ray knows how far it has to
// look, needs one bit, and stops at its first occluder.
//
// Launched, sized and staged exactly like rays_kernel (persistent workgroups, make_lds with four waves, 64 consecutive rays per
// wave block, 16-byte ray loads).  any_hit is a function of its own — closest_hit is not touched — that keeps a per-lane `open`
// flag (active and not yet occluded); every phase ends as soon as the wave's ballot of `open` is empty:
//   0. segment culling: t_max = NaN closes the lane (no distance is below a NaN).  With t_max <= 0 nothing with a distance
//      window can occlude — Box::Raytrace and the triangle test report t >= 0.01 only — which leaves Sphere::Raytrace, whose
//      distance tc - sqrt(r*r - d2) is negative for an origin inside the sphere.  Such lanes run a sphere-only scan behind a
//      conservative inside test (proof at `inside`) and close; from outside every sphere they evaluate nothing.
//   1. uniform spheres, one broadcast row per trip, the arithmetic of closest_hit's part1 / candidates (same bits, the short
//      square root under SCENE_LDS included); a lane leaves at its first sphere with t1 < t_max.
//   2. clustered spheres: closest_hit's conservative cluster bounds give each lane its clusters; the lane then walks its own
//      clusters sphere by sphere (per-lane LDS gather) and leaves at the first occluder.  No work list and no merge: there is
//      nothing to merge, and the early out makes the rounds short.  Non-unit directions take the brute-force scan, as there.
//   3. boxes: box_ray_setup / ibox_dist as closest_hit calls them.
//   4. meshes: closest_hit's root-box and bounding-sphere tests with best = t_max, then its wave-cooperative traversal of the
//      8-wide quantized BVH with t_max as the (constant) culling distance.  A triangle with t < t_max sets the ray's word in LDS
//      (an OR of ones, written as a plain store of 1: idempotent, as the key merge is under atomicMin, so the abandon-and-redo
//      overflow scheme carries over) and the ray's remaining items are dropped as they are popped.
// Work counts (COUNT instantiations only): lane-level tests executed for rays of the batch, accumulated per wave in scalar
// registers and added to a handle-owned record with ONE vector atomic per wave at the end.  Without COUNT there is no atomic.
#pragma once

#include "srt_kernel.hip.h"

namespace srt {

enum { OCC_WORK_RAYS = 0, OCC_WORK_OCCLUDED, OCC_WORK_ANALYTIC, OCC_WORK_NODES, OCC_WORK_TRIANGLES, OCC_WORK_N };

struct OcclusionIO {
    const float4* origin;      // (o.xyz, ignored)
    const float4* direction;   // (d.xyz, t_max)
    uint32_t count;            // rays, 1 .. 2^30
    uint32_t normalize;        // SRT_OCCLUSION_NORMALIZE: d = float3::Normalized(d) first
    int32_t* occluded;         // 1: some object reports a valid hit with distance < t_max; else 0
    unsigned long long* work;  // COUNT: [OCC_WORK_N] totals of the launch (zeroed by the host before it)
};

// per-wave work counts: wave-uniform 64-bit sums of ballot populations
template <bool ON>
struct OccWork {
    __device__ __forceinline__ void add(int, unsigned long long) {}
};
template <>
struct OccWork<true> {
    unsigned long long n[OCC_WORK_N] = {0ull, 0ull, 0ull, 0ull, 0ull};
    __device__ __forceinline__ void add(int i, unsigned long long lanes) { n[i] += (unsigned long long)__builtin_popcountll(lanes); }
};

// Is there a valid hit with distance < t_max?  Must be called from wave-uniform control flow; lanes with active == false take
// part in the cooperative mesh phase but trace nothing themselves and count nothing.
template <bool MESH, bool COUNT, bool SHORT_SQRT>
__device__ __forceinline__ bool any_hit(const Lds& S, const KernelParams& P, V3 o, V3 d, float t_max, bool active, OccWork<COUNT>& W) {
    bool occ = false;
    // Sphere::line_sphere_intersection (Object.hpp:104-141) as closest_hit's part1 + candidates spell it: the same expressions,
    // so the same bits; the square root only when some lane has a candidate
    auto sphere_hits = [&](const float4 s, bool on) {
        float Lx = s.x - o.x, Ly = s.y - o.y, Lz = s.z - o.z;                    // :115
        float tc = fabsf((Lx * d.x + Ly * d.y) + Lz * d.z);                      // :118-119
        float qx = d.x * tc + o.x, qy = d.y * tc + o.y, qz = d.z * tc + o.z;     // :121
        float ex = qx - s.x, ey = qy - s.y, ez = qz - s.z;                       // :124
        float d2 = (ex * ex + ey * ey) + ez * ez;                                // :125
        const bool c = on && !(d2 > s.w);                                        // :127
        bool hit = false;
        if (__builtin_amdgcn_ballot_w64(c) != 0ull) {
            const float x = s.w - d2;
            const float t1 = tc - (SHORT_SQRT ? sqrt_window(x) : sqrtf(x));  // :131-133
            hit = c & (t1 < t_max);                                         // (a NaN distance never records: Raytracer.cpp:132)
        }
        return hit;
    };
    // one sphere row for the lanes `want` that are not occluded yet; false when no lane is left
    auto scan_row = [&](int row, bool want) {
        const bool on = want && !occ;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(on);
        if (m == 0ull) return false;
        W.add(OCC_WORK_ANALYTIC, m);
        occ = occ | sphere_hits(S.v[row], on);
        return true;
    };
    const float dd = __builtin_fmaf(d.z, d.z, __builtin_fmaf(d.y, d.y, d.x * d.x));
    const bool unit = fabsf(dd - 1.0f) <= 1e-6f;  // false for NaN
    const float o1 = (fabsf(o.x) + fabsf(o.y)) + fabsf(o.z);
    // ---- 0. segment culling
    bool open = active && t_max == t_max;
    const bool back = open && !(t_max > 0.0f);
    if (__builtin_amdgcn_ballot_w64(back) != 0ull) {
        // t1 = tc - sqrt(r*r - d2) < t_max <= 0 needs sqrt(r*r - d2) > tc, i.e. (every rounding is monotone, eps = 2^-24)
        // r*r - d2 > tc^2 * (1 - 4 eps).  For |d.d - 1| <= 1e-6 the proof of srt_scene_image.h bounds d2 from below by
        // D^2 - [4.2e-7 * D * (|L| + |o|) + 4e-7 * D^2 + 2e-12 * |L|^2] (D: distance of the centre from the line, L = c - o; for a
        // sphere behind the ray d2 >= |L|^2 outright), and tc^2 >= (L.d)^2 - 4e-7 * |L|^2 >= (|L|^2 - D^2) * (1 - 1e-6) - 4e-7 * |L|^2.
        // With D <= |L| and |L| * |o| <= (|L|^2 + |o|^2) / 2 this gives  r*r > |L|^2 * (1 - 3e-6) - 2.1e-7 * (|L|^2 + |o|_1^2):
        // the origin lies inside the (slightly inflated) sphere.  The test below has more than twice that slack over the
        // 3e-7 * LL its own FMA chain may be off by, so "not inside" implies t1 >= 0: the sphere cannot occlude this segment.
        // Directions that are not unit length take every sphere, as closest_hit's brute-force scan does.
        auto inside = [&](const float4 s) {
            const float Lx = s.x - o.x, Ly = s.y - o.y, Lz = s.z - o.z;
            const float LL = __builtin_fmaf(Lz, Lz, __builtin_fmaf(Ly, Ly, Lx * Lx));
            return !unit || LL <= __builtin_fmaf(1e-5f, __builtin_fmaf(o1, o1, LL), s.w);
        };
        for (int j = 0; j < S.nsT; ++j) {
            if (j == S.nu) j = S.nu4;  // (the uniform group's padding)
            if (j >= S.nsT || __builtin_amdgcn_ballot_w64(back && !occ) == 0ull) break;
            scan_row(j, back && inside(S.v[j]));
        }
        open = open && !back;  // boxes and triangles report t >= 0.01 only
    }
    // ---- 1. uniform spheres
    for (int j = 0; j < S.nu; ++j)
        if (!scan_row(j, open)) break;
    // ---- 2. clustered spheres
    if (S.nc > 0 && __builtin_amdgcn_ballot_w64(open && !occ) != 0ull) {
        if (__builtin_amdgcn_ballot_w64(open && !occ && !unit) == 0ull) {
            // closest_hit's conservative cluster bounds (srt_scene_image.h): a cluster that fails holds no candidate
            auto passes = [&](int k) {
                const float4 b = S.bound(k);
                float Lx = b.x - o.x, Ly = b.y - o.y, Lz = b.z - o.z;
                float LL = __builtin_fmaf(Lz, Lz, __builtin_fmaf(Ly, Ly, Lx * Lx));
                float sd = __builtin_fmaf(Lz, d.z, __builtin_fmaf(Ly, d.y, Lx * d.x));
                float Rinf = __builtin_fmaf(8e-6f, o1, b.w);
                float lhs = __builtin_fmaf(-sd, sd, LL);
                float rhs = __builtin_fmaf(4e-6f, LL, Rinf * Rinf);
                return lhs <= rhs ? 1ull : 0ull;
            };
            unsigned long long mask = 0ull;
            for (int k = 0; k < S.nc; ++k) mask |= passes(k) << k;  // (nc <= 64)
            if (!(open && !occ)) mask = 0ull;
            // every lane walks its own clusters, lowest first, and each cluster sphere by sphere
            while (__builtin_amdgcn_ballot_w64(mask != 0ull) != 0ull) {
                const bool has = mask != 0ull;
                const int k = has ? __builtin_ctzll(mask) : 0;
                mask &= mask - 1ull;
                const int first = S.nu4 + k * S.K;
                for (int i = 0; i < S.K; ++i) {
                    const bool on = has && !occ;
                    const unsigned long long m = __builtin_amdgcn_ballot_w64(on);
                    if (m == 0ull) break;
                    W.add(OCC_WORK_ANALYTIC, m);
                    occ = occ | sphere_hits(S.v[first + i], on);  // per-lane gather
                }
                if (occ) mask = 0ull;
            }
        } else {  // some lane's direction is not unit length: every clustered sphere
            for (int j = S.nu4; j < S.nsT; ++j)
                if (!scan_row(j, open)) break;
        }
    }
    // ---- 3. boxes
    if (S.nb > 0 && __builtin_amdgcn_ballot_w64(open && !occ) != 0ull) {
        const BoxRay br = box_ray_setup(d);
        const float dsum = (d.x + d.y) + d.z;
        const bool no_nan = (P.flags & KF_BOXES_FINITE) != 0 && __builtin_amdgcn_ballot_w64(active && !(o1 < 1e29f && fabsf(dsum) < __builtin_inff())) == 0ull;
        auto boxes = [&](auto tag) {
            for (int j = 0; j < S.nb; ++j) {
                const bool on = open && !occ;
                const unsigned long long m = __builtin_amdgcn_ballot_w64(on);
                if (m == 0ull) break;
                W.add(OCC_WORK_ANALYTIC, m);
                const float4 c = S.box_c(j), hs = S.box_h(j);
                V3 t1;
                const float dist = ibox_dist<decltype(tag)::value>(br, v3(o.x - c.x, o.y - c.y, o.z - c.z), v3(hs.x, hs.y, hs.z), t1);
                occ = occ | (on & (dist != 3.402823466e+38f) & (dist < t_max));  // Object.hpp:231
            }
        };
        if (no_nan) boxes(std::true_type{});
        else boxes(std::false_type{});
    }
    // ---- 4. triangle meshes: closest_hit's step 4 with best = t_max
    if constexpr (MESH) {
        if (P.n_tris > 0 && __builtin_amdgcn_ballot_w64(open && !occ) != 0ull) {
            const float best = t_max;
            const float pad = 1e-5f * (((fabsf(o.x - P.mesh_center[0]) + fabsf(o.y - P.mesh_center[1])) + fabsf(o.z - P.mesh_center[2])) + P.mesh_r1) + 1e-7f;
            const V3 inv = v3(__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z));
            const V3 rinv_own = v3(fminf(fmaxf(inv.x, -0x1p96f), 0x1p96f), fminf(fmaxf(inv.y, -0x1p96f), 0x1p96f), fminf(fmaxf(inv.z, -0x1p96f), 0x1p96f));
            bool go;
            {
                float t1x = ((P.mesh_center[0] - P.mesh_half[0] - pad) - o.x) * inv.x, t2x = ((P.mesh_center[0] + P.mesh_half[0] + pad) - o.x) * inv.x;
                float t1y = ((P.mesh_center[1] - P.mesh_half[1] - pad) - o.y) * inv.y, t2y = ((P.mesh_center[1] + P.mesh_half[1] + pad) - o.y) * inv.y;
                float t1z = ((P.mesh_center[2] - P.mesh_half[2] - pad) - o.z) * inv.z, t2z = ((P.mesh_center[2] + P.mesh_half[2] + pad) - o.z) * inv.z;
                float tmin = fmaxf(fmaxf(fminf(t1x, t2x), fminf(t1y, t2y)), fminf(t1z, t2z));
                float tmax = fminf(fminf(fmaxf(t1x, t2x), fmaxf(t1y, t2y)), fmaxf(t1z, t2z));
                go = open && !occ && tmin <= tmax * 1.00001f + 1e-6f && tmax * 1.00001f + 1e-6f >= MESH_T_MIN_CULL && tmin <= 10001.0f && tmin * 0.9999f - 1e-5f <= best;
            }
            {
                const float Lx = P.mesh_center[0] - o.x, Ly = P.mesh_center[1] - o.y, Lz = P.mesh_center[2] - o.z;
                const float LL = __builtin_fmaf(Lz, Lz, __builtin_fmaf(Ly, Ly, Lx * Lx));
                const float sd = __builtin_fmaf(Lz, d.z, __builtin_fmaf(Ly, d.y, Lx * d.x));
                const float Rp = P.mesh_bs_radius + 2.0f * pad;
                const float disc = __builtin_fmaf(4e-6f, LL, Rp * Rp) - __builtin_fmaf(-sd, sd, LL);
                const float q = __builtin_amdgcn_sqrtf(fmaxf(disc, 0.0f)) * 1.00001f;
                const bool inside = disc >= 0.0f && (sd + q) + pad >= MESH_T_MIN_CULL && ((sd - q) - pad) * 0.9999f - 1e-5f <= best;
                go = go && (inside || !unit);
            }
            unsigned long long pend = __builtin_amdgcn_ballot_w64(go);
            if (pend != 0ull) {
                const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                unsigned* qn = S.meshq;                // node item i at qn[i]
                unsigned* qlt = S.meshq + MESH_Q - 1;  // leaf item i at qlt[-i]
                unsigned* hitbit = reinterpret_cast<unsigned*>(S.res);  // [64] one word per ray lane: 1 = occluded by a triangle
                bool overflow = false;
                auto mbcnt64 = [](unsigned long long m) { return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)); };
                hitbit[lane] = 0u;
                // the culling distance is constant: <= (t_max + 1e-5) / 0.9999 (written as an upper bound of it), and <= 10001
                const float thr2_own = fminf(__builtin_fmaf(fabsf(best), 2e-4f, best + 1e-5f), 10001.0f);
                int batch = 64;
                bool strict = false;
                __builtin_amdgcn_wave_barrier();
                while (pend != 0ull) {
                    const bool mine = (pend >> lane) & 1ull;
                    const int rank = mbcnt64(pend);
                    const bool sel = mine && rank < batch;
                    const unsigned long long selmask = __builtin_amdgcn_ballot_w64(sel);
                    int nN = 0, nL = 0;
                    overflow = false;
                    {  // the selected rays enter at the root (at most 64 items: cannot overflow)
                        if (sel) qn[mbcnt64(selmask)] = (unsigned)lane << 26;
                        nN = __builtin_popcountll(selmask);
                    }
                    __builtin_amdgcn_wave_barrier();
                    while (!overflow && (nN > 0 || nL > 0)) {
                        const bool node_round = nN > 0 && nL < 64;
                        if (node_round) {
                            int logP = 3, takeN = 1;
                            if (!strict) {
                                logP = nN <= 8 ? 3 : nN <= 16 ? 2 : nN <= 32 ? 1 : 0;
                                takeN = nN < (64 >> logP) ? nN : (64 >> logP);
                                int room = (MESH_Q - nN - nL) / 6;  // (about 3 pushes per item to either queue)
                                room = room < 8 ? 8 : room;
                                takeN = takeN < room ? takeN : room;
                            }
                            nN -= takeN;  // the items [nN, nN + takeN) are popped
                            const int slotN = lane >> logP, sub = lane & ((1 << logP) - 1);
                            const bool popped = slotN < takeN;
                            const unsigned item = popped ? qn[nN + slotN] : 0u;
                            const int src = (int)(item >> 26), code = (int)(item & 0x3FFFFFFu);
                            const float4* rowp = P.bvh_nodes + 5 * (size_t)code;
                            const float4 h0 = rowp[0], h1 = rowp[1], q0 = rowp[2], q1 = rowp[3], q2 = rowp[4];
                            const V3 ro = v3(__shfl(o.x, src), __shfl(o.y, src), __shfl(o.z, src));
                            const V3 rinv = v3(__shfl(rinv_own.x, src), __shfl(rinv_own.y, src), __shfl(rinv_own.z, src));
                            const float rpad = __shfl(pad, src);
                            const float thr2 = __shfl(thr2_own, src);
                            const bool onN = popped && hitbit[src] == 0u;  // an occluded ray's items are dropped
                            W.add(OCC_WORK_NODES, __builtin_amdgcn_ballot_w64(onN && sub == 0));
                            const unsigned ex = __float_as_uint(h0.w);
                            const unsigned innermask = ex >> 24, lw = __float_as_uint(h1.z), leafmask = lw & 255u, counts = lw >> 8;
                            const float sx = __uint_as_float((ex & 255u) << 23) * rinv.x, sy = __uint_as_float(((ex >> 8) & 255u) << 23) * rinv.y,
                                        sz = __uint_as_float(((ex >> 16) & 255u) << 23) * rinv.z;
                            const float lx0 = ((h0.x - rpad) - ro.x) * rinv.x, hx0 = ((h0.x + rpad) - ro.x) * rinv.x;
                            const float ly0 = ((h0.y - rpad) - ro.y) * rinv.y, hy0 = ((h0.y + rpad) - ro.y) * rinv.y;
                            const float lz0 = ((h0.z - rpad) - ro.z) * rinv.z, hz0 = ((h0.z + rpad) - ro.z) * rinv.z;
                            const bool px = rinv.x >= 0.0f, py = rinv.y >= 0.0f, pz = rinv.z >= 0.0f;
                            const float bnx = px ? lx0 : hx0, bfx = px ? hx0 : lx0, bny = py ? ly0 : hy0, bfy = py ? hy0 : ly0, bnz = pz ? lz0 : hz0,
                                        bfz = pz ? hz0 : lz0;
                            const unsigned lox0 = __float_as_uint(q0.x), lox1 = __float_as_uint(q0.y), loy0 = __float_as_uint(q0.z), loy1 = __float_as_uint(q0.w);
                            const unsigned loz0 = __float_as_uint(q1.x), loz1 = __float_as_uint(q1.y), hix0 = __float_as_uint(q1.z), hix1 = __float_as_uint(q1.w);
                            const unsigned hiy0 = __float_as_uint(q2.x), hiy1 = __float_as_uint(q2.y), hiz0 = __float_as_uint(q2.z), hiz1 = __float_as_uint(q2.w);
                            auto byte_f = [](unsigned w, int b) { return (float)((w >> (8 * b)) & 255u); };
                            auto enters = [&](unsigned nx, unsigned ny, unsigned nz, unsigned fx, unsigned fy, unsigned fz, int b) {
                                const float tnx = __builtin_fmaf(byte_f(nx, b), sx, bnx), tfx = __builtin_fmaf(byte_f(fx, b), sx, bfx);
                                const float tny = __builtin_fmaf(byte_f(ny, b), sy, bny), tfy = __builtin_fmaf(byte_f(fy, b), sy, bfy);
                                const float tnz = __builtin_fmaf(byte_f(nz, b), sz, bnz), tfz = __builtin_fmaf(byte_f(fz, b), sz, bfz);
                                const float tn = fmaxf(fmaxf(tnx, tny), tnz), tf = fminf(fminf(tfx, tfy), tfz);
                                const float lo = (MESH_T_MIN_CULL > tn) ? MESH_T_MIN_CULL : tn;
                                const float hi = fminf(__builtin_fmaf(tf, 1.00001f, 1e-6f), thr2);
                                return lo <= hi;
                            };
                            unsigned mask = 0u;
                            if (logP == 0) {  // one lane per item: all 8 children
                                const unsigned nx0 = px ? lox0 : hix0, fx0 = px ? hix0 : lox0, ny0 = py ? loy0 : hiy0, fy0 = py ? hiy0 : loy0, nz0 = pz ? loz0 : hiz0,
                                               fz0 = pz ? hiz0 : loz0;
                                const unsigned nx1 = px ? lox1 : hix1, fx1 = px ? hix1 : lox1, ny1 = py ? loy1 : hiy1, fy1 = py ? hiy1 : loy1, nz1 = pz ? loz1 : hiz1,
                                               fz1 = pz ? hiz1 : loz1;
#pragma unroll
                                for (int b = 0; b < 4; ++b) {
                                    mask |= enters(nx0, ny0, nz0, fx0, fy0, fz0, b) ? (1u << b) : 0u;
                                    mask |= enters(nx1, ny1, nz1, fx1, fy1, fz1, b) ? (16u << b) : 0u;
                                }
                            } else {  // 2 / 4 / 8 lanes per item: this lane takes 4 / 2 / 1 consecutive children
                                const int nb = 8 >> logP;
                                const int first = sub * nb;
                                const bool second = first >= 4;
                                const unsigned sh = (unsigned)(first & 3) * 8u;
                                const unsigned wlx = (second ? lox1 : lox0) >> sh, wly = (second ? loy1 : loy0) >> sh, wlz = (second ? loz1 : loz0) >> sh;
                                const unsigned whx = (second ? hix1 : hix0) >> sh, why = (second ? hiy1 : hiy0) >> sh, whz = (second ? hiz1 : hiz0) >> sh;
                                const unsigned nx = px ? wlx : whx, fx = px ? whx : wlx, ny = py ? wly : why, fy = py ? why : wly, nz = pz ? wlz : whz, fz = pz ? whz : wlz;
                                unsigned m4 = enters(nx, ny, nz, fx, fy, fz, 0) ? 1u : 0u;
                                if (nb >= 2) {
                                    m4 |= enters(nx, ny, nz, fx, fy, fz, 1) ? 2u : 0u;
                                    if (nb == 4) {
                                        m4 |= enters(nx, ny, nz, fx, fy, fz, 2) ? 4u : 0u;
                                        m4 |= enters(nx, ny, nz, fx, fy, fz, 3) ? 8u : 0u;
                                    }
                                }
                                mask = m4 << first;
                            }
                            if (!onN) mask = 0u;
                            const unsigned tag = (unsigned)src << 26;
                            unsigned mi = mask & innermask, ml = mask & leafmask;
                            const unsigned both = (unsigned)__builtin_popcount(mi) | ((unsigned)__builtin_popcount(ml) << 16);
                            const unsigned incl = wave_inclusive_scan(both);
                            const unsigned total = (unsigned)__builtin_amdgcn_readlane((int)incl, 63), excl = incl - both;
                            const int totN = (int)(total & 0xFFFFu), totL = (int)(total >> 16);
                            if (nN + totN + nL + totL > MESH_Q) {
                                overflow = true;
                            } else {
                                if (totN > 0) {  // surviving inner children -> node LIFO
                                    const unsigned first_inner = __float_as_uint(h1.x);
                                    int w = nN + (int)(excl & 0xFFFFu);
                                    while (__builtin_amdgcn_ballot_w64(mi != 0u) != 0ull) {
                                        if (mi != 0u) {
                                            const unsigned below = (mi & (0u - mi)) - 1u;
                                            qn[w++] = tag | (first_inner + (unsigned)__builtin_popcount(innermask & below));
                                            mi &= mi - 1u;
                                        }
                                    }
                                    nN += totN;
                                }
                                if (totL > 0) {  // surviving leaf children -> leaf queue, item = (first triangle) * 4 + (count - 1)
                                    const unsigned first_tri = __float_as_uint(h1.y);
                                    int w = nL + (int)(excl >> 16);
                                    while (__builtin_amdgcn_ballot_w64(ml != 0u) != 0ull) {
                                        if (ml != 0u) {
                                            const unsigned bit = ml & (0u - ml), below = bit - 1u;
                                            const unsigned below2 = bit * bit - 1u;
                                            const unsigned cf = counts & below2;
                                            const unsigned first = first_tri + (unsigned)__builtin_popcount(leafmask & below) + (unsigned)__builtin_popcount(cf & 0x5555u) +
                                                                   2u * (unsigned)__builtin_popcount(cf & 0xAAAAu);
                                            const unsigned c2 = 2u * (unsigned)__builtin_ctz(bit);
                                            qlt[-(w++)] = tag | (first * 4u + ((counts >> c2) & 3u));
                                            ml &= ml - 1u;
                                        }
                                    }
                                    nL += totL;
                                }
                            }
                        } else {
                            const int logL = nL <= 16 ? 2 : nL <= 32 ? 1 : 0;
                            const int takeL = nL < (64 >> logL) ? nL : (64 >> logL);
                            const int trips = 4 >> logL;
                            nL -= takeL;  // the items [nL, nL + takeL) are popped
                            const int slotL = lane >> logL, subL = lane & ((1 << logL) - 1);
                            const bool popped = slotL < takeL;
                            const unsigned item = popped ? qlt[-(nL + slotL)] : 0u;
                            const int src = (int)(item >> 26), code = (int)(item & 0x3FFFFFFu);
                            const int lcnt = (code & 3) + 1;
                            const float4* rowp = P.bvh_tris + 3 * (size_t)((code >> 2) + (subL < lcnt ? subL : 0));  // (idle lanes: triangle 0)
                            float4 a = rowp[0], b = rowp[1], c = rowp[2];
                            const V3 ro = v3(__shfl(o.x, src), __shfl(o.y, src), __shfl(o.z, src));
                            const V3 rd = v3(__shfl(d.x, src), __shfl(d.y, src), __shfl(d.z, src));
                            const float tm = __shfl(best, src);
                            const bool onL = popped && hitbit[src] == 0u;  // an occluded ray's items are dropped
                            for (int j = 0;; ++j) {
                                const int k = subL + (j << logL);  // this trip's triangle of the leaf
                                const bool more = j + 1 < trips;   // (wave-uniform)
                                float4 na = a, nb = b, nc = c;
                                if (more) {
                                    const int kn = subL + ((j + 1) << logL);
                                    const float4* np = P.bvh_tris + 3 * (size_t)((code >> 2) + (kn < lcnt ? kn : 0));
                                    na = np[0], nb = np[1], nc = np[2];
                                }
                                W.add(OCC_WORK_TRIANGLES, __builtin_amdgcn_ballot_w64(onL && k < lcnt));
                                // Moller-Trumbore, binary32, no FMA, fixed order (the oracle's triangle_raytrace), as closest_hit
                                V3 pv = v3(rd.y * c.z - rd.z * c.y, rd.z * c.x - rd.x * c.z, rd.x * c.y - rd.y * c.x);
                                float det = (b.x * pv.x + b.y * pv.y) + b.z * pv.z;
                                float idet = 1.0f / det;
                                V3 tv = v3(ro.x - a.x, ro.y - a.y, ro.z - a.z);
                                float u = ((tv.x * pv.x + tv.y * pv.y) + tv.z * pv.z) * idet;
                                V3 qv = v3(tv.y * b.z - tv.z * b.y, tv.z * b.x - tv.x * b.z, tv.x * b.y - tv.y * b.x);
                                float vv = ((rd.x * qv.x + rd.y * qv.y) + rd.z * qv.z) * idet;
                                float t = ((c.x * qv.x + c.y * qv.y) + c.z * qv.z) * idet;
                                const bool ok = onL & (k < lcnt) & (fabsf(det) >= 1e-12f) & (u >= 0.0f) & (u <= 1.0f) & (vv >= 0.0f) & (u + vv <= 1.0f) &
                                                (t >= (float)0.01) & (t <= 10000.0f) & (t < tm);
                                if (ok) hitbit[src] = 1u;  // every writer stores the same word: idempotent, redoing a batch changes nothing
                                if (!more) break;
                                a = na, b = nb, c = nc;
                            }
                        }
                        __builtin_amdgcn_wave_barrier();
                    }
                    if (!overflow) {
                        pend &= ~selmask;
                    } else if (batch > 1) {
                        batch = batch > 4 ? batch >> 2 : 1;
                    } else {
                        strict = true;  // cannot overflow: the host bounds 7 * depth + 80 (the stack + the leaves that may wait) by MESH_Q
                    }
                    pend &= ~__builtin_amdgcn_ballot_w64(hitbit[lane] != 0u);  // (an abandoned batch may have found some of its rays occluded)
                }
                occ = occ | (go && hitbit[lane] != 0u);
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    return occ;
}

// LDS: the path-trace kernel's layout (make_lds with four waves), as rays_kernel.
template <bool SCENE_LDS, bool MESH, bool COUNT>
__global__ void __launch_bounds__(WG_THREADS) occlusion_kernel(const KernelParams P, const OcclusionIO io) {
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
    OccWork<COUNT> W;
    const uint32_t blocks = (io.count + 63u) >> 6;  // count <= 2^30: at most 2^24 blocks
    const bool norm = io.normalize != 0u;           // (a kernel argument: wave-uniform)
    // wave-uniform loop: every lane of a wave runs the same trips, so any_hit sees all 64 lanes in each call
    for (uint32_t b = blockIdx.x * (uint32_t)WAVES + (uint32_t)wave; b < blocks; b += gridDim.x * (uint32_t)WAVES) {
        const uint32_t i = (b << 6) + (uint32_t)lane;
        const bool active = i < io.count;
        // lanes past the batch load nothing: they carry a closed segment through the wave's rounds and store nothing
        float4 o4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), d4 = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
        if (active) o4 = io.origin[i], d4 = io.direction[i];  // 16-byte loads
        V3 dir = v3(d4.x, d4.y, d4.z);
        if (norm) dir = normalized(dir);  // float3::Normalized (Common.hpp:159-162); its window test is wave-level: called by all lanes
        const bool occ = any_hit<MESH, COUNT, SCENE_LDS>(S, P, v3(o4.x, o4.y, o4.z), dir, d4.w, active, W);
        W.add(OCC_WORK_RAYS, __builtin_amdgcn_ballot_w64(active));
        W.add(OCC_WORK_OCCLUDED, __builtin_amdgcn_ballot_w64(active && occ));
        if (active) io.occluded[i] = occ ? 1 : 0;
    }
    if constexpr (COUNT) {  // the wave's sums: lane k adds counter k — one vector atomic per wave
        unsigned long long v = 0ull;
#pragma unroll
        for (int k = 0; k < OCC_WORK_N; ++k) v = lane == k ? W.n[k] : v;
        if (lane < OCC_WORK_N) atomicAdd(&io.work[lane], v);
    }
}

}  // namespace srt
