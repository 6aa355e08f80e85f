// srt_probe_tail.hip.h — gfx950 probe tail (srt_probe_tail): a path of radiance_kernel or light_probe_kernel that ends because
// the bounce limit was reached on a surface adds the probe grid's hemisphere-mean radiance at that surface, times its throughput
// (rules T1 – T6 of srt_pathtrace.h).  ONE lookup, probe_tail_lookup, called from both path-end sites: run_sample_pool
// (srt_sample_pool.hip.h) and light_probe_kernel's own text.  It is a composition of the probe-grid shading rules and calls their
// per-corner pieces (probe_grid_cell, probe_depth_weigh, probe_grid_irradiance of srt_probe_grid.hip.h): for the hit's point x
// and normal n it computes what probe_grid_shade writes for a pixel with those guides — rules 2 – 6, 7b, 3s / 4s, 8 and 9 in the
// same operation order, corners summed in ascending c from +0, a skipped corner contributing +0.
//
// LANE-SERIAL: the loop c = 0 .. 7 runs in wave-uniform control flow while any lane of the step terminates, and each terminating
// lane does its own eight corners — one record load under STATES, one 16-byte moment load under DEPTH, nine 16-byte coefficient
// loads.  The summation order falls out of this form and it needs no LDS (the pool's records are live during the pool).  With
// max_bounces == 1 every busy lane terminates in the same step, so the wave is full.  Only the caller's L, T, x, n, g and task
// word are live across it.  The loop stays rolled: one corner's nine loads are in flight at a time, not seventy-two.
// Every coefficient, record and moment index is built from cell indices clamped to [0, n_a - 1] per axis, as in the shading body:
// no load can leave the arrays whatever the path state holds.
// The three rule switches (NORMAL_WEIGHT, DEPTH, STATES) are kernel arguments, wave-uniform, not template parameters.
// Work counts: wave-uniform 64-bit sums kept by every TAIL instantiation (they are scalar), flushed with ONE vector atomic per wave
// at the end and only when the launch was given a record.  No atomic reaches an output.
#pragma once

#include "srt_probe_grid.hip.h"

namespace srt {

enum { PT_WORK_TAILS = 0, PT_WORK_CORNERS, PT_WORK_OPEN, PT_WORK_DARK, PT_WORK_MIRROR_ENDS, PT_WORK_WAVE_LOOKUPS, PT_WORK_N };

constexpr uint32_t PT_NORMAL_WEIGHT = 1u, PT_DEPTH = 2u, PT_STATES = 4u;  // SRT_PROBE_TAIL_*: the bits of ProbeTailIO::flags

// the tail's inputs: a kernel argument of its own, passed only to the TAIL instantiations
struct ProbeTailIO {
    const float4* coefficients;  // [nx * ny * nz][9]
    const float4* depth;         // PT_DEPTH: [nx * ny * nz][R*R]
    const float4* states;        // PT_STATES: [nx * ny * nz] (o.xyz, state bits)
    float origin[3], spacing[3];
    int32_t counts[3];
    float band_weight[3];
    uint32_t flags;              // PT_*
    uint32_t resolution;         // PT_DEPTH: R: 4, 8 or 16
    float bias, min_variance;    // PT_DEPTH
    unsigned long long* work;    // [PT_WORK_N] totals of the launch (zeroed by the host before it); NULL: not requested
};

// what a TAIL instantiation carries for the tail, inside its work counts (TailWaveWork, LpTailWork): the kernel argument and the sums
struct ProbeTail {
    const ProbeTailIO* io = nullptr;
    unsigned long long n[PT_WORK_N] = {};
    __device__ __forceinline__ void flush(int lane) const {  // lane k adds counter k — one vector atomic per wave
        if (!io->work) return;
        unsigned long long v = 0ull;
#pragma unroll
        for (int k = 0; k < PT_WORK_N; ++k) v = lane == k ? n[k] : v;
        if (lane < PT_WORK_N) atomicAdd(&io->work[lane], v);
    }
};

// Rules T3 – T5 for the lanes with `term` (the path ended at the bounce limit on the surface at x with normal n; T is the
// throughput after that hit's colour, g = 1 - Smoothness * spec).  True for a lane that adds; `add` is then k * M per colour
// lane.  Every lane of the wave calls it; nothing happens unless a lane terminates.
__device__ __forceinline__ bool probe_tail_lookup(ProbeTail& tail, bool term, V3 x, V3 n, RGB T, float g, RGB& add) {
    if (__builtin_amdgcn_ballot_w64(term) == 0ull) return false;
    const ProbeTailIO& io = *tail.io;
    auto lanes = [](bool b) { return (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(b)); };
    const bool look = term && g > 0.0f;  // T3 (a NaN fails)
    tail.n[PT_WORK_WAVE_LOOKUPS] += 1ull;
    tail.n[PT_WORK_TAILS] += lanes(look);
    tail.n[PT_WORK_MIRROR_ENDS] += lanes(term && !look);
    const bool weigh = (io.flags & PT_NORMAL_WEIGHT) != 0u, moments = (io.flags & PT_DEPTH) != 0u, records = (io.flags & PT_STATES) != 0u;  // (wave-uniform)
    const int nx = io.counts[0], ny = io.counts[1], nz = io.counts[2];
    const int R = (int)io.resolution;
    // rule 2: the cell; rule 5's origin
    int i0, i1, i2;
    float f0, f1, f2;
    probe_grid_cell(x.x, io.origin[0], io.spacing[0], nx, i0, f0);
    probe_grid_cell(x.y, io.origin[1], io.spacing[1], ny, i1, f1);
    probe_grid_cell(x.z, io.origin[2], io.spacing[2], nz, i2, f2);
    const float ofs = .00001f;
    const V3 o = v3(x.x + n.x * ofs, x.y + n.y * ofs, x.z + n.z * ofs);  // :177
    float E0 = 0.0f, E1 = 0.0f, E2 = 0.0f, A = 0.0f;
#pragma unroll 1
    for (int c = 0; c < 8; ++c) {  // (wave-uniform)
        const int cx = c & 1, cy = (c >> 1) & 1, cz = (c >> 2) & 1;
        // rule 3: the trilinear weight
        const float w0 = cx ? f0 : (1.0f - f0), w1 = cy ? f1 : (1.0f - f1), w2 = cz ? f2 : (1.0f - f2);
        float tw = (w0 * w1) * w2;
        bool live = look && tw > 0.0f;  // (a NaN fails)
        // the corner's probe, clamped per axis: in [0, n_a - 1] whatever the path state holds
        const int k0 = min(max(i0 + cx, 0), nx - 1), k1 = min(max(i1 + cy, 0), ny - 1), k2 = min(max(i2 + cz, 0), nz - 1);
        const size_t probe = (size_t)k0 + (size_t)nx * ((size_t)k1 + (size_t)ny * (size_t)k2);
        // rule 4: the probe; rule 5: the segment to it
        V3 p = v3(io.origin[0] + (float)(i0 + cx) * io.spacing[0], io.origin[1] + (float)(i1 + cy) * io.spacing[1],
                  io.origin[2] + (float)(i2 + cz) * io.spacing[2]);
        if (records) {  // rule 3s: a buried probe is skipped and enters no counter; rule 4s: the others stand where they were moved to
            float4 st = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (live) st = io.states[probe];  // 16-byte load
            live = live && !(__float_as_uint(st.w) & PG_STATE_BURIED);
            p = v3(p.x + st.x, p.y + st.y, p.z + st.z);
        }
        const V3 v = v3(p.x - o.x, p.y - o.y, p.z - o.z);
        const float q = (v.x * v.x + v.y * v.y) + v.z * v.z;
        const float L = sqrtf(q);
        live = live && L > 0.0f;
        const V3 d = v3(v.x / L, v.y / L, v.z / L);
        if (weigh) {  // rule 6
            const float hh = (((d.x * n.x + d.y * n.y) + d.z * n.z) + 1.0f) * 0.5f;
            tw = tw * ((hh * hh) + 0.2f);
        }
        bool ok = live;
        if (moments) {  // rule 7b
            ok = false;
            if (live) {
                tw = probe_depth_weigh(io.depth + probe * (size_t)(R * R), R, d, L, io.bias, io.min_variance, tw);
                ok = tw > 0.0f;
            }
        }
        tail.n[PT_WORK_CORNERS] += lanes(live);
        tail.n[PT_WORK_OPEN] += lanes(ok);
        // rule 8: the corner's irradiance at the normal; rule 9: ascending c, a skipped corner contributes +0
        float4 res = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (ok) {
            const V3 e = probe_grid_irradiance(io.coefficients + probe * (size_t)PG_COEFFS, n, io.band_weight);
            res = make_float4(tw * e.x, tw * e.y, tw * e.z, tw);
        }
        E0 = E0 + res.x, E1 = E1 + res.y, E2 = E2 + res.z, A = A + res.w;
    }
    // T4: (M, a) = (E / A, A); nothing is added unless a > 0; SH ringing and NaN stay out of the mean
    const bool adds = look && A > 0.0f;
    tail.n[PT_WORK_DARK] += lanes(look && !adds);
    float M0 = E0 / A, M1 = E1 / A, M2 = E2 / A;
    M0 = !(M0 > 0.0f) ? 0.0f : M0, M1 = !(M1 > 0.0f) ? 0.0f : M1, M2 = !(M2 > 0.0f) ? 0.0f : M2;
    // T5: the dissipation the next bounce would have applied (:169-171), and the share of its direction that would have been random
    add = RGB{((T.r * 0.8f) * g) * M0, ((T.g * 0.8f) * g) * M1, ((T.b * 0.8f) * g) * M2};
    return adds;
}

}  // namespace srt
