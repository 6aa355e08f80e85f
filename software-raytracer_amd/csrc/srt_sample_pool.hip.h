// srt_sample_pool.hip.h — the wave-level sample pool of radiance_kernel and adaptive_kernel: 64 slots that share nothing but a
// first hit each, and (slot, sample) tasks dealt to whichever lanes are free.  (light_probe_kernel runs the same pool from a
// text of its own: DESIGN.md §4.32 says why.)
//
// A kernel takes ONE closest_hit for the 64 primary rays of its unit (a block of rays, a pixel tile):
// there is no jitter, every sample of a slot shares its first hit.  A lane whose colour does not depend on the sample (a miss,
// or max_bounces == 0) folds that colour itself (fold_constant_colour).  The other lanes leave a record in slot `lane` of the
// wave's LDS records (write_first_hit_record) and the wave calls run_sample_pool:
//   1. Every step the free lanes take tasks from the slots that have samples left — the slots are dealt to the free lanes
//      round-robin, so a slot hands out as many consecutive samples in one step as it is dealt lanes (one slot x 64 samples fills
//      the wave) — and all 64 lanes go through one closest_hit; idle lanes ride along through its wave-uniform rounds.  One
//      bounce is restated here from pathtrace_kernel (which stays as it is), expression by expression: the same bits.
//   2. A finished sample's colour (r, g, b, alpha tag) goes to row (sample - chunk start), slot, of the wave's OWN region of a
//      scratch buffer in global memory: RAD_CHUNK rows of 64 float4.  When the pool has drained, the owner lanes fold their
//      slot's rows in sample order — the ROWS kernel's scheme with its workgroup-scope release / acquire pair in front of the
//      read-back.  More than RAD_CHUNK samples run chunk after chunk on the same wave, folding in between; the running mean
//      stays in the owner's registers.  The scratch is sized by the grid (waves x RAD_CHUNK x 64 x 16 B), never by the work.
// The fold order per slot is fixed (ascending sample) whatever the packing does, and no atomic reaches an output.
//
// What a kernel brings is its sample source, a small type:
//   last()             the wave-uniform end of the chunk loop (called once, by all lanes)
//   chunk(c0)          the slot's part of the chunk at c0: first(), end (samples [first, end) are handed out), owner() (the lane
//                      folds), count() (rows to fold, row 0 first)
//   frame(r, sidx)     the frame of sample sidx of the slot whose record is r: the last round of srt_rng_key
//   fold(acc, c, a, s) sample s of the lane's own slot into its running mean
//   CLOSEST, WAVE_CALLS  the indices of the two work counts the pool adds to
// LaunchSamples (below) is radiance_kernel's: every traced slot runs the launch's samples, so the chunk bounds are wave-uniform
// scalars.  adaptive_kernel's PixelSamples (srt_adaptive.hip.h) has them per lane.  With lim = traced ? n : 0 the per-lane form
// computes the uniform form's values; it is kept apart for the vector registers it costs.
#pragma once

#include "srt_kernel.hip.h"
#include "srt_probe_tail.hip.h"
#include "srt_sun_sampling.hip.h"

namespace srt {

// samples per chunk: rows of the wave's scratch region (srt_radiance_host.h: RADIANCE_CHUNK; srt_capi.hip asserts that they agree)
constexpr int RAD_CHUNK = 64;

// The scene image into LDS, staged as pathtrace_kernel stages it (see there): every load issued before the first LDS store.
// Every thread of the workgroup calls it; the image is there when it returns.
template <bool SCENE_LDS>
__device__ __forceinline__ void stage_scene(const KernelParams& P, float4* lds_scene) {
    if constexpr (SCENE_LDS) {
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
}

// per-wave work counts: N wave-uniform 64-bit sums, added to a handle-owned record with ONE vector atomic per wave at the end
// (lane k adds counter k).  Without ON there is no atomic.
template <bool ON, int N>
struct WaveWork {
    static constexpr bool TAIL = false, SUN = false;
    __device__ __forceinline__ void add(int, unsigned long long) {}
    __device__ __forceinline__ void flush(unsigned long long*, int) const {}
};
template <int N>
struct WaveWork<true, N> {
    static constexpr bool TAIL = false, SUN = false;
    unsigned long long n[N] = {};
    __device__ __forceinline__ void add(int i, unsigned long long v) { n[i] += v; }
    __device__ __forceinline__ void flush(unsigned long long* work, int lane) const {
        unsigned long long v = 0ull;
#pragma unroll
        for (int k = 0; k < N; ++k) v = lane == k ? n[k] : v;
        if (lane < N) atomicAdd(&work[lane], v);
    }
};
// the work counts of a TAIL instantiation (srt_probe_tail.hip.h): run_sample_pool ends a path that reaches the bounce limit on a
// surface in the probe grid when its Work says TAIL, and finds the tail's kernel argument and sums here.  Both records' sums are
// always kept (they are scalar) and flushed when the launch has the record.
template <int N>
struct TailWaveWork : WaveWork<true, N> {
    static constexpr bool TAIL = true;
    ProbeTail tail;
    __device__ __forceinline__ void flush(unsigned long long* work, int lane) const {
        if (work) WaveWork<true, N>::flush(work, lane);
        tail.flush(lane);
    }
};

// the work counts of a SUN instantiation (srt_sun_sampling.hip.h): run_sample_pool samples the sun at every diffuse vertex when its
// Work says SUN, and finds the frame here.  The sums are always kept and flushed when the launch has the record.
template <int N>
struct SunWaveWork : WaveWork<true, N> {
    static constexpr bool SUN = true;
    const SunIO* sun = nullptr;
    __device__ __forceinline__ void flush(unsigned long long* work, int lane) const {
        if (work) WaveWork<true, N>::flush(work, lane);
    }
};

// the work counts of an instantiation with both (srt_render_adaptive_tail with SRT_ADAPTIVE_SUN_SAMPLING, rule AS4): the tail's
// kernel argument and sums, and the frame
template <int N>
struct TailSunWaveWork : TailWaveWork<N> {
    static constexpr bool SUN = true;
    const SunIO* sun = nullptr;
};

// the number of lanes for which b holds / of set bits of m below this lane
__device__ __forceinline__ unsigned long long wave_lanes(bool b) { return (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(b)); }
__device__ __forceinline__ int lanes_below(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}
// this wave's region of the scratch: RAD_CHUNK rows of 64 slots
__device__ __forceinline__ float4* wave_sample_rows(float4* rows, int wave) {
    return rows + ((size_t)blockIdx.x * (WG_TILES_X * WG_TILES_Y) + (size_t)wave) * (size_t)(RAD_CHUNK * 64);
}

// the samples of radiance_kernel: [0, P.sample_count) for every traced slot, frame P.first_sample + sample
template <int CLOSEST_, int WAVE_CALLS_>
struct LaunchSamples {
    static constexpr int CLOSEST = CLOSEST_, WAVE_CALLS = WAVE_CALLS_;
    const KernelParams& P;
    bool traced;
    struct Chunk {
        uint32_t c0, end;  // (wave-uniform)
        bool traced;
        __device__ __forceinline__ uint32_t first() const { return traced ? c0 : end; }
        __device__ __forceinline__ bool owner() const { return traced; }
        __device__ __forceinline__ uint32_t count() const { return end - c0; }
    };
    __device__ __forceinline__ uint32_t last() const { return P.sample_count; }
    __device__ __forceinline__ Chunk chunk(uint32_t c0) const {
        const uint32_t n = P.sample_count;
        return Chunk{c0, n - c0 < (uint32_t)RAD_CHUNK ? n : c0 + (uint32_t)RAD_CHUNK, traced};
    }
    __device__ __forceinline__ uint32_t frame(const float*, uint32_t sidx) const { return P.first_sample + sidx; }
    __device__ __forceinline__ void fold(float4& acc, RGB c, float a, uint32_t s) const { accumulate_sample(P, acc, c, a, s); }
};

// ---- the lanes whose colour does not depend on the sample: a miss -> env(d) every sample (Raytracer.cpp:143-145);
// MAXBOUNCES == 0 -> the first hit's EmissiveColor (:162, 212).  Folded `count` times.
template <class Src>
__device__ __forceinline__ void fold_constant_colour(const Lds& S, const Src& src, V3 dir0, const Hit& h0, uint32_t count, float4& acc) {
    RGB c;
    float ca = 0.0f;  // the colour's alpha (+0 from the emissive colour)
    if (h0.prim < 0) {
        c = environment(S, dir0);
        ca = environment_alpha(dir0);
    } else {
        const float4 m1 = S.mat(h0.prim, 1);
        c = RGB{clamp0(m1.y), clamp0(m1.z), clamp0(m1.w)};
    }
    for (uint32_t s = 0; s < count; ++s) src.fold(acc, c, ca, s);
}

// ---- slot `lane` of the wave's records, [64][12] floats in S.pix: dir, n0, p0, prim0, the seed-and-id half of the RNG key
// (word 11 is the sample source's)
__device__ __forceinline__ void write_first_hit_record(const Lds& S, int lane, V3 dir0, const Hit& h0, uint32_t seed, uint32_t id) {
    float* r = S.pix + lane * 12;
    r[0] = dir0.x, r[1] = dir0.y, r[2] = dir0.z;
    r[3] = h0.n.x, r[4] = h0.n.y, r[5] = h0.n.z;
    r[6] = h0.p.x, r[7] = h0.p.y, r[8] = h0.p.z;
    r[9] = __int_as_float(h0.prim);
    // srt_rng_key's first two rounds depend on seed and id only: done here once, the sample's round at the hand-out
    r[10] = __uint_as_float(srt_mix32(srt_mix32(seed ^ 0xA511E9B3U) + id));
}

// path state of the task a lane is running (whether it runs one is a flag of its own, `busy`: a lane mask, not a register)
struct PoolLane {
    uint32_t task = 0;  // sample << 6 | slot
    RGB L{0, 0, 0}, T{0, 0, 0};
    V3 sray = v3(0, 0, 1), hn = v3(0, 0, 0), hp = v3(0, 0, 0);
    int hprim = 0, bounce = 0;
    float spec = 0.0f;
    uint32_t rng = 0;
};

// ---- hand out tasks: the slots that have samples left are dealt round-robin to the free lanes, and a slot hands out as many
// consecutive samples as it is dealt lanes, up to what it has left (pathtrace_kernel's MULTI hand-out).  Two passes: entries that
// stayed empty in the first because a slot ran out find another slot in the second.  `match`: [64] of (sample << 6 | slot),
// ~0 = nothing; `rot`: the wave-uniform rotation of the slot priority; samples [.., own_next) of this lane's slot have been handed
// out, `end` is where they stop.  True for a lane that has just taken a task.
__device__ __forceinline__ bool pool_hand_out(unsigned* match, int lane, int& rot, uint32_t& own_next, uint32_t end, bool busy, uint32_t& task) {
    bool fresh = false;
#pragma unroll 1  // (unrolled, the two passes cost vector registers: DESIGN.md §4.32)
    for (int pass = 0; pass < 2; ++pass) {
        const unsigned long long freem = __builtin_amdgcn_ballot_w64(!busy);
        const int avail = own_next < end ? (int)(end - own_next) : 0;
        const bool can = avail > 0;
        const unsigned long long canm = __builtin_amdgcn_ballot_w64(can);
        if (freem == 0ull || canm == 0ull) break;
        const int nfree = __builtin_popcountll(freem), ncan = __builtin_popcountll(canm);
        // the slot priority rotates so that all slots advance at the same pace: rank among the slots that can,
        // counted cyclically from lane `rot`
        rot = (rot + 23) & 63;
        const int crank = lanes_below(canm) - __builtin_popcountll(canm & ((1ull << rot) - 1ull)) + (lane < rot ? ncan : 0);
        const int frank = lanes_below(freem);
        if (!busy) match[frank] = 0xFFFFFFFFu;
        __builtin_amdgcn_wave_barrier();
        if (can) {
            int given = 0;
            for (int j = crank; j < nfree && given < avail; j += ncan) {
                match[j] = ((own_next + (uint32_t)given) << 6) | (unsigned)lane;
                ++given;
            }
            own_next += (uint32_t)given;
        }
        __builtin_amdgcn_wave_barrier();
        const unsigned m = !busy ? match[frank] : 0xFFFFFFFFu;
        if (m != 0xFFFFFFFFu) {  // (the sample is set up by the caller, once for the lanes of both passes)
            task = m;
            busy = true;
            fresh = true;
        }
        __builtin_amdgcn_wave_barrier();
    }
    return fresh;
}

// ---- a lane that has just taken a task: Raytracer.cpp:162-166 for sample sidx of that slot
template <class Src>
__device__ __forceinline__ void pool_start_sample(const Lds& S, const Src& src, PoolLane& t) {
    const uint32_t sidx = t.task >> 6;
    const float* r = S.pix + (int)(t.task & 63u) * 12;
    const int prim0 = __float_as_int(r[9]);
    t.rng = srt_mix32(__float_as_uint(r[10]) + src.frame(r, sidx));  // = srt_rng_key(seed, id, frame), see the record
    const uint32_t rr = srt_mix32(t.rng) >> 17;                      // draw 0: the specular lottery at the first hit
    t.rng += 0x9E3779B9U;
    const float4 m0 = S.mat(prim0, 0), m1 = S.mat(prim0, 1);
    t.spec = (m0.y >= rand_unit(rr)) ? 1.0f : 0.0f;  // :165
    t.L = RGB{m1.y, m1.z, m1.w};                     // :162 (clamped in the image)
    t.T = RGB{m0.z, m0.w, m1.x};                     // :163
    t.sray = v3(r[0], r[1], r[2]);                   // :164
    t.hn = v3(r[3], r[4], r[5]);
    t.hp = v3(r[6], r[7], r[8]);
    t.hprim = prim0;
    t.bounce = 0;
}

// ---- one bounce for a busy lane (Raytracer.cpp:169-177): the new direction in t.sray, the ray's origin returned
__device__ __forceinline__ V3 pool_bounce(const Lds& S, bool busy, PoolLane& t) {
    V3 o = v3(0, 0, 0);
    const float ofs = .00001f;
    if (busy) {
        if (t.bounce != 0) {  // :169-171
            t.T = RGB{t.T.r * 0.8f, t.T.g * 0.8f, t.T.b * 0.8f};  // (NN)
        }
        // reflectedRay = sray.Reflect(normal)  (:172, Common.hpp:163-165)
        const float k2 = 2 * dot3(t.sray, t.hn);
        const V3 refl = v3(t.sray.x - t.hn.x * k2, t.sray.y - t.hn.y * k2, t.sray.z - t.hn.z * k2);
        // GetRandomNormalOrientedHemisphere (:90-105): exactly three draws, x then y then z
        const uint32_t r0 = srt_mix32(t.rng) >> 17;
        const uint32_t r1 = srt_mix32(t.rng + 0x9E3779B9U) >> 17;
        const uint32_t r2 = srt_mix32(t.rng + 2u * 0x9E3779B9U) >> 17;
        t.rng += 3u * 0x9E3779B9U;
        V3 sr = v3((rand_unit(r0) - 0.5f) * 2, (rand_unit(r1) - 0.5f) * 2, (rand_unit(r2) - 0.5f) * 2);
        sr = normalized_in_window(sr);  // (inside normalized()'s window by construction: see there)
        if (dot3(sr, t.hn) < 0) sr = v3(sr.x * -1, sr.y * -1, sr.z * -1);
        // float3::Lerp(sray, reflectedRay, Smoothness * specularProb)  (:175)
        const float tt = S.mat(t.hprim, 0).x * t.spec;
        const V3 l = v3(sr.x * (1 - tt) + refl.x * tt, sr.y * (1 - tt) + refl.y * tt, sr.z * (1 - tt) + refl.z * tt);
        t.sray = normalized(l);                                                    // :176
        o = v3(t.hp.x + t.hn.x * ofs, t.hp.y + t.hn.y * ofs, t.hp.z + t.hn.z * ofs);  // :177
    }
    return o;
}

// ---- what the bounce's ray met (Raytracer.cpp:178-184), for a busy lane.  True when the path has ended; `atag` is then the
// sample's alpha: NaN only from the environment (T's alpha is +0).  E0: a lane with `no_sun` — its bounce was blind and the sun has
// been sampled for it (rule S7) — meets the environment without the sun.
template <bool E0 = false>
__device__ __forceinline__ bool pool_hit_update(const Lds& S, const Hit& h, int B, PoolLane& t, uint32_t& atag, [[maybe_unused]] bool no_sun = false) {
    bool end_path;
    if (h.prim < 0) {  // :178-181
        const RGB e = environment<E0>(S, t.sray, no_sun);
        t.L = RGB{t.L.r + e.r * t.T.r, t.L.g + e.g * t.T.g, t.L.b + e.b * t.T.b};  // (NN)
        atag = alpha_tag(environment_alpha(t.sray));
        end_path = true;
    } else {
        const float4 m0 = S.mat(h.prim, 0), m1 = S.mat(h.prim, 1), m2 = S.mat(h.prim, 2);
        const uint32_t r = srt_mix32(t.rng) >> 17;  // one lottery per further hit
        t.rng += 0x9E3779B9U;
        t.spec = (m0.y >= rand_unit(r)) ? 1.0f : 0.0f;  // :182
        const RGB Em{m1.y, m1.z, m1.w};
        t.L = RGB{t.L.r + Em.r * t.T.r, t.L.g + Em.g * t.T.g, t.L.b + Em.b * t.T.b};  // :183 (NN)
        const RGB Bc{m0.z, m0.w, m1.x}, Sc{m2.x, m2.y, m2.z};
        const float ns = 1 - t.spec;  // :184, Color::Lerp with t = 0 or 1 (NN)
        const RGB f{Bc.r * ns + Sc.r * t.spec, Bc.g * ns + Sc.g * t.spec, Bc.b * ns + Sc.b * t.spec};
        t.T = RGB{t.T.r * f.r, t.T.g * f.g, t.T.b * f.b};
        t.hn = h.n;
        t.hp = h.p;
        t.hprim = h.prim;
        ++t.bounce;
        end_path = t.bounce >= B;
    }
    return end_path;
}

// ---- the finished sample's colour into row (sample - c0), slot, of the wave's region; written exactly once (the sample is in
// [c0, c0 + RAD_CHUNK): handed out by this chunk)
__device__ __forceinline__ void pool_store_row(float4* rows, uint32_t c0, uint32_t atag, const PoolLane& t) {
    const uint32_t sidx = t.task >> 6;
    rows[((sidx - c0) << 6) + (t.task & 63u)] = make_float4(t.L.r, t.L.g, t.L.b, __uint_as_float(sidx | atag));
}

// ---- lane l folds rows 0 .. cnt - 1 of slot l, in sample order, ROWS_IN_FLIGHT loads in flight; row 0 is sample s0 of the slot
template <class Src>
__device__ __forceinline__ void pool_fold_rows(const Src& src, const float4* row, uint32_t s0, uint32_t cnt, float4& acc) {
    uint32_t s = 0;
    for (; s + ROWS_IN_FLIGHT <= cnt; s += ROWS_IN_FLIGHT) {
        float4 c[ROWS_IN_FLIGHT];
#pragma unroll
        for (int k = 0; k < ROWS_IN_FLIGHT; ++k) c[k] = row[(size_t)(s + k) * 64];
#pragma unroll
        for (int k = 0; k < ROWS_IN_FLIGHT; ++k) src.fold(acc, RGB{c[k].x, c[k].y, c[k].z}, tag_alpha(__float_as_uint(c[k].w)), s0 + s + k);
    }
    for (; s < cnt; ++s) {
        const float4 c = row[(size_t)s * 64];
        src.fold(acc, RGB{c.x, c.y, c.z}, tag_alpha(__float_as_uint(c.w)), s0 + s);
    }
}

// ---- the pool over (slot, sample): lane l owns slot l, whose record the caller has written (and passed a wave barrier since);
// `rows` is the wave's region of the scratch, `acc` the owner's running mean.  Every lane of the wave calls it.
// A Work with TAIL (TailWaveWork) ends a path that reaches the bounce limit on a surface in the probe grid (srt_probe_tail.hip.h);
// the tail travels inside the Work, not as a parameter, so that the other instantiations compile to what they did.
// A Work with SUN (SunWaveWork) samples the sun at every diffuse vertex (srt_sun_sampling.hip.h), by the same scheme.
// A Work with both (TailSunWaveWork) does both: the segment stands before the bounce's closest_hit and the lookup behind it, so the
// two never share a moment — any_hit's words in S.res and S.meshq are dead again when the lookup, which uses no LDS, runs.
template <bool MESH, bool SCENE_LDS, class Src, class Work>
__device__ __forceinline__ void run_sample_pool(const Lds& S, const KernelParams& P, const Src& src, float4* rows, int lane, float4& acc, Work& W SRT_PROF_PARAM) {
    unsigned* const match = reinterpret_cast<unsigned*>(S.work);
    const int B = P.max_bounces;
    Tally<false> no_tally;
    bool deferred = false;  // (defer_min = 1: every call resolves its mesh rays itself)
    bool busy = false;
    PoolLane t;
    int rot = 0;
    const uint32_t last = src.last();
    for (uint32_t c0 = 0; c0 < last; c0 += (uint32_t)RAD_CHUNK) {  // (wave-uniform)
        const auto ch = src.chunk(c0);
        uint32_t own_next = ch.first();
        // the fold of the chunk before has read the rows this chunk's paths overwrite
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        while (__builtin_amdgcn_ballot_w64(busy || own_next < ch.end) != 0ull) {
            const bool fresh = pool_hand_out(match, lane, rot, own_next, ch.end, busy, t.task);
            busy = busy || fresh;
            if (fresh) pool_start_sample(S, src, t);
            W.add(Src::CLOSEST, wave_lanes(fresh));  // the sample's primary GetClosestObject call (:142)
            const V3 o = pool_bounce(S, busy, t);
            [[maybe_unused]] bool diffuse = false;  // SUN: this lane's bounce was blind (rule S2); kept across closest_hit for S7
            if constexpr (Work::SUN) {  // rules S3 - S6 in wave-uniform control flow, before the bounce's own result is added
                diffuse = busy && (S.mat(t.hprim, 0).x * t.spec) == 0.0f;  // tt of :175, as pool_bounce computed it
                W.add(Src::WAVE_CALLS, sun_sample<MESH, SCENE_LDS>(S, P, *W.sun, diffuse, t.rng, o, t.hn, t.T, t.L));
            }
            // the scan runs in wave-uniform control flow: idle lanes help with other lanes' rays
            const Hit h = closest_hit<MESH, false, SCENE_LDS>(S, P, o, t.sray, busy, 1, deferred, no_tally SRT_PROF_ARG);
            W.add(Src::WAVE_CALLS, 1ull);
            W.add(Src::CLOSEST, wave_lanes(busy));
            if constexpr (Work::TAIL) {  // rules T1 - T6: the lookup runs in wave-uniform control flow, between the hit and the row
                uint32_t atag = 0u;
                const bool ended = busy && pool_hit_update<Work::SUN>(S, h, B, t, atag, diffuse);  // (AS4: the hit the limit is reached at, too)
                // T1, T2: the limit was reached on a surface; T and spec are that hit's, no draw is consumed
                const bool term = ended && h.prim >= 0;
                float g = 0.0f;
                if (term) g = 1.0f - (S.mat(t.hprim, 0).x * t.spec);  // T3 (:175)
                RGB add;
                if (probe_tail_lookup(W.tail, term, t.hp, t.hn, t.T, g, add)) t.L = RGB{t.L.r + add.r, t.L.g + add.g, t.L.b + add.b};  // T5
                if (ended) {
                    pool_store_row(rows, c0, atag, t);
                    busy = false;
                }
            } else if (busy) {
                uint32_t atag = 0u;
                if (pool_hit_update<Work::SUN>(S, h, B, t, atag, diffuse)) {
                    pool_store_row(rows, c0, atag, t);
                    busy = false;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        // The wave's own stores, made by whichever lane ran the path, are read back by the slots' owner lanes: the ROWS
        // kernel's release / acquire pair at workgroup scope (see pathtrace_kernel); no other wave ever touches these rows.
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (ch.owner()) pool_fold_rows(src, rows + lane, c0, ch.count(), acc);
    }
}

}  // namespace srt
