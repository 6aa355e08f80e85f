    // srt_light_probes_body.inc — the text of light_probe_kernel, light_probe_tail_kernel and light_probe_sun_kernel
    // (srt_light_probes.hip.h includes it into all three).  Reads the kernel's P and io, its template parameters, and TAIL, SUN, COUNT,
    // tio and sio as the including function has them.
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
#if defined(SRT_STATS) && SRT_STATS == 3
    Prof prof{};
#endif
    Tally<false> no_tally;
    // (named through a template parameter: the type is dependent in every including kernel, so the branches of the modes a kernel
    // does not have are discarded without being checked against its Work)
    using WorkOfMode = std::conditional_t<SUN, LpSunWork, std::conditional_t<TAIL, LpTailWork, LpWork<COUNT>>>;
    std::conditional_t<SCENE_LDS, WorkOfMode, WorkOfMode> W;
    if constexpr (TAIL) W.tail.io = tio;
    if constexpr (SUN) W.sun = sio;
    W.add(LP_WORK_WAVES, 1ull);
    auto lanes = [](bool b) { return (unsigned long long)__builtin_popcountll(__builtin_amdgcn_ballot_w64(b)); };
    auto below = [](unsigned long long m) { return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)); };
    // this wave's region of the scratch: RAD_CHUNK rows of 64 slots
    float4* const rows = io.rows + ((size_t)blockIdx.x * WAVES + (size_t)wave) * (size_t)(RAD_CHUNK * 64);
    float* const rec = S.pix;                                      // [64][12]: dir, n0, p0, prim0, the key's seed-and-id half
    unsigned* const match = reinterpret_cast<unsigned*>(S.work);  // [64] of (sample << 6 | slot), ~0 = nothing
    const uint32_t n = P.sample_count;
    const int B = P.max_bounces;
    const bool reset = (P.flags & 1u) != 0;
    const uint32_t K = io.directions, J = io.blocks;
    uint32_t listed = io.probes;
    if constexpr (LISTED) {
        const uint32_t ln = io.list[0];              // (one address for the launch)
        listed = ln < io.probes ? ln : io.probes;  // (a list holds at most P indices: nothing is read past 4 + P)
    }
    const uint32_t units = listed * J;  // P*K <= 2^30, so P*J <= 2^30
    const bool norm = io.normalize != 0u;  // (a kernel argument: wave-uniform)
    // wave-uniform loop: every lane of a wave runs the same trips, so closest_hit sees all 64 lanes in each call
    for (uint32_t u = blockIdx.x * (uint32_t)WAVES + (uint32_t)wave; u < units; u += gridDim.x * (uint32_t)WAVES) {
        uint32_t p = u / J;
        const uint32_t j = u - p * J;
        uint32_t slot = u;  // where the projection goes (unlisted, J == 1: u == p)
        if constexpr (LISTED) {
            // wave-uniform values, moved to scalar registers: the listed instantiations keep the vector register count, and with it
            // the occupancy, of the unlisted ones
            const uint32_t us = (uint32_t)__builtin_amdgcn_readfirstlane((int)u);
            p = (uint32_t)__builtin_amdgcn_readfirstlane((int)io.list[4u + p]);
            if (p >= io.probes) continue;  // a bad word skips the unit: no store can go out of range
            slot = J == 1u ? p : us;
        }
        const uint32_t k = (j << 6) + (uint32_t)lane;
        const bool active = k < K;
        const uint32_t i = p * K + k;  // the ray's element and stream offset (< 2^30 for an active lane)
        // lanes past K load no direction: they carry a harmless unit ray through the primary call and own no slot
        const float4 o4 = io.position[p];  // (one address for the wave: a broadcast 16-byte load)
        float4 d4 = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
        if (active) d4 = io.direction[k];
        V3 dir0 = v3(d4.x, d4.y, d4.z);
        if (norm) dir0 = normalized(dir0);  // float3::Normalized (Common.hpp:159-162); its window test is wave-level: called by all lanes
        bool deferred = false;              // (defer_min = 1: every call resolves its mesh rays itself)
        // ---- primary hit: identical for every sample (Raytracer.cpp:142)
        const Hit h0 = closest_hit<MESH, false, SCENE_LDS>(S, P, v3(o4.x, o4.y, o4.z), dir0, active, 1, deferred, no_tally SRT_PROF_ARG);
        const bool traced = active && h0.prim >= 0 && B > 0;
        W.add(LP_WORK_WAVE_CALLS, 1ull);
        W.add(LP_WORK_PROBES, j == 0u ? 1ull : 0ull);
        W.add(LP_WORK_RAYS, lanes(active));
        W.add(LP_WORK_SAMPLES, lanes(active) * n);
        W.add(LP_WORK_CLOSEST, lanes(active && !traced) * n);  // the primary counts once per sample (srt_stats.rays' rule)
        float4 acc = make_float4(0, 0, 0, 0);
        if (active && !reset) acc = io.radiance[i];  // (the host refuses a continuation without the RADIANCE output)
        // ---- rays whose colour does not depend on the sample: a miss -> env(d) every sample (:143-145); MAXBOUNCES == 0 ->
        // the first hit's EmissiveColor (:162, 212)
        if (active && !traced) {
            RGB c;
            float ca = 0.0f;  // the colour's alpha (+0 from the emissive colour)
            if (h0.prim < 0) {
                c = environment(S, dir0);
                ca = environment_alpha(dir0);
            } else {
                const float4 m1 = S.mat(h0.prim, 1);
                c = RGB{clamp0(m1.y), clamp0(m1.z), clamp0(m1.w)};
            }
            for (uint32_t s = 0; s < n; ++s) accumulate_sample(P, acc, c, ca, s);
        }
        if (__builtin_amdgcn_ballot_w64(traced) != 0ull) {
            // ---- wave-level path pool over (slot, sample): lane l owns slot l
            if (traced) {
                float* r = rec + lane * 12;
                r[0] = dir0.x, r[1] = dir0.y, r[2] = dir0.z;
                r[3] = h0.n.x, r[4] = h0.n.y, r[5] = h0.n.z;
                r[6] = h0.p.x, r[7] = h0.p.y, r[8] = h0.p.z;
                r[9] = __int_as_float(h0.prim);
                // srt_rng_key's first two rounds depend on seed and id only: done here once, the sample's round at the hand-out
                r[10] = __uint_as_float(srt_mix32(srt_mix32(P.seed ^ 0xA511E9B3U) + (io.id_base + i)));
            }
            __builtin_amdgcn_wave_barrier();
            // path state of the task this lane is running
            bool busy = false;
            uint32_t task = 0;  // sample << 6 | slot
            RGB L{0, 0, 0}, T{0, 0, 0};
            V3 sray = v3(0, 0, 1), hn = v3(0, 0, 0), hp = v3(0, 0, 0);
            int hprim = 0, bounce = 0;
            float spec = 0.0f;
            uint32_t rng = 0;
            int rot = 0;  // wave-uniform rotation of the slot priority
            for (uint32_t c0 = 0; c0 < n; c0 += (uint32_t)RAD_CHUNK) {  // (wave-uniform)
                const uint32_t end = n - c0 < (uint32_t)RAD_CHUNK ? n : c0 + (uint32_t)RAD_CHUNK;
                uint32_t own_next = traced ? c0 : end;  // samples [c0, own_next) of this slot have been handed out
                // the fold of the chunk before has read the rows this chunk's paths overwrite
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                while (__builtin_amdgcn_ballot_w64(busy || own_next < end) != 0ull) {
                    // ---- hand out tasks: radiance_kernel's two-pass round-robin deal of the slots to the free lanes
                    bool fresh = false;
                    for (int pass = 0; pass < 2; ++pass) {
                        const unsigned long long freem = __builtin_amdgcn_ballot_w64(!busy);
                        const int avail = own_next < end ? (int)(end - own_next) : 0;
                        const bool can = avail > 0;
                        const unsigned long long canm = __builtin_amdgcn_ballot_w64(can);
                        if (freem == 0ull || canm == 0ull) break;
                        const int nfree = __builtin_popcountll(freem), ncan = __builtin_popcountll(canm);
                        rot = (rot + 23) & 63;
                        const int crank = below(canm) - __builtin_popcountll(canm & ((1ull << rot) - 1ull)) + (lane < rot ? ncan : 0);
                        const int frank = below(freem);
                        if (!busy) match[frank] = 0xFFFFFFFFu;
                        __builtin_amdgcn_wave_barrier();
                        if (can) {
                            int given = 0;
                            for (int q = crank; q < nfree && given < avail; q += ncan) {
                                match[q] = ((own_next + (uint32_t)given) << 6) | (unsigned)lane;
                                ++given;
                            }
                            own_next += (uint32_t)given;
                        }
                        __builtin_amdgcn_wave_barrier();
                        const unsigned m = !busy ? match[frank] : 0xFFFFFFFFu;
                        if (m != 0xFFFFFFFFu) {  // (the sample is set up below, once for the lanes of both passes)
                            task = m;
                            busy = true;
                            fresh = true;
                        }
                        __builtin_amdgcn_wave_barrier();
                    }
                    if (fresh) {  // a lane that has just taken a task: Raytracer.cpp:162-166 for sample sidx of that ray
                        const uint32_t sidx = task >> 6;
                        const float* r = rec + (int)(task & 63u) * 12;
                        const int prim0 = __float_as_int(r[9]);
                        rng = srt_mix32(__float_as_uint(r[10]) + (P.first_sample + sidx));  // = srt_rng_key(seed, id, sample), see the record
                        const uint32_t rr = srt_mix32(rng) >> 17;                            // draw 0: the specular lottery at the first hit
                        rng += 0x9E3779B9U;
                        const float4 m0 = S.mat(prim0, 0), m1 = S.mat(prim0, 1);
                        spec = (m0.y >= rand_unit(rr)) ? 1.0f : 0.0f;  // :165
                        L = RGB{m1.y, m1.z, m1.w};                     // :162 (clamped in the image)
                        T = RGB{m0.z, m0.w, m1.x};                     // :163
                        sray = v3(r[0], r[1], r[2]);                   // :164
                        hn = v3(r[3], r[4], r[5]);
                        hp = v3(r[6], r[7], r[8]);
                        hprim = prim0;
                        bounce = 0;
                    }
                    W.add(LP_WORK_CLOSEST, lanes(fresh));  // the sample's primary GetClosestObject call (:142)
                    // ---- one bounce for every busy lane
                    V3 o = v3(0, 0, 0);
                    const float ofs = .00001f;
                    if (busy) {
                        if (bounce != 0) {  // :169-171
                            T = RGB{T.r * 0.8f, T.g * 0.8f, T.b * 0.8f};  // (NN)
                        }
                        // reflectedRay = sray.Reflect(normal)  (:172, Common.hpp:163-165)
                        const float k2 = 2 * dot3(sray, hn);
                        const V3 refl = v3(sray.x - hn.x * k2, sray.y - hn.y * k2, sray.z - hn.z * k2);
                        // GetRandomNormalOrientedHemisphere (:90-105): exactly three draws, x then y then z
                        const uint32_t r0 = srt_mix32(rng) >> 17;
                        const uint32_t r1 = srt_mix32(rng + 0x9E3779B9U) >> 17;
                        const uint32_t r2 = srt_mix32(rng + 2u * 0x9E3779B9U) >> 17;
                        rng += 3u * 0x9E3779B9U;
                        V3 sr = v3((rand_unit(r0) - 0.5f) * 2, (rand_unit(r1) - 0.5f) * 2, (rand_unit(r2) - 0.5f) * 2);
                        sr = normalized_in_window(sr);  // (inside normalized()'s window by construction: see there)
                        if (dot3(sr, hn) < 0) sr = v3(sr.x * -1, sr.y * -1, sr.z * -1);
                        // float3::Lerp(sray, reflectedRay, Smoothness * specularProb)  (:175)
                        const float tt = S.mat(hprim, 0).x * spec;
                        const V3 l = v3(sr.x * (1 - tt) + refl.x * tt, sr.y * (1 - tt) + refl.y * tt, sr.z * (1 - tt) + refl.z * tt);
                        sray = normalized(l);                                            // :176
                        o = v3(hp.x + hn.x * ofs, hp.y + hn.y * ofs, hp.z + hn.z * ofs);  // :177
                    }
                    [[maybe_unused]] bool diffuse = false;  // SUN: this lane's bounce was blind (rule S2); kept across closest_hit for S7
                    if constexpr (SUN) {  // rules S3 - S6 in wave-uniform control flow, before the bounce's own result is added
                        diffuse = busy && (S.mat(hprim, 0).x * spec) == 0.0f;  // tt of :175, as computed above
                        W.add(LP_WORK_WAVE_CALLS, sun_sample<MESH, SCENE_LDS>(S, P, *W.sun, diffuse, rng, o, hn, T, L));
                    }
                    // the scan runs in wave-uniform control flow: idle lanes help with other lanes' rays
                    const Hit h = closest_hit<MESH, false, SCENE_LDS>(S, P, o, sray, busy, 1, deferred, no_tally SRT_PROF_ARG);
                    W.add(LP_WORK_WAVE_CALLS, 1ull);
                    W.add(LP_WORK_CLOSEST, lanes(busy));
                    [[maybe_unused]] bool ended = false;  // TAIL: this lane's path has ended in this step, with this alpha tag
                    [[maybe_unused]] uint32_t ended_atag = 0u;
                    if (busy) {
                        bool end_path;
                        uint32_t atag = 0u;  // the sample's alpha: NaN only from the environment (T's alpha is +0)
                        if (h.prim < 0) {    // :178-181
                            const RGB e = environment<SUN>(S, sray, diffuse);  // (S7: without the sun after a blind bounce)
                            L = RGB{L.r + e.r * T.r, L.g + e.g * T.g, L.b + e.b * T.b};  // (NN)
                            atag = alpha_tag(environment_alpha(sray));
                            end_path = true;
                        } else {
                            const float4 m0 = S.mat(h.prim, 0), m1 = S.mat(h.prim, 1), m2 = S.mat(h.prim, 2);
                            const uint32_t r = srt_mix32(rng) >> 17;  // one lottery per further hit
                            rng += 0x9E3779B9U;
                            spec = (m0.y >= rand_unit(r)) ? 1.0f : 0.0f;  // :182
                            const RGB Em{m1.y, m1.z, m1.w};
                            L = RGB{L.r + Em.r * T.r, L.g + Em.g * T.g, L.b + Em.b * T.b};  // :183 (NN)
                            const RGB Bc{m0.z, m0.w, m1.x}, Sc{m2.x, m2.y, m2.z};
                            const float ns = 1 - spec;  // :184, Color::Lerp with t = 0 or 1 (NN)
                            const RGB f{Bc.r * ns + Sc.r * spec, Bc.g * ns + Sc.g * spec, Bc.b * ns + Sc.b * spec};
                            T = RGB{T.r * f.r, T.g * f.g, T.b * f.b};
                            hn = h.n;
                            hp = h.p;
                            hprim = h.prim;
                            ++bounce;
                            end_path = bounce >= B;
                        }
                        if constexpr (TAIL) {
                            ended = end_path, ended_atag = atag;
                        } else if (end_path) {  // the sample's colour into row (sample - c0), slot, of the wave's region; written exactly once
                            const uint32_t sidx = task >> 6;
                            rows[((sidx - c0) << 6) + (task & 63u)] = make_float4(L.r, L.g, L.b, __uint_as_float(sidx | atag));
                            busy = false;
                        }
                    }
                    if constexpr (TAIL) {  // rules T1 - T5 in wave-uniform control flow, then the row as above
                        const bool term = ended && h.prim >= 0;
                        float g = 0.0f;
                        if (term) g = 1.0f - (S.mat(hprim, 0).x * spec);  // T3 (:175)
                        RGB add;
                        if (probe_tail_lookup(W.tail, term, hp, hn, T, g, add)) L = RGB{L.r + add.r, L.g + add.g, L.b + add.b};  // T5
                        if (ended) {
                            const uint32_t sidx = task >> 6;
                            rows[((sidx - c0) << 6) + (task & 63u)] = make_float4(L.r, L.g, L.b, __uint_as_float(sidx | ended_atag));
                            busy = false;
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                }
                // The wave's own stores, made by whichever lane ran the path, are read back by the slots' owner lanes: the ROWS
                // kernel's release / acquire pair at workgroup scope (see pathtrace_kernel); no other wave ever touches these rows.
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                if (traced) {  // lane l folds rows 0 .. end - c0 - 1 of slot l, in sample order
                    const float4* row = rows + lane;
                    const uint32_t cnt = end - c0;
                    uint32_t s = 0;
                    for (; s + ROWS_IN_FLIGHT <= cnt; s += ROWS_IN_FLIGHT) {
                        float4 c[ROWS_IN_FLIGHT];
#pragma unroll
                        for (int q = 0; q < ROWS_IN_FLIGHT; ++q) c[q] = row[(size_t)(s + q) * 64];
#pragma unroll
                        for (int q = 0; q < ROWS_IN_FLIGHT; ++q) accumulate_sample(P, acc, RGB{c[q].x, c[q].y, c[q].z}, tag_alpha(__float_as_uint(c[q].w)), c0 + s + q);
                    }
                    for (; s < cnt; ++s) {
                        const float4 c = row[(size_t)s * 64];
                        accumulate_sample(P, acc, RGB{c.x, c.y, c.z}, tag_alpha(__float_as_uint(c.w)), c0 + s);
                    }
                }
            }
        }
        if (active && io.radiance) io.radiance[i] = acc;
        // ---- the projection: t_c = w * b_c on the direction as traced, v = (L.r t_c, L.g t_c, L.b t_c, t_c), +0 past K
        float4* const dst = J == 1u ? io.coefficients : io.partial;  // (wave-uniform; NULL: COEFFICIENTS not requested)
        if (dst) {
            // the direction as traced, loaded and normalized again (the same expressions on the same input: the same bits) rather than
            // kept in registers across the pool
            float4 e4 = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
            if (active) e4 = io.direction[k];
            V3 dirp = v3(e4.x, e4.y, e4.z);
            if (norm) dirp = normalized(dirp);
            const float x = dirp.x, y = dirp.y, z = dirp.z, w = e4.w;
            float b[LP_COEFFS];
            b[0] = 0.282095f;
            b[1] = 0.488603f * y;
            b[2] = 0.488603f * z;
            b[3] = 0.488603f * x;
            b[4] = 1.092548f * (x * y);
            b[5] = 1.092548f * (y * z);
            b[6] = 0.315392f * ((3.0f * (z * z)) - 1.0f);
            b[7] = 1.092548f * (x * z);
            b[8] = 0.546274f * ((x * x) - (y * y));
            float4* const out = dst + (size_t)slot * LP_COEFFS;
#pragma unroll
            for (int c = 0; c < LP_COEFFS; ++c) {
                const float t = w * b[c];
                const float sr = lp_wave_tree(active ? acc.x * t : 0.0f);
                const float sg = lp_wave_tree(active ? acc.y * t : 0.0f);
                const float sb = lp_wave_tree(active ? acc.z * t : 0.0f);
                const float sw = lp_wave_tree(active ? t : 0.0f);
                if (lane == 0) out[c] = make_float4(sr, sg, sb, sw);
            }
        }
        __builtin_amdgcn_wave_barrier();  // (the next unit rewrites the records)
    }
    if constexpr (TAIL) {
        if (io.work) {
            unsigned long long v = 0ull;
#pragma unroll
            for (int q = 0; q < LP_WORK_N; ++q) v = lane == q ? W.n[q] : v;
            if (lane < LP_WORK_N) atomicAdd(&io.work[lane], v);
        }
        W.tail.flush(lane);
    } else if constexpr (SUN) {  // the sums are always kept; flushed when the launch has the record
        if (io.work) {
            unsigned long long v = 0ull;
#pragma unroll
            for (int q = 0; q < LP_WORK_N; ++q) v = lane == q ? W.n[q] : v;
            if (lane < LP_WORK_N) atomicAdd(&io.work[lane], v);
        }
    } else if constexpr (COUNT) {  // the wave's sums: lane k adds counter k — one vector atomic per wave
        unsigned long long v = 0ull;
#pragma unroll
        for (int q = 0; q < LP_WORK_N; ++q) v = lane == q ? W.n[q] : v;
        if (lane < LP_WORK_N) atomicAdd(&io.work[lane], v);
    }
