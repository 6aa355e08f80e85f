    // srt_adaptive_body.inc — the text of adaptive_kernel, adaptive_tail_kernel, adaptive_sun_kernel and adaptive_tail_sun_kernel
    // (srt_adaptive.hip.h includes it into all four and says why).  Reads the kernel's P and io, its template parameters, and TAIL,
    // SUN, COUNT, tio and sio as the including function has them.
    extern __shared__ float4 lds_scene[];
    stage_scene<SCENE_LDS>(P, lds_scene);
    constexpr int WAVES = WG_TILES_X * WG_TILES_Y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Lds S = make_lds<SCENE_LDS>(P, lds_scene, WAVES, wave);
#if defined(SRT_STATS) && SRT_STATS == 3
    Prof prof{};
#endif
    Tally<false> no_tally;
    // (named through a template parameter: the type is dependent in every including kernel, so the branches of the modes a kernel
    // does not have are discarded without being checked against its Work)
    using WorkOfMode = std::conditional_t<SUN, std::conditional_t<TAIL, TailSunWaveWork<ADP_WORK_N>, SunWaveWork<ADP_WORK_N>>,
                                          std::conditional_t<TAIL, TailWaveWork<ADP_WORK_N>, WaveWork<COUNT, ADP_WORK_N>>>;
    std::conditional_t<SCENE_LDS, WorkOfMode, WorkOfMode> Wk;
    if constexpr (TAIL) Wk.tail.io = tio;
    if constexpr (SUN) Wk.sun = sio;
    float4* const rows = wave_sample_rows(io.rows, wave);
    const int B = P.max_bounces;
    const int W = P.width, H = P.height;
    const int tiles_x = (W + TILE_W - 1) / TILE_W, tiles_y = (P.rows + TILE_H - 1) / TILE_H;
    const uint32_t tiles = (uint32_t)(tiles_x * tiles_y);
    const V3 cam = v3(P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]);
    // wave-uniform loop: every lane of a wave runs the same trips, so closest_hit sees all 64 lanes in each call
    for (;;) {
        uint32_t t = 0u;
        if (lane == 0) t = __hip_atomic_fetch_add(io.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
        if (t >= tiles) break;
        const int tx = (int)(t % (uint32_t)tiles_x), ty = (int)(t / (uint32_t)tiles_x);
        const int px = tx * TILE_W + (lane & 7), py = ty * TILE_H + (lane >> 3);
        const bool in_range = px < W && py < P.rows;
        // lanes outside the frame or band stand on the nearest pixel, load nothing, trace nothing and store nothing
        const int x = px < W ? px : W - 1, y = P.y0 + (py < P.rows ? py : P.rows - 1);
        const uint32_t pix = (uint32_t)x + (uint32_t)y * (uint32_t)W;
        uint32_t n0 = 0u, e = 0u;
        if (in_range) {
            n0 = io.counts[pix];
            e = effective_budget(io.budget[pix], n0, io.max_samples);
        }
        const bool want = e > 0u;
        if (__builtin_amdgcn_ballot_w64(want) == 0ull) continue;
        // ---- GetRayDirection (Raytracer.cpp:106-122), as gbuffer_kernel / pathtrace_kernel ----
        float nX = ((float)x / (float)W) * 2 - 1;
        float nY = ((float)y / (float)H) * 2 - 1;
        V3 u = v3(P.right_rd[0] * nX, P.right_rd[1] * nX, P.right_rd[2] * nX);
        V3 vv = v3(P.up_ld[0] * nY, P.up_ld[1] * nY, P.up_ld[2] * nY);
        const V3 dir0 = normalized(v3((u.x + vv.x) + P.fwd_clip[0], (u.y + vv.y) + P.fwd_clip[1], (u.z + vv.z) + P.fwd_clip[2]));
        bool deferred = false;  // (defer_min = 1: every call resolves its mesh rays itself)
        // ---- primary hit: identical for every sample (Raytracer.cpp:142); pixels without a budget trace no ray
        const Hit h0 = closest_hit<MESH, false, SCENE_LDS>(S, P, cam, dir0, want, 1, deferred, no_tally SRT_PROF_ARG);
        const bool traced = want && h0.prim >= 0 && B > 0;
        const uint32_t first_frame = n0 + 1u;  // (n0 < ADP_FRAME_LIMIT where want)
        Wk.add(ADP_WORK_WAVE_CALLS, 1ull);
        Wk.add(ADP_WORK_PIXELS, wave_lanes(want));
        if constexpr (COUNT) {
            Wk.add(ADP_WORK_SAMPLES, (unsigned long long)wave_sum_u32(e));
            Wk.add(ADP_WORK_CLOSEST, (unsigned long long)wave_sum_u32(traced ? 0u : e));  // the primary counts once per sample (srt_stats.rays' rule)
        }
        float4 acc = make_float4(0, 0, 0, 0);
        if (want && n0 != 0u) acc = P.accumulator[pix];
        // samples [0, lim) of this slot; the chunk loop runs to the tile's largest
        const uint32_t lim = traced ? e : 0u;
        const PixelSamples samples{lim, first_frame};
        if (want && !traced) {  // the colour does not depend on the sample
            fold_constant_colour(S, samples, dir0, h0, e, acc);
            store_pixel(P, pix, acc);
            if (!io.keep_counts) io.counts[pix] = n0 + e;
        }
        if (__builtin_amdgcn_ballot_w64(traced) == 0ull) continue;
        if (traced) {  // srt_rng_key's id of a pixel: its index
            write_first_hit_record(S, lane, dir0, h0, P.seed, pix);
            S.pix[lane * 12 + 11] = __uint_as_float(first_frame);
        }
        __builtin_amdgcn_wave_barrier();
        run_sample_pool<MESH, SCENE_LDS>(S, P, samples, rows, lane, acc, Wk SRT_PROF_ARG);
        if (traced) {
            store_pixel(P, pix, acc);
            if (!io.keep_counts) io.counts[pix] = n0 + e;
        }
        __builtin_amdgcn_wave_barrier();  // (the next tile rewrites the records)
    }
    Wk.flush(io.work, lane);
