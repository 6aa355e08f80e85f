    // srt_radiance_body.inc — the text of radiance_kernel, radiance_tail_kernel and radiance_sun_kernel (srt_radiance.hip.h includes
    // it into all three and says why).  Reads the kernel's P and io, its template parameters, and TAIL, SUN, COUNT, tio and sio as the
    // including function has them.
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
    using WorkOfMode = std::conditional_t<SUN, SunWaveWork<RAD_WORK_N>, std::conditional_t<TAIL, TailWaveWork<RAD_WORK_N>, WaveWork<COUNT, RAD_WORK_N>>>;
    std::conditional_t<SCENE_LDS, WorkOfMode, WorkOfMode> W;
    if constexpr (TAIL) W.tail.io = tio;
    if constexpr (SUN) W.sun = sio;
    float4* const rows = wave_sample_rows(io.rows, wave);
    const uint32_t n = P.sample_count;
    const int B = P.max_bounces;
    const bool reset = (P.flags & 1u) != 0;
    const uint32_t blocks = (io.count + 63u) >> 6;  // count <= 2^30: at most 2^24 blocks
    const bool norm = io.normalize != 0u;           // (a kernel argument: wave-uniform)
    // wave-uniform loop: every lane of a wave runs the same trips, so closest_hit sees all 64 lanes in each call
    for (uint32_t b = blockIdx.x * (uint32_t)WAVES + (uint32_t)wave; b < blocks; b += gridDim.x * (uint32_t)WAVES) {
        const uint32_t i = (b << 6) + (uint32_t)lane;
        const bool active = i < io.count;
        // lanes past the batch load nothing: they carry a harmless unit ray through the primary call and own no slot
        float4 o4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), d4 = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
        if (active) o4 = io.origin[i], d4 = io.direction[i];  // 16-byte loads
        V3 dir0 = v3(d4.x, d4.y, d4.z);
        if (norm) dir0 = normalized(dir0);  // float3::Normalized (Common.hpp:159-162); its window test is wave-level: called by all lanes
        bool deferred = false;              // (defer_min = 1: every call resolves its mesh rays itself)
        // ---- primary hit: identical for every sample (Raytracer.cpp:142)
        const Hit h0 = closest_hit<MESH, false, SCENE_LDS>(S, P, v3(o4.x, o4.y, o4.z), dir0, active, 1, deferred, no_tally SRT_PROF_ARG);
        const bool traced = active && h0.prim >= 0 && B > 0;
        W.add(RAD_WORK_WAVE_CALLS, 1ull);
        W.add(RAD_WORK_RAYS, wave_lanes(active));
        W.add(RAD_WORK_SAMPLES, wave_lanes(active) * n);
        W.add(RAD_WORK_CLOSEST, wave_lanes(active && !traced) * n);  // the primary counts once per sample (srt_stats.rays' rule)
        float4 acc = make_float4(0, 0, 0, 0);
        if (active && !reset) acc = io.out[i];
        const LaunchSamples<RAD_WORK_CLOSEST, RAD_WORK_WAVE_CALLS> samples{P, traced};
        if (active && !traced) {  // the colour does not depend on the sample
            fold_constant_colour(S, samples, dir0, h0, n, acc);
            io.out[i] = acc;
        }
        if (__builtin_amdgcn_ballot_w64(traced) == 0ull) continue;
        // srt_rng_key's id of ray i: id_base + i
        if (traced) write_first_hit_record(S, lane, dir0, h0, P.seed, io.id_base + i);
        __builtin_amdgcn_wave_barrier();
        run_sample_pool<MESH, SCENE_LDS>(S, P, samples, rows, lane, acc, W SRT_PROF_ARG);
        if (traced) io.out[i] = acc;
        __builtin_amdgcn_wave_barrier();  // (the next block rewrites the records)
    }
    W.flush(io.work, lane);
