// adaptive_sun_check.cpp — the host-side rules of SRT_ADAPTIVE_SUN_SAMPLING (software-raytracer_amd/csrc/srt_adaptive_sun_host.h,
// rules AS5 and AS6 of srt_pathtrace.h) as a stand-alone program: the flag's value and that the adaptive calls' own mask is still
// 3; the wrappers' order of refusals — bits 4 and 8 with the calls' own argument errors, each own error in its order, for the tail
// call the mode and the grid's inputs and the overlaps, and the sun's direction last; that the direction is nobody's business
// without the bit and is tested with max_bounces == 0 too; that the probe-tail mode never refuses the flag here; and which of
// the four kernels a call selects for every (tail call, mode, flag, max_bounces 0 / 1) combination.
// Built with -fsanitize=address,undefined and run on the CPU.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "srt_adaptive_sun_host.h"
#include "srt_pathtrace.h"

using namespace srt;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // the flag: 16, outside the mask of the calls' own checks, which stays 3
    CHECK(SRT_ADAPTIVE_SUN_SAMPLING == 16u && ADAPTIVE_FLAG_SUN_SAMPLING == 16u && SUN_SAMPLING_FLAG == 16u);
    CHECK(ADAPTIVE_FLAG_ALL == 3u && !(ADAPTIVE_FLAG_ALL & ADAPTIVE_FLAG_SUN_SAMPLING));
    CHECK(SRT_ADAPTIVE_KEEP_COUNTS == 1u && SRT_ADAPTIVE_COUNT_WORK == 2u);
    CHECK(sizeof(srt_adaptive_params) == 28 && sizeof(AdaptiveCall) == 28);

    constexpr int W = 6, H = 4;
    constexpr size_t PROBES = 2 * 3 * 2, COEFF_BYTES = PROBES * 9 * 16;
    alignas(16) static unsigned char mem[W * H * 16 + W * H * 4 + COEFF_BYTES + 256];
    unsigned char* const acc = mem;
    unsigned char* const fb = acc + W * H * 16;
    unsigned char* const coeff = fb + W * H * 4;
    const AdaptiveTailTargets tg = adaptive_tail_targets(acc, fb, W, H);

    const float unit[3] = {0.0f, -1.0f, 0.0f}, diagonal[3] = {0.57735027f, -0.57735027f, -0.57735027f};
    const float bad[4][3] = {{0.0f, -2.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {nan, -1.0f, 0.0f}, {inf, 0.0f, 0.0f}};
    const char* why = nullptr;

    AdaptiveCall c;
    adaptive_call_default(c);
    c.row_begin = 0, c.row_end = H, c.max_bounces = 1, c.flags = 16u;

    // ---- srt_render_adaptive (AS5): the own errors in their order with the bit taken out, then the direction
    {
        auto check = [&](const AdaptiveCall& call, bool scene, bool camera, bool counts, bool budget, const float* dir) {
            return sun_adaptive_check(call, scene, camera, H, counts, budget, dir, &why);
        };
        AdaptiveCall v = c;
        v.row_end = H + 1, v.flags = 16u | 4u, v.reserved = 1u, v.max_samples = 0u, v.max_bounces = -1;
        CHECK(check(v, false, false, false, false, bad[0]) == RAYS_STATE && std::strstr(why, "srt_set_scene"));
        CHECK(check(v, true, false, false, false, bad[0]) == RAYS_STATE && std::strstr(why, "srt_set_camera"));
        CHECK(check(v, true, true, false, false, bad[0]) == RAYS_INVALID_ARG && std::strstr(why, "row band"));
        v.row_end = H;
        // bits 4 and 8, alone and with 16, and every other unknown bit: the call's own "unknown flags"
        for (uint32_t f : {4u, 8u, 4u | 16u, 8u | 16u, 12u | 16u | 3u, 32u, 32u | 16u, 0x80000010u, ~0u, ~16u}) {
            v.flags = f;
            CHECK(check(v, true, true, false, false, bad[0]) == RAYS_INVALID_ARG && std::strstr(why, "flags"));
        }
        v.flags = 16u | 3u;
        CHECK(check(v, true, true, false, false, bad[0]) == RAYS_INVALID_ARG && std::strstr(why, "reserved"));
        v.reserved = 0u;
        CHECK(check(v, true, true, false, false, bad[0]) == RAYS_INVALID_ARG && std::strstr(why, "max_samples"));
        v.max_samples = 4096u;
        CHECK(check(v, true, true, false, false, bad[0]) == RAYS_INVALID_ARG && std::strstr(why, "max_bounces"));
        v.max_bounces = 1;
        CHECK(check(v, true, true, false, false, bad[0]) == RAYS_STATE && std::strstr(why, "sample counts"));
        CHECK(check(v, true, true, true, false, bad[0]) == RAYS_STATE && std::strstr(why, "sample budget"));
        // every one of them is what adaptive_check gives without the bit
        {
            AdaptiveCall u = v;
            u.flags &= ~16u;
            const char* why2 = nullptr;
            CHECK(check(v, true, true, true, false, bad[0]) == adaptive_check(u, true, true, H, true, false, &why2) && !std::strcmp(why, why2));
            CHECK(adaptive_check(v, true, true, H, true, true, &why2) == RAYS_INVALID_ARG);  // (the call's own check alone refuses the bit)
        }
        // ... and only then the direction, with every flag set below 16, also at max_bounces == 0
        for (uint32_t f = 0; f <= 3u; ++f)
            for (int32_t b : {0, 1, 8}) {
                v.flags = f | 16u, v.max_bounces = b;
                CHECK(check(v, true, true, true, true, unit) == RAYS_OK && check(v, true, true, true, true, diagonal) == RAYS_OK);
                for (const auto& d : bad) CHECK(check(v, true, true, true, true, d) == RAYS_STATE && std::strstr(why, "sun_direction"));
                // without the bit the direction is nobody's business
                v.flags = f;
                for (const auto& d : bad) CHECK(check(v, true, true, true, true, d) == RAYS_OK);
            }
        CHECK(sun_adaptive_check(c, true, true, H, true, true, bad[1], nullptr) == RAYS_STATE);  // (a NULL reason is allowed)
        CHECK(std::strstr((check(c, true, true, true, true, bad[2]), why), "finite") && std::strstr((check(c, true, true, true, true, bad[0]), why), "unit"));
    }

    // ---- srt_render_adaptive_tail (AS5): all of R1, then the direction
    ProbeTailState tail;  // off
    ProbeGridState g;
    ProbeGridDepthState d;
    ProbeStatesState st;
    {
        auto check = [&](const AdaptiveCall& call, bool counts, bool budget, const void* co, const float* dir) {
            return sun_adaptive_tail_check(call, true, true, H, counts, budget, tail, g, d, st, co, tg, dir, &why);
        };
        AdaptiveCall v = c;
        v.flags = 16u | 8u;
        CHECK(check(v, false, false, coeff, bad[0]) == RAYS_INVALID_ARG && std::strstr(why, "flags"));
        v.flags = 16u | 4u;
        CHECK(check(v, true, true, coeff, bad[0]) == RAYS_INVALID_ARG && std::strstr(why, "flags"));
        v.flags = 16u;
        CHECK(check(v, false, false, coeff, bad[0]) == RAYS_STATE && std::strstr(why, "sample counts"));
        CHECK(check(v, true, false, coeff, bad[0]) == RAYS_STATE && std::strstr(why, "sample budget"));
        // the mode off: before the direction, at any bounce count
        CHECK(check(v, true, true, coeff, bad[0]) == RAYS_STATE && std::strstr(why, "srt_probe_tail is off"));
        v.max_bounces = 0;
        CHECK(check(v, true, true, coeff, bad[0]) == RAYS_STATE && std::strstr(why, "srt_probe_tail is off"));
        ProbeTailCall set = probe_tail_defaults();
        set.flags = PROBE_TAIL_FLAG_DEPTH | PROBE_TAIL_FLAG_STATES;
        probe_tail_set(tail, set);
        // R2 with the flag: no grid input is checked, but the direction is
        CHECK(check(v, true, true, nullptr, unit) == RAYS_OK);
        CHECK(check(v, true, true, nullptr, bad[0]) == RAYS_STATE && std::strstr(why, "sun_direction"));
        v.flags = 0u;
        CHECK(check(v, true, true, nullptr, bad[0]) == RAYS_OK);
        v.flags = 16u, v.max_bounces = 1;
        // the grid's inputs in the probe-tail block's order, each before the direction
        CHECK(check(v, true, true, coeff, bad[0]) == RAYS_STATE && std::strstr(why, "no grid"));
        g.grid_set = true, g.grid = ProbeGrid{{0, 0, 0}, {1, 1, 1}, {2, 3, 2}};
        CHECK(check(v, true, true, coeff, bad[0]) == RAYS_STATE && std::strstr(why, "no coefficients"));
        g.coefficients.bound = coeff, g.coefficients.bound_count = PROBES - 1;
        CHECK(check(v, true, true, coeff, bad[0]) == RAYS_STATE && std::strstr(why, "coefficient count"));
        g.coefficients.bound_count = PROBES;
        CHECK(check(v, true, true, coeff, bad[0]) == RAYS_STATE && std::strstr(why, "no depth maps"));
        d.moments.bound = coeff, d.moments.bound_count = PROBES, d.bound_resolution = 4;
        CHECK(check(v, true, true, coeff, bad[0]) == RAYS_STATE && std::strstr(why, "no states"));
        st.states.bound = coeff, st.states.bound_count = PROBES;
        // the two overlaps
        CHECK(check(v, true, true, acc, bad[0]) == RAYS_STATE && std::strstr(why, "this call writes") && !std::strstr(why, "framebuffer"));
        CHECK(check(v, true, true, fb, bad[0]) == RAYS_STATE && std::strstr(why, "framebuffer"));
        // ... and last the direction; the mode is on and does not refuse the flag (AS4)
        for (const auto& dir : bad) CHECK(check(v, true, true, coeff, dir) == RAYS_STATE && std::strstr(why, "sun_direction"));
        CHECK(check(v, true, true, coeff, unit) == RAYS_OK && check(v, true, true, coeff, diagonal) == RAYS_OK);
        CHECK(sun_adaptive_tail_check(v, true, true, H, true, true, tail, g, d, st, coeff, tg, unit, nullptr) == RAYS_OK);
        // without the bit the wrapper is adaptive_tail_check
        v.flags = 3u;
        for (const auto& dir : bad) CHECK(check(v, true, true, coeff, dir) == RAYS_OK);
        const char* why2 = nullptr;
        CHECK(check(v, true, true, acc, unit) == adaptive_tail_check(v, true, true, H, true, true, tail, g, d, st, acc, tg, &why2) && !std::strcmp(why, why2));
        // srt_render_adaptive with the flag while the mode is on: accepted (AS1); the radiance call's refusal is S5's own
        CHECK(tail.enabled && sun_adaptive_check(c, true, true, H, true, true, unit, &why) == RAYS_OK);
        CHECK(sun_sampling_check(unit, tail.enabled, &why) == RAYS_STATE && std::strstr(why, "srt_probe_tail"));
    }

    // ---- AS6: which kernel runs, for every combination
    {
        ProbeTailState off, on;
        probe_tail_set(on, probe_tail_defaults());
        CHECK(!off.enabled && on.enabled);
        for (int tail_call = 0; tail_call < 2; ++tail_call)
            for (int mode = 0; mode < 2; ++mode)
                for (uint32_t sun : {0u, 16u})
                    for (uint32_t low = 0; low <= 3u; ++low)
                        for (int32_t b : {0, 1, 8}) {
                            AdaptiveCall v = c;
                            v.flags = low | sun, v.max_bounces = b;
                            const bool t = tail_call && mode && b >= 1, s = sun != 0u && b >= 1;
                            const AdaptiveKernelChoice want = t ? (s ? ADAPTIVE_KERNEL_TAIL_SUN : ADAPTIVE_KERNEL_TAIL) : (s ? ADAPTIVE_KERNEL_SUN : ADAPTIVE_KERNEL_PLAIN);
                            CHECK(adaptive_kernel_choice(tail_call != 0, mode ? on : off, v) == want);
                        }
        // the four are distinct, and the plain one is what both calls launch at max_bounces == 0 (AS6, R2)
        CHECK(ADAPTIVE_KERNEL_PLAIN != ADAPTIVE_KERNEL_TAIL && ADAPTIVE_KERNEL_SUN != ADAPTIVE_KERNEL_TAIL_SUN && ADAPTIVE_KERNEL_TAIL != ADAPTIVE_KERNEL_SUN &&
              ADAPTIVE_KERNEL_PLAIN != ADAPTIVE_KERNEL_SUN && ADAPTIVE_KERNEL_PLAIN != ADAPTIVE_KERNEL_TAIL_SUN && ADAPTIVE_KERNEL_TAIL != ADAPTIVE_KERNEL_TAIL_SUN);
        // the work record follows COUNT_WORK, whatever the sun bit says
        AdaptiveState a;
        adaptive_rendered(a, 16u);
        CHECK(a.call.work() == RAYS_STATE);
        adaptive_rendered(a, 16u | ADAPTIVE_FLAG_COUNT_WORK);
        CHECK(a.call.work() == RAYS_OK);
    }

    if (failures) return 1;
    std::printf("ok adaptive sun sampling host rules\n");
    return 0;
}
