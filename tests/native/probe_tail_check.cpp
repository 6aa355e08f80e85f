// probe_tail_check.cpp — the host-side rules of the probe tail (software-raytracer_amd/csrc/srt_probe_tail_host.h) as a stand-alone
// program: the header's struct layouts, the defaults, every refusal of srt_probe_tail with its edges, the rule "a refused call
// leaves the setting", what an affected trace requires of the grid's inputs (in the header's order), the byte-range overlap
// predicate with its edges (adjacent ranges, empty ranges, a range at the top of the address space), and when the work record may
// be read.  Built with -fsanitize=address,undefined and run on the CPU.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "srt_probe_tail_host.h"
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
    // the layouts are the ones the rules use
    CHECK(sizeof(srt_probe_tail_params) == 32 && sizeof(ProbeTailCall) == 32 && sizeof(srt_probe_tail_work) == 56);
    CHECK(offsetof(srt_probe_tail_params, enabled) == 0 && offsetof(ProbeTailCall, enabled) == 0);
    CHECK(offsetof(srt_probe_tail_params, flags) == 4 && offsetof(ProbeTailCall, flags) == 4);
    CHECK(offsetof(srt_probe_tail_params, band_weight) == 8 && offsetof(ProbeTailCall, band_weight) == 8);
    CHECK(offsetof(srt_probe_tail_params, bias) == 20 && offsetof(ProbeTailCall, bias) == 20);
    CHECK(offsetof(srt_probe_tail_params, min_variance) == 24 && offsetof(ProbeTailCall, min_variance) == 24);
    CHECK(offsetof(srt_probe_tail_params, reserved) == 28 && offsetof(ProbeTailCall, reserved) == 28);
    CHECK(offsetof(srt_probe_tail_work, tails) == 8 && offsetof(srt_probe_tail_work, wave_lookups) == 48);
    CHECK(SRT_PROBE_TAIL_NORMAL_WEIGHT == PROBE_TAIL_FLAG_NORMAL_WEIGHT && SRT_PROBE_TAIL_DEPTH == PROBE_TAIL_FLAG_DEPTH &&
          SRT_PROBE_TAIL_STATES == PROBE_TAIL_FLAG_STATES && SRT_PROBE_TAIL_COUNT_WORK == PROBE_TAIL_FLAG_COUNT_WORK && PROBE_TAIL_FLAG_ALL == 15u);

    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float tiny = std::numeric_limits<float>::denorm_min();
    const char* why = nullptr;

    // the defaults, and the state before any call
    const ProbeTailCall def = probe_tail_defaults();
    CHECK(def.enabled == 1 && def.flags == 0 && def.band_weight[0] == 1.0f && def.band_weight[1] == 0.5f && def.band_weight[2] == 0.0f);
    CHECK(def.bias == 0.0f && def.min_variance == 1e-4f && def.reserved == 0);
    CHECK(probe_tail_check(def, &why) == RAYS_OK && probe_tail_check(def, nullptr) == RAYS_OK);
    ProbeTailState s;
    CHECK(!s.enabled && !s.last.ran && !s.last.counted && s.last.work() == RAYS_STATE && !probe_tail_applies(s, 8));

    // every refusal: each error hides the later ones
    {
        ProbeTailCall v{2, 16u, {nan, 0.5f, 0.0f}, -1.0f, 0.0f, 1u};
        CHECK(probe_tail_check(v, &why) == RAYS_INVALID_ARG && std::strstr(why, "enabled"));
        v.enabled = 0;  // (also when switching off)
        CHECK(probe_tail_check(v, &why) == RAYS_INVALID_ARG && std::strstr(why, "flags"));
        v.flags = 15u;
        CHECK(probe_tail_check(v, &why) == RAYS_INVALID_ARG && std::strstr(why, "band_weight"));
        v.band_weight[0] = -inf;  // (any number is a weight)
        CHECK(probe_tail_check(v, &why) == RAYS_INVALID_ARG && std::strstr(why, "bias"));
        v.bias = 0.0f;
        CHECK(probe_tail_check(v, &why) == RAYS_INVALID_ARG && std::strstr(why, "min_variance"));
        v.min_variance = tiny;
        CHECK(probe_tail_check(v, &why) == RAYS_INVALID_ARG && std::strstr(why, "reserved"));
        v.reserved = 0;
        CHECK(probe_tail_check(v, &why) == RAYS_OK);
    }
    for (int e : {-1, 2, 3, std::numeric_limits<int>::max(), std::numeric_limits<int>::min()}) {
        ProbeTailCall v = def;
        v.enabled = e;
        CHECK(probe_tail_check(v, &why) == RAYS_INVALID_ARG && std::strstr(why, "enabled"));
    }
    for (uint32_t f : {16u, 32u, 0x80000000u, ~0u, 15u | 64u}) {
        ProbeTailCall v = def;
        v.flags = f;
        CHECK(probe_tail_check(v, &why) == RAYS_INVALID_ARG && std::strstr(why, "flags"));
        v = def, v.reserved = f;
        CHECK(probe_tail_check(v, &why) == RAYS_INVALID_ARG && std::strstr(why, "reserved"));
    }
    for (uint32_t f = 0; f <= 15u; ++f) {
        ProbeTailCall v = def;
        v.flags = f;
        CHECK(probe_tail_check(v, &why) == RAYS_OK);
    }
    for (int b = 0; b < 3; ++b) {
        ProbeTailCall v = def;
        v.band_weight[b] = nan;
        CHECK(probe_tail_check(v, &why) == RAYS_INVALID_ARG && std::strstr(why, "band_weight"));
        v.band_weight[b] = -nan;
        CHECK(probe_tail_check(v, &why) == RAYS_INVALID_ARG);
        for (float w : {0.0f, -0.0f, -3.0f, 1e30f, inf, -inf}) {
            v.band_weight[b] = w;
            CHECK(probe_tail_check(v, &why) == RAYS_OK);
        }
    }
    for (float x : {nan, -nan, inf, -inf, -1.0f, -tiny}) {
        ProbeTailCall v = def;
        v.bias = x;
        CHECK(probe_tail_check(v, &why) == RAYS_INVALID_ARG && std::strstr(why, "bias"));
    }
    for (float x : {0.0f, -0.0f, tiny, 0.25f, 1e30f}) {
        ProbeTailCall v = def;
        v.bias = x;
        CHECK(probe_tail_check(v, &why) == RAYS_OK);
    }
    for (float x : {nan, -nan, inf, -inf, 0.0f, -0.0f, -1.0f, -tiny}) {
        ProbeTailCall v = def;
        v.min_variance = x;
        CHECK(probe_tail_check(v, &why) == RAYS_INVALID_ARG && std::strstr(why, "min_variance"));
    }
    for (float x : {tiny, 1e-4f, 1.0f, 1e30f}) {
        ProbeTailCall v = def;
        v.min_variance = x;
        CHECK(probe_tail_check(v, &why) == RAYS_OK);
    }

    // an accepted call takes effect; a refused one is never applied, so the previous setting stands; T1: max_bounces == 0 is unchanged
    {
        ProbeTailState t;
        ProbeTailCall v = def;
        v.flags = PROBE_TAIL_FLAG_DEPTH | PROBE_TAIL_FLAG_COUNT_WORK, v.bias = 0.5f;
        probe_tail_set(t, v);
        CHECK(t.enabled && t.call.flags == v.flags && t.call.bias == 0.5f);
        CHECK(probe_tail_applies(t, 1) && probe_tail_applies(t, 8) && !probe_tail_applies(t, 0) && !probe_tail_applies(t, -1));
        ProbeTailCall bad = def;
        bad.enabled = 0, bad.min_variance = nan;
        CHECK(probe_tail_check(bad, &why) == RAYS_INVALID_ARG && t.enabled && t.call.bias == 0.5f);
        // the work record: only of a trace that ran with the mode on and counted
        CHECK(t.last.work() == RAYS_STATE);
        CHECK(probe_tail_traced(t) && t.last.work() == RAYS_OK);
        v.flags = PROBE_TAIL_FLAG_DEPTH;
        probe_tail_set(t, v);
        CHECK(t.last.work() == RAYS_OK);  // (setting the mode is not a trace: the last trace's record stands)
        CHECK(!probe_tail_traced(t) && t.last.work() == RAYS_STATE);
        v.flags = PROBE_TAIL_FLAG_COUNT_WORK, v.enabled = 0;
        probe_tail_set(t, v);
        CHECK(!t.enabled && !probe_tail_applies(t, 8) && !probe_tail_traced(t) && t.last.work() == RAYS_STATE);
    }

    // the overlap predicate
    {
        alignas(16) static unsigned char buf[256];
        CHECK(probe_tail_ranges_overlap(buf, 64, buf, 64));
        CHECK(probe_tail_ranges_overlap(buf, 64, buf + 63, 1) && probe_tail_ranges_overlap(buf + 63, 1, buf, 64));
        CHECK(!probe_tail_ranges_overlap(buf, 64, buf + 64, 64) && !probe_tail_ranges_overlap(buf + 64, 64, buf, 64));  // adjacent
        CHECK(probe_tail_ranges_overlap(buf, 256, buf + 100, 8) && probe_tail_ranges_overlap(buf + 100, 8, buf, 256));  // contained
        CHECK(probe_tail_ranges_overlap(buf, 65, buf + 64, 64));
        CHECK(!probe_tail_ranges_overlap(buf, 0, buf, 64) && !probe_tail_ranges_overlap(buf, 64, buf, 0));              // empty
        CHECK(!probe_tail_ranges_overlap(nullptr, 64, buf, 64) && !probe_tail_ranges_overlap(buf, 64, nullptr, 64));    // absent
        // at the top of the address space: no sum of address and size is formed
        const void* top = (const void*)(UINTPTR_MAX - 15);
        CHECK(probe_tail_ranges_overlap(top, 16, top, 16) && probe_tail_ranges_overlap(top, 16, (const void*)(UINTPTR_MAX - 31), 32));
        CHECK(!probe_tail_ranges_overlap(top, 16, (const void*)(UINTPTR_MAX - 31), 16));
        CHECK(!probe_tail_ranges_overlap(buf, SIZE_MAX, buf, 0) && probe_tail_ranges_overlap(buf, SIZE_MAX, buf + 255, 1));
    }

    // what an affected trace requires, in the header's order
    {
        alignas(16) static unsigned char coeff[2 * 3 * 2 * 9 * 16], out[64];
        ProbeTailState t;
        ProbeTailCall v = def;
        v.flags = PROBE_TAIL_FLAG_DEPTH | PROBE_TAIL_FLAG_STATES;
        probe_tail_set(t, v);
        ProbeGridState g;
        ProbeGridDepthState d;
        ProbeStatesState st;
        auto check = [&](const void* written, size_t bytes) { return probe_tail_check_trace(t, g, d, st, coeff, written, bytes, &why); };
        CHECK(check(out, 64) == RAYS_STATE && std::strstr(why, "no grid"));
        g.grid_set = true, g.grid = ProbeGrid{{0, 0, 0}, {1, 1, 1}, {2, 3, 2}};
        CHECK(check(out, 64) == RAYS_STATE && std::strstr(why, "no coefficients"));
        g.coefficients.bound = coeff, g.coefficients.bound_count = 11;
        CHECK(check(out, 64) == RAYS_STATE && std::strstr(why, "coefficient count"));
        g.coefficients.bound_count = 12;
        CHECK(check(out, 64) == RAYS_STATE && std::strstr(why, "no depth maps"));
        d.moments.bound = coeff, d.moments.bound_count = 13, d.bound_resolution = 4;
        CHECK(check(out, 64) == RAYS_STATE && std::strstr(why, "depth probe count"));
        d.moments.bound_count = 12;
        CHECK(check(out, 64) == RAYS_STATE && std::strstr(why, "no states"));
        st.states.bound = coeff, st.states.bound_count = 1;
        CHECK(check(out, 64) == RAYS_STATE && std::strstr(why, "state count"));
        st.states.bound_count = 12;
        CHECK(check(out, 64) == RAYS_OK && check(nullptr, 64) == RAYS_OK && probe_tail_check_trace(t, g, d, st, coeff, out, 64, nullptr) == RAYS_OK);
        // the feedback loop: the array the tail reads is 12 probes x 9 float4
        CHECK(check(coeff, 16) == RAYS_STATE && std::strstr(why, "this call writes"));
        CHECK(check(coeff + sizeof coeff - 16, 4096) == RAYS_STATE && check(coeff + sizeof coeff, 4096) == RAYS_OK);
        // without the flags the maps and records are not asked for
        v.flags = 0;
        probe_tail_set(t, v);
        d = ProbeGridDepthState{}, st = ProbeStatesState{};
        CHECK(check(out, 64) == RAYS_OK);
    }

    if (failures) return 1;
    std::printf("ok probe tail host rules\n");
    return 0;
}
