// adaptive_check.cpp — the host-side rules of adaptive sampling (software-raytracer_amd/csrc/srt_adaptive_host.h) as a stand-alone
// program: the header's constants and struct layouts, the defaults, the effective budget at its edges (the cap, the last frame),
// srt_render_adaptive's and srt_sample_budget's checks in their order — every refusal the header lists — the budget of one pixel
// by hand (equality with T, the cap, a T that underflows, NaN and infinities), when srt_get_adaptive_work and
// srt_get_budget_total may report, the count and budget slots' "present" rule, the grid for a few bands and a sample scratch that
// depends on the grid alone.  Built with -fsanitize=address,undefined and run on the CPU.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <limits>
#include <vector>

#include "srt_pathtrace.h"
#include "srt_adaptive_host.h"

using namespace srt;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static AdaptiveCall acall(int rb, int re, int bounces, uint32_t max_samples, uint32_t flags, uint32_t reserved = 0) {
    return AdaptiveCall{rb, re, bounces, 0u, max_samples, flags, reserved};
}

int main() {
    // the header's constants and layouts are the ones the rules use
    CHECK(SRT_ADAPTIVE_KEEP_COUNTS == ADAPTIVE_FLAG_KEEP_COUNTS && SRT_ADAPTIVE_COUNT_WORK == ADAPTIVE_FLAG_COUNT_WORK &&
          (SRT_ADAPTIVE_KEEP_COUNTS | SRT_ADAPTIVE_COUNT_WORK) == ADAPTIVE_FLAG_ALL && SRT_BUDGET_ALBEDO == BUDGET_FLAG_ALBEDO && BUDGET_FLAG_ALL == 1u);
    CHECK(sizeof(srt_adaptive_params) == 28 && sizeof(AdaptiveCall) == 28 && offsetof(srt_adaptive_params, row_begin) == 0 &&
          offsetof(srt_adaptive_params, row_end) == 4 && offsetof(srt_adaptive_params, max_bounces) == 8 && offsetof(srt_adaptive_params, seed) == 12 &&
          offsetof(srt_adaptive_params, max_samples) == 16 && offsetof(srt_adaptive_params, flags) == 20 && offsetof(srt_adaptive_params, reserved) == 24);
    CHECK(offsetof(AdaptiveCall, max_bounces) == 8 && offsetof(AdaptiveCall, seed) == 12 && offsetof(AdaptiveCall, max_samples) == 16 &&
          offsetof(AdaptiveCall, flags) == 20 && offsetof(AdaptiveCall, reserved) == 24);
    CHECK(sizeof(srt_budget_params) == 16 && sizeof(BudgetCall) == 16 && offsetof(srt_budget_params, threshold) == 0 && offsetof(srt_budget_params, floor) == 4 &&
          offsetof(srt_budget_params, max_budget) == 8 && offsetof(srt_budget_params, flags) == 12);
    CHECK(sizeof(srt_adaptive_work) == 40 && offsetof(srt_adaptive_work, pixels) == 8 && offsetof(srt_adaptive_work, samples) == 16 &&
          offsetof(srt_adaptive_work, closest_calls) == 24 && offsetof(srt_adaptive_work, wave_calls) == 32);
    {
        AdaptiveCall d = acall(5, 6, -9, 9, ~0u, 9);
        d.seed = 9;
        adaptive_call_default(d);
        CHECK(d.row_begin == 0 && d.row_end == 0 && d.max_bounces == 8 && d.seed == 0 && d.max_samples == 4096 && d.flags == 0 && d.reserved == 0);
        BudgetCall b{0, 0, 0, ~0u};
        budget_call_default(b);
        CHECK(b.threshold == 0.05f && b.floor == 0.01f && b.max_budget == 64 && b.flags == BUDGET_FLAG_ALBEDO);
    }

    // rule 1: the effective budget
    CHECK(adaptive_effective(0, 3, 4096) == 0 && adaptive_effective(5, 0, 4096) == 5 && adaptive_effective(5000, 0, 4096) == 4096);
    CHECK(adaptive_effective(100, 0, 9) == 9 && adaptive_effective(0xFFFFFFFFu, 7, 4096) == 4096);
    CHECK(adaptive_effective(5, 2147483644u, 4096) == 2 && adaptive_effective(5, 2147483645u, 4096) == 1);
    CHECK(adaptive_effective(5, 2147483646u, 4096) == 0 && adaptive_effective(5, 2147483647u, 4096) == 0 && adaptive_effective(5, 0xFFFFFFFFu, 4096) == 0);

    // srt_render_adaptive's checks: scene and camera, the arguments, the buffers
    const char* why = nullptr;
    const AdaptiveCall ok = acall(0, 20, 8, 4096, 0);
    CHECK(adaptive_check(ok, false, true, 20, true, true, &why) == RAYS_STATE && why);
    CHECK(adaptive_check(ok, true, false, 20, true, true, &why) == RAYS_STATE);
    CHECK(adaptive_check(acall(0, 20, -1, 0, 4), false, false, 20, false, false, nullptr) == RAYS_STATE);  // (the state first, and why may be NULL)
    CHECK(adaptive_check(ok, true, true, 20, true, true, &why) == RAYS_OK);
    CHECK(adaptive_check(acall(4, 12, 0, 1, 3), true, true, 20, true, true, &why) == RAYS_OK);
    for (const AdaptiveCall& c : {acall(0, 0, 8, 64, 0), acall(5, 5, 8, 64, 0), acall(6, 5, 8, 64, 0), acall(-1, 20, 8, 64, 0), acall(0, 21, 8, 64, 0),
                                  acall(0, 20, 8, 64, 4), acall(0, 20, 8, 64, ~0u), acall(0, 20, 8, 64, 0, 1), acall(0, 20, 8, 0, 0), acall(0, 20, 8, 4097, 0),
                                  acall(0, 20, -1, 64, 0)}) {
        CHECK(adaptive_check(c, true, true, 20, true, true, &why) == RAYS_INVALID_ARG);
        CHECK(adaptive_check(c, true, true, 20, false, false, &why) == RAYS_INVALID_ARG);  // the arguments before the buffers
    }
    CHECK(adaptive_check(ok, true, true, 20, false, true, &why) == RAYS_STATE);
    CHECK(adaptive_check(ok, true, true, 20, true, false, &why) == RAYS_STATE);

    // srt_sample_budget's checks: the arguments, then the inputs
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const BudgetCall bok{0.05f, 0.01f, 64, BUDGET_FLAG_ALBEDO};
    CHECK(budget_check(bok, true, true, true, true, true, true, &why) == RAYS_OK);
    CHECK(budget_check(BudgetCall{inf, 0.0f, 1, 0}, true, false, true, true, false, true, &why) == RAYS_OK);  // +inf allowed; no ALBEDO guide needed
    CHECK(budget_check(BudgetCall{0.05f, inf, 4096, 0}, true, false, true, false, true, true, &why) == RAYS_OK);  // a bound variance is the caller's
    for (const BudgetCall& c : {BudgetCall{0.0f, 0.01f, 64, 0}, BudgetCall{-1.0f, 0.01f, 64, 0}, BudgetCall{nan, 0.01f, 64, 0}, BudgetCall{0.05f, -0.5f, 64, 0},
                                BudgetCall{0.05f, nan, 64, 0}, BudgetCall{0.05f, 0.01f, 0, 0}, BudgetCall{0.05f, 0.01f, 4097, 0}, BudgetCall{0.05f, 0.01f, 64, 2}}) {
        CHECK(budget_check(c, true, true, true, true, false, true, &why) == RAYS_INVALID_ARG);
        CHECK(budget_check(c, false, false, false, true, false, false, &why) == RAYS_INVALID_ARG);  // the arguments before the inputs
    }
    CHECK(budget_check(bok, false, true, true, true, true, true, &why) == RAYS_STATE);   // no OBJECT guide
    CHECK(budget_check(bok, true, false, true, true, true, true, &why) == RAYS_STATE);   // no ALBEDO guide, with the flag
    CHECK(budget_check(bok, true, true, false, true, true, true, &why) == RAYS_STATE);   // no variance
    CHECK(budget_check(bok, true, true, true, true, false, true, &why) == RAYS_STATE);   // an own variance without ALBEDO, the call with
    CHECK(budget_check(BudgetCall{0.05f, 0.01f, 64, 0}, true, true, true, true, true, true, &why) == RAYS_STATE);  // ... and the other way round
    CHECK(budget_check(bok, true, true, true, false, false, true, &why) == RAYS_OK);     // a bound one is not checked
    CHECK(budget_check(bok, true, true, true, true, true, false, &why) == RAYS_STATE);   // no counts

    // rules 3-4 for one pixel: threshold 0.5, floor 0, l = 1 -> T = 0.25
    const BudgetCall half{0.5f, 0.0f, 64, 0};
    CHECK(budget_value(1.0f, 1.0f, 4, half) == 12);                                   // r = 4, e = 4 * 4 - 4
    CHECK(budget_value(0.25f, 1.0f, 4, half) == 0);                                   // g == T
    CHECK(budget_value(std::nextafter(0.25f, 1.0f), 1.0f, 4, half) == 1);             // max(1, ceil(4 * 2^-23))
    CHECK(budget_value(1.0f, 1.0f, 1, half) == 3 && budget_value(0.0f, 1.0f, 4, half) == 0);
    CHECK(budget_value(inf, 1.0f, 4, half) == 64 && budget_value(nan, 1.0f, 4, half) == 0 && budget_value(1.0f, nan, 4, half) == 0);
    CHECK(budget_value(1.0f, 1.0f, 4, BudgetCall{0.5f, 0.0f, 12, 0}) == 12 && budget_value(1.0f, 1.0f, 4, BudgetCall{0.5f, 0.0f, 11, 0}) == 11);
    CHECK(budget_value(1.0f, 1.0f, 4, BudgetCall{0.5f, 1.0f, 64, 0}) == 0);           // the floor: T = 1
    CHECK(budget_value(1e-30f, 1.0f, 4, BudgetCall{1e-30f, 0.0f, 77, 0}) == 77);      // T underflows to 0: r = +inf
    CHECK(budget_value(1e30f, 1.0f, 4, BudgetCall{inf, 0.0f, 77, 0}) == 0 && budget_value(inf, 1.0f, 4, BudgetCall{inf, 0.0f, 77, 0}) == 0);
    CHECK(budget_value(0.5f, 1.0f, 0x80000000u, BudgetCall{0.5f, 0.0f, 4096, 0}) == 4096);

    // what may report
    AdaptiveState st;
    CHECK(st.call.work() == RAYS_STATE && budget_check_total(st) == RAYS_STATE);
    adaptive_rendered(st, 0);
    CHECK(st.call.work() == RAYS_STATE);
    adaptive_rendered(st, ADAPTIVE_FLAG_COUNT_WORK | ADAPTIVE_FLAG_KEEP_COUNTS);
    CHECK(st.call.work() == RAYS_OK && budget_check_total(st) == RAYS_STATE);
    adaptive_rendered(st, ADAPTIVE_FLAG_KEEP_COUNTS);
    CHECK(st.call.work() == RAYS_STATE);
    st.budgeted = true;
    CHECK(budget_check_total(st) == RAYS_OK);

    // the slots: present once bound, or once the own buffer exists (it is allocated by its first write or fill)
    {
        std::vector<uint32_t> own(4), mine(4);
        OutputSlot s;
        CHECK(s.current(nullptr) == nullptr);
        CHECK(s.target(0, 16).own && s.target(0, 16).grow);
        s.wrote(own.data());
        CHECK(s.current(own.data()) == own.data() && !s.target(16, 16).grow);
        s.bind(mine.data());
        CHECK(s.current(own.data()) == mine.data() && !s.target(16, 16).own);
        s.bind(nullptr);
        CHECK(s.current(own.data()) == own.data());
        OutputSlot b;
        b.bind(mine.data());
        CHECK(b.current(nullptr) == mine.data());  // bound and never written: present
    }

    // the grid: one workgroup per four tiles, at most the resident ones, never none; the scratch follows the grid
    CHECK(adaptive_grid(24, 20, 4, 1024) == 3 && adaptive_grid(21, 13, 4, 1024) == 2 && adaptive_grid(64, 64, 4, 1024) == 16);
    CHECK(adaptive_grid(8, 8, 4, 1024) == 1 && adaptive_grid(1, 1, 4, 0) == 1 && adaptive_grid(1920, 1080, 4, 1024) == 1024);
    CHECK(adaptive_scratch_bytes(1, 4) == 4u * 64 * 64 * 16 && adaptive_scratch_bytes(1024, 4) == radiance_scratch_bytes(1024, 4));

    if (failures) return 1;
    std::printf("ok adaptive host rules\n");
    return 0;
}
