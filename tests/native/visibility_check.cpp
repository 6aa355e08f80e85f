// visibility_check.cpp — the host-side rules of the per-pixel visibility pass (software-raytracer_amd/csrc/srt_visibility_host.h)
// as a stand-alone program: the header's constants and struct layouts, srt_render_visibility's checks in the header's order
// (the scene, the arguments, the guides), the record of which outputs the last call wrote to which buffers, and when
// srt_get_visibility_work may report.  Built with -fsanitize=address,undefined and run on the CPU.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "srt_pathtrace.h"
#include "srt_visibility_host.h"

using namespace srt;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

// srt_read_visibility's rule as srt_capi.hip composes it: the slot, then the shared record's read
static RaysStatus read_visibility(const VisibilityState& s, uint32_t output, const void** src) {
    const int i = visibility_slot(output);
    if (i < 0) return RAYS_INVALID_ARG;
    return (*src = s.last.read(output, i)) ? RAYS_OK : RAYS_STATE;
}

static bool same(const VisibilityState& a, const VisibilityState& b) {
    return a.call.ran == b.call.ran && a.call.counted == b.call.counted && a.last.outputs == b.last.outputs && a.last.dst[0] == b.last.dst[0] && a.last.dst[1] == b.last.dst[1];
}

int main() {
    // the header's constants and layouts are the ones the rules use
    CHECK(SRT_VIS_AO == VIS_OUT_AO && SRT_VIS_SUN == VIS_OUT_SUN && (SRT_VIS_AO | SRT_VIS_SUN) == VIS_OUT_ALL);
    CHECK(SRT_VIS_COUNT_WORK == VIS_FLAG_COUNT_WORK && VIS_FLAG_ALL == 1u);
    CHECK(sizeof(srt_visibility_params) == 32 && sizeof(VisibilityCall) == 32);
    CHECK(offsetof(srt_visibility_params, row_begin) == offsetof(VisibilityCall, row_begin) && offsetof(srt_visibility_params, row_end) == offsetof(VisibilityCall, row_end));
    CHECK(offsetof(srt_visibility_params, outputs) == 8 && offsetof(VisibilityCall, outputs) == 8 && offsetof(srt_visibility_params, flags) == 12 && offsetof(VisibilityCall, flags) == 12);
    CHECK(offsetof(srt_visibility_params, ao_samples) == 16 && offsetof(VisibilityCall, ao_samples) == 16);
    CHECK(offsetof(srt_visibility_params, first_sample) == 20 && offsetof(VisibilityCall, first_sample) == 20);
    CHECK(offsetof(srt_visibility_params, seed) == 24 && offsetof(VisibilityCall, seed) == 24 && offsetof(srt_visibility_params, ao_radius) == 28 && offsetof(VisibilityCall, ao_radius) == 28);
    CHECK(sizeof(srt_visibility_work) == 56 && offsetof(srt_visibility_work, valid) == 0 && offsetof(srt_visibility_work, reserved) == 4);
    CHECK(offsetof(srt_visibility_work, segments) == 8 && offsetof(srt_visibility_work, open) == 16 && offsetof(srt_visibility_work, wave_trips) == 24);
    CHECK(offsetof(srt_visibility_work, analytic_tests) == 32 && offsetof(srt_visibility_work, node_visits) == 40 && offsetof(srt_visibility_work, triangle_tests) == 48);
    CHECK(visibility_slot(SRT_VIS_AO) == 0 && visibility_slot(SRT_VIS_SUN) == 1);
    for (uint32_t o : {0u, 3u, 4u, 8u, 0x80000000u, ~0u}) CHECK(visibility_slot(o) == -1);

    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const VisibilityCall good{0, 20, VIS_OUT_ALL, 0, 16, 1, 0, inf};
    const bool all[VIS_GUIDES] = {true, true, true}, none[VIS_GUIDES] = {false, false, false};
    const char* why = nullptr;
    const int H = 20;

    // the checks in their order: the scene, the arguments, the guides
    CHECK(visibility_check(good, true, H, all, &why) == RAYS_OK);
    CHECK(visibility_check(good, true, H, all, nullptr) == RAYS_OK);  // (a NULL reason is allowed)
    CHECK(visibility_check(good, false, H, all, &why) == RAYS_STATE && std::strstr(why, "srt_set_scene"));
    {
        VisibilityCall v = good;
        v.outputs = 0, v.row_end = 21;
        CHECK(visibility_check(v, false, H, none, &why) == RAYS_STATE && std::strstr(why, "srt_set_scene"));  // the scene comes first
        CHECK(visibility_check(v, true, H, none, &why) == RAYS_INVALID_ARG && std::strstr(why, "band"));     // the arguments before the guides
        v.row_end = 20;
        CHECK(visibility_check(v, true, H, none, &why) == RAYS_INVALID_ARG && std::strstr(why, "outputs"));
        v.outputs = VIS_OUT_SUN;
        CHECK(visibility_check(v, true, H, none, &why) == RAYS_STATE && std::strstr(why, "OBJECT"));
    }
    // bands
    for (int rb = -1; rb <= H + 1; ++rb)
        for (int re = -1; re <= H + 1; ++re) {
            VisibilityCall v = good;
            v.row_begin = rb, v.row_end = re;
            const bool ok = rb >= 0 && re <= H && rb < re;
            CHECK(visibility_check(v, true, H, all, &why) == (ok ? RAYS_OK : RAYS_INVALID_ARG));
            if (!ok) CHECK(std::strstr(why, "band") != nullptr);
        }
    // outputs and flags
    for (uint32_t o : {1u, 2u, 3u}) {
        VisibilityCall v = good;
        v.outputs = o;
        for (uint32_t f : {0u, 1u}) {
            v.flags = f;
            CHECK(visibility_check(v, true, H, all, &why) == RAYS_OK);
        }
        for (uint32_t f : {2u, 3u, 4u, 0x80000000u, ~0u}) {
            v.flags = f;
            CHECK(visibility_check(v, true, H, all, &why) == RAYS_INVALID_ARG && std::strstr(why, "flags"));
        }
    }
    for (uint32_t o : {0u, 4u, 5u, 7u, 0x80000001u, ~0u}) {
        VisibilityCall v = good;
        v.outputs = o;
        CHECK(visibility_check(v, true, H, all, &why) == RAYS_INVALID_ARG && std::strstr(why, "outputs"));
    }
    // the AO arguments: read with SRT_VIS_AO only
    struct Bad {
        uint32_t n, f0;
        float r;
        const char* word;
    };
    const Bad bad[] = {{0, 1, inf, "ao_samples"},          {4097, 1, inf, "ao_samples"},      {~0u, 1, inf, "ao_samples"},     {16, 0, inf, "first_sample"},
                       {2, 0xFFFFFFFFu, inf, "2^32"},      {4096, 0xFFFFF001u, inf, "2^32"},  {16, 1, nan, "ao_radius"},       {16, 1, 0.0f, "ao_radius"},
                       {16, 1, -0.0f, "ao_radius"},        {16, 1, -1.0f, "ao_radius"},       {16, 1, -inf, "ao_radius"}};
    for (const Bad& b : bad) {
        VisibilityCall v = good;
        v.ao_samples = b.n, v.first_sample = b.f0, v.ao_radius = b.r;
        for (uint32_t o : {1u, 3u}) {
            v.outputs = o;
            CHECK(visibility_check(v, true, H, all, &why) == RAYS_INVALID_ARG && std::strstr(why, b.word));
        }
        v.outputs = VIS_OUT_SUN;
        CHECK(visibility_check(v, true, H, all, &why) == RAYS_OK);
    }
    {
        VisibilityCall v = good;
        v.ao_samples = 1, v.first_sample = 0xFFFFFFFFu, v.ao_radius = 1e-30f;
        CHECK(visibility_check(v, true, H, all, &why) == RAYS_OK);
        v.ao_samples = 4096, v.first_sample = 0xFFFFF000u;
        CHECK(visibility_check(v, true, H, all, &why) == RAYS_OK);
    }
    // the guides, each on its own and in slot order
    static const char* const names[VIS_GUIDES] = {"OBJECT", "NORMAL_DEPTH", "POSITION"};
    for (int m = 0; m < 7; ++m) {
        const bool g[VIS_GUIDES] = {(m & 1) != 0, (m & 2) != 0, (m & 4) != 0};
        int first = 0;
        while (g[first]) ++first;
        CHECK(visibility_check(good, true, H, g, &why) == RAYS_STATE && std::strstr(why, names[first]) == why + 4);
    }

    // the record of the last call
    VisibilityState s;
    const void* src = nullptr;
    float ao_buf, sun_buf, other;
    CHECK(read_visibility(s, SRT_VIS_AO, &src) == RAYS_STATE && read_visibility(s, SRT_VIS_SUN, &src) == RAYS_STATE);
    CHECK(read_visibility(s, 3, &src) == RAYS_INVALID_ARG && read_visibility(s, 0, &src) == RAYS_INVALID_ARG);
    CHECK(s.call.work() == RAYS_STATE);  // no call yet
    void* both[VIS_SLOTS] = {&ao_buf, &sun_buf};
    visibility_rendered(s, VIS_OUT_ALL, both, 0);
    CHECK(read_visibility(s, SRT_VIS_AO, &src) == RAYS_OK && src == &ao_buf);
    CHECK(read_visibility(s, SRT_VIS_SUN, &src) == RAYS_OK && src == &sun_buf);
    CHECK(s.call.work() == RAYS_STATE);  // rendered, but not counted
    // a refused check in between changes nothing
    {
        const VisibilityState before = s;
        VisibilityCall v = good;
        v.flags = 2;
        CHECK(visibility_check(v, true, H, all, &why) == RAYS_INVALID_ARG && same(s, before));
    }
    // AO alone, to another buffer: SUN is no longer readable, and the slot of an output not asked for is not recorded
    void* moved[VIS_SLOTS] = {&other, &sun_buf};
    visibility_rendered(s, VIS_OUT_AO, moved, VIS_FLAG_COUNT_WORK);
    CHECK(read_visibility(s, SRT_VIS_AO, &src) == RAYS_OK && src == &other);
    CHECK(read_visibility(s, SRT_VIS_SUN, &src) == RAYS_STATE && s.last.dst[1] == nullptr);
    CHECK(s.call.work() == RAYS_OK);
    void* sun_only[VIS_SLOTS] = {nullptr, &sun_buf};
    visibility_rendered(s, VIS_OUT_SUN, sun_only, 0);  // a call without the flag ends the record
    CHECK(read_visibility(s, SRT_VIS_SUN, &src) == RAYS_OK && src == &sun_buf && read_visibility(s, SRT_VIS_AO, &src) == RAYS_STATE);
    CHECK(s.call.work() == RAYS_STATE);

    if (failures) return 1;
    std::printf("ok visibility host rules\n");
    return 0;
}
