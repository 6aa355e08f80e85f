// reflection_check.cpp — the host-side rules of the reflection guides (software-raytracer_amd/csrc/srt_reflection_host.h) as a
// stand-alone program: the header's constants and struct layouts, srt_render_reflection_gbuffer's checks in the header's order
// with their edges (max_bounces 0 / 64 / 65, NaN and +inf thresholds), the five slots with their element sizes, binding and the
// read rule, and when srt_get_reflection_work may report.  Built with
// -fsanitize=address,undefined and run on the CPU.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "srt_pathtrace.h"
#include "srt_reflection_host.h"

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
    // the header's constants and layouts are the ones the rules use
    CHECK(SRT_REFL_OBJECT == REFL_OUT_OBJECT && SRT_REFL_NORMAL_DEPTH == REFL_OUT_NORMAL_DEPTH && SRT_REFL_POSITION == REFL_OUT_POSITION);
    CHECK(SRT_REFL_ALBEDO == REFL_OUT_ALBEDO && SRT_REFL_BOUNCES == REFL_OUT_BOUNCES && SRT_REFL_GUIDES == REFL_OUT_GUIDES && SRT_REFL_ALL == REFL_OUT_ALL);
    CHECK(SRT_REFL_GUIDES == SRT_GBUF_ALL && SRT_REFL_OBJECT == SRT_GBUF_OBJECT && SRT_REFL_NORMAL_DEPTH == SRT_GBUF_NORMAL_DEPTH);
    CHECK(SRT_REFL_POSITION == SRT_GBUF_POSITION && SRT_REFL_ALBEDO == SRT_GBUF_ALBEDO);
    CHECK(SRT_REFL_COUNT_WORK == REFL_FLAG_COUNT_WORK && REFL_FLAG_ALL == 1u && REFL_MAX_BOUNCES == 64 && REFL_SLOTS == 5);
    CHECK(sizeof(srt_reflection_params) == 32 && sizeof(ReflectionCall) == 32);
    CHECK(offsetof(srt_reflection_params, row_begin) == 0 && offsetof(ReflectionCall, row_begin) == 0 && offsetof(srt_reflection_params, row_end) == 4 && offsetof(ReflectionCall, row_end) == 4);
    CHECK(offsetof(srt_reflection_params, outputs) == 8 && offsetof(ReflectionCall, outputs) == 8 && offsetof(srt_reflection_params, flags) == 12 && offsetof(ReflectionCall, flags) == 12);
    CHECK(offsetof(srt_reflection_params, max_bounces) == 16 && offsetof(ReflectionCall, max_bounces) == 16);
    CHECK(offsetof(srt_reflection_params, min_smoothness) == 20 && offsetof(ReflectionCall, min_smoothness) == 20);
    CHECK(offsetof(srt_reflection_params, min_specular) == 24 && offsetof(ReflectionCall, min_specular) == 24);
    CHECK(offsetof(srt_reflection_params, reserved) == 28 && offsetof(ReflectionCall, reserved) == 28);
    CHECK(sizeof(srt_reflection_work) == 40 && offsetof(srt_reflection_work, valid) == 0 && offsetof(srt_reflection_work, reserved) == 4);
    CHECK(offsetof(srt_reflection_work, pixels) == 8 && offsetof(srt_reflection_work, reflections) == 16);
    CHECK(offsetof(srt_reflection_work, wave_calls) == 24 && offsetof(srt_reflection_work, waves) == 32);
    // slots and element sizes: the SRT_GBUF_* element types, int32 for BOUNCES
    CHECK(reflection_slot(1) == 0 && reflection_slot(2) == 1 && reflection_slot(4) == 2 && reflection_slot(8) == 3 && reflection_slot(16) == 4);
    for (uint32_t o : {0u, 3u, 5u, 15u, 17u, 31u, 32u, 0x80000000u, ~0u}) CHECK(reflection_slot(o) == -1);
    CHECK(reflection_elem_bytes(0) == 4 && reflection_elem_bytes(1) == 16 && reflection_elem_bytes(2) == 16 && reflection_elem_bytes(3) == 16 && reflection_elem_bytes(4) == 4);

    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int H = 20;
    const char* why = nullptr;

    // the defaults
    const ReflectionCall def = reflection_defaults();
    CHECK(def.row_begin == 0 && def.row_end == 0 && def.outputs == 31u && def.flags == 0 && def.max_bounces == 8 && def.min_smoothness == 1.0f &&
          def.min_specular == 1.0f && def.reserved == 0);
    CHECK(reflection_check(def, true, true, H, &why) == RAYS_INVALID_ARG && std::strstr(why, "band"));  // the band is the caller's
    ReflectionCall good = def;
    good.row_end = H;
    CHECK(reflection_check(good, true, true, H, &why) == RAYS_OK);
    CHECK(reflection_check(good, true, true, H, nullptr) == RAYS_OK);  // (a NULL reason is allowed)

    // the order: scene, camera, band, outputs, flags, reserved, max_bounces, min_smoothness, min_specular — each error hides the later ones
    {
        ReflectionCall v = good;
        v.row_end = H + 1, v.outputs = 0, v.flags = 2, v.reserved = 1, v.max_bounces = 65, v.min_smoothness = nan, v.min_specular = nan;
        CHECK(reflection_check(v, false, false, H, &why) == RAYS_STATE && std::strstr(why, "srt_set_scene"));
        CHECK(reflection_check(v, false, true, H, &why) == RAYS_STATE && std::strstr(why, "srt_set_scene"));
        CHECK(reflection_check(v, true, false, H, &why) == RAYS_STATE && std::strstr(why, "srt_set_camera"));
        CHECK(reflection_check(v, true, true, H, &why) == RAYS_INVALID_ARG && std::strstr(why, "band"));
        v.row_end = H;
        CHECK(reflection_check(v, true, true, H, &why) == RAYS_INVALID_ARG && std::strstr(why, "outputs"));
        v.outputs = 32u | 1u;
        CHECK(reflection_check(v, true, true, H, &why) == RAYS_INVALID_ARG && std::strstr(why, "outputs"));
        v.outputs = REFL_OUT_BOUNCES;
        CHECK(reflection_check(v, true, true, H, &why) == RAYS_INVALID_ARG && std::strstr(why, "flags"));
        v.flags = REFL_FLAG_COUNT_WORK;
        CHECK(reflection_check(v, true, true, H, &why) == RAYS_INVALID_ARG && std::strstr(why, "reserved"));
        v.reserved = 0;
        CHECK(reflection_check(v, true, true, H, &why) == RAYS_INVALID_ARG && std::strstr(why, "max_bounces"));
        v.max_bounces = 64;
        CHECK(reflection_check(v, true, true, H, &why) == RAYS_INVALID_ARG && std::strstr(why, "min_smoothness"));
        v.min_smoothness = inf;
        CHECK(reflection_check(v, true, true, H, &why) == RAYS_INVALID_ARG && std::strstr(why, "min_specular"));
        v.min_specular = -inf;
        CHECK(reflection_check(v, true, true, H, &why) == RAYS_OK);
        // a good call before the scene or the camera is still a state error
        CHECK(reflection_check(v, false, true, H, &why) == RAYS_STATE && reflection_check(v, true, false, H, &why) == RAYS_STATE);
    }
    // bands
    for (int rb = -1; rb <= H + 1; ++rb)
        for (int re = -1; re <= H + 1; ++re) {
            ReflectionCall v = good;
            v.row_begin = rb, v.row_end = re;
            const bool ok = rb >= 0 && re <= H && rb < re;
            CHECK(reflection_check(v, true, true, H, &why) == (ok ? RAYS_OK : RAYS_INVALID_ARG));
            if (!ok) CHECK(std::strstr(why, "band") != nullptr);
        }
    // every non-empty set of the five bits, both flags; anything else is refused
    for (uint32_t o = 1; o <= 31u; ++o)
        for (uint32_t f : {0u, 1u}) {
            ReflectionCall v = good;
            v.outputs = o, v.flags = f;
            CHECK(reflection_check(v, true, true, H, &why) == RAYS_OK);
        }
    for (uint32_t o : {0u, 32u, 33u, 63u, 0x80000001u, ~0u}) {
        ReflectionCall v = good;
        v.outputs = o;
        CHECK(reflection_check(v, true, true, H, &why) == RAYS_INVALID_ARG && std::strstr(why, "outputs"));
    }
    for (uint32_t f : {2u, 3u, 4u, 0x80000000u, ~0u}) {
        ReflectionCall v = good;
        v.flags = f;
        CHECK(reflection_check(v, true, true, H, &why) == RAYS_INVALID_ARG && std::strstr(why, "flags"));
    }
    for (uint32_t r : {1u, 2u, 0x80000000u, ~0u}) {
        ReflectionCall v = good;
        v.reserved = r;
        CHECK(reflection_check(v, true, true, H, &why) == RAYS_INVALID_ARG && std::strstr(why, "reserved"));
    }
    // max_bounces: 0 .. 64
    for (int b : {0, 1, 8, 63, 64}) {
        ReflectionCall v = good;
        v.max_bounces = b;
        CHECK(reflection_check(v, true, true, H, &why) == RAYS_OK);
    }
    for (int b : {-1, 65, 66, std::numeric_limits<int>::max(), std::numeric_limits<int>::min()}) {
        ReflectionCall v = good;
        v.max_bounces = b;
        CHECK(reflection_check(v, true, true, H, &why) == RAYS_INVALID_ARG && std::strstr(why, "max_bounces"));
    }
    // thresholds: anything but a NaN, either sign of it
    for (float t : {0.0f, -0.0f, -1.0f, 0.7f, 1.0f, 1e30f, inf, -inf, std::numeric_limits<float>::denorm_min()}) {
        ReflectionCall v = good;
        v.min_smoothness = t;
        CHECK(reflection_check(v, true, true, H, &why) == RAYS_OK);
        v = good, v.min_specular = t;
        CHECK(reflection_check(v, true, true, H, &why) == RAYS_OK);
    }
    for (float t : {nan, -nan}) {
        ReflectionCall v = good;
        v.min_smoothness = t;
        CHECK(reflection_check(v, true, true, H, &why) == RAYS_INVALID_ARG && std::strstr(why, "min_smoothness"));
        v = good, v.min_specular = t;
        CHECK(reflection_check(v, true, true, H, &why) == RAYS_INVALID_ARG && std::strstr(why, "min_specular"));
    }

    // slots, binding, the read rule and the record of the last call
    ReflectionSlots slots;
    CallRecord s;
    const void* src = nullptr;
    int own_obj, own_nd, own_pos, own_alb, own_j, mine;
    const void* none[REFL_SLOTS] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    for (uint32_t o : {1u, 2u, 4u, 8u, 16u}) CHECK(reflection_check_read(slots, o, none, &src) == RAYS_STATE);  // neither bound nor rendered
    for (uint32_t o : {0u, 3u, 31u, 32u}) CHECK(reflection_check_read(slots, o, none, &src) == RAYS_INVALID_ARG);
    CHECK(s.work() == RAYS_STATE);  // no call yet
    // a bound buffer is readable at once (srt_read_gbuffer's rule), the others still are not
    slots.out[3].bind(&mine);
    CHECK(reflection_check_read(slots, REFL_OUT_ALBEDO, none, &src) == RAYS_OK && src == &mine);
    CHECK(reflection_check_read(slots, REFL_OUT_OBJECT, none, &src) == RAYS_STATE);
    // the first call: OBJECT and BOUNCES into own buffers, ALBEDO into the bound one, not counted
    {
        const void* own[REFL_SLOTS] = {&own_obj, nullptr, nullptr, nullptr, &own_j};
        CHECK(slots.out[0].target(0, 100).own && slots.out[0].target(0, 100).grow && !slots.out[3].target(0, 100).own && !slots.out[3].target(0, 100).grow);
        void* dst[REFL_SLOTS] = {&own_obj, nullptr, nullptr, &mine, &own_j};
        reflection_rendered(s, slots, REFL_OUT_OBJECT | REFL_OUT_ALBEDO | REFL_OUT_BOUNCES, dst, 0);
        CHECK(s.ran && !s.counted && s.work() == RAYS_STATE);
        CHECK(reflection_check_read(slots, REFL_OUT_OBJECT, own, &src) == RAYS_OK && src == &own_obj);
        CHECK(reflection_check_read(slots, REFL_OUT_BOUNCES, own, &src) == RAYS_OK && src == &own_j);
        CHECK(reflection_check_read(slots, REFL_OUT_ALBEDO, own, &src) == RAYS_OK && src == &mine);
        CHECK(reflection_check_read(slots, REFL_OUT_NORMAL_DEPTH, own, &src) == RAYS_STATE && reflection_check_read(slots, REFL_OUT_POSITION, own, &src) == RAYS_STATE);
        CHECK(slots.out[0].written && slots.out[0].last == &own_obj && !slots.out[1].written && slots.out[3].last == &mine);
        CHECK(!slots.out[0].target(100, 100).grow && slots.out[0].target(100, 101).grow);
    }
    // a counting call of all five; unbinding ALBEDO returns to the own buffer
    {
        const void* own[REFL_SLOTS] = {&own_obj, &own_nd, &own_pos, &own_alb, &own_j};
        void* dst[REFL_SLOTS] = {&own_obj, &own_nd, &own_pos, &mine, &own_j};
        reflection_rendered(s, slots, REFL_OUT_ALL, dst, REFL_FLAG_COUNT_WORK);
        CHECK(s.counted && s.work() == RAYS_OK);
        CHECK(reflection_check_read(slots, REFL_OUT_ALBEDO, own, &src) == RAYS_OK && src == &mine);
        slots.out[3].bind(nullptr);
        CHECK(reflection_check_read(slots, REFL_OUT_ALBEDO, own, &src) == RAYS_OK && src == &own_alb);
        CHECK(reflection_check_read(slots, REFL_OUT_NORMAL_DEPTH, own, &src) == RAYS_OK && src == &own_nd);
        // a refused check in between changes nothing
        ReflectionCall v = good;
        v.max_bounces = 65;
        CHECK(reflection_check(v, true, true, H, &why) == RAYS_INVALID_ARG && s.ran && s.counted && s.work() == RAYS_OK);
        // a call without the flag ends the record
        void* one[REFL_SLOTS] = {nullptr, nullptr, nullptr, nullptr, &own_j};
        reflection_rendered(s, slots, REFL_OUT_BOUNCES, one, 0);
        CHECK(s.ran && !s.counted && s.work() == RAYS_STATE);
        CHECK(slots.out[0].last == &own_obj);  // an output not asked for keeps its record
    }

    if (failures) return 1;
    std::printf("ok reflection host rules\n");
    return 0;
}
