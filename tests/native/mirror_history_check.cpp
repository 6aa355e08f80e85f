// mirror_history_check.cpp — the host-side rules of the mirror history (software-raytracer_amd/csrc/srt_mirror_history_host.h) as
// a stand-alone program: the header's struct layout, every refusal of srt_mirror_history with its edges (enabled -1 / 2, a zero,
// negative, NaN and +inf radius, flags, reserved), the rule "toggling drops the history, the radius alone does not", rho against
// a long-double evaluation, and the tags.  Built with -fsanitize=address,undefined and run on the CPU.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "srt_mirror_history_host.h"
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
    CHECK(sizeof(srt_mirror_history_params) == 16 && sizeof(MirrorHistoryCall) == 16);
    CHECK(offsetof(srt_mirror_history_params, enabled) == 0 && offsetof(MirrorHistoryCall, enabled) == 0);
    CHECK(offsetof(srt_mirror_history_params, radius_pixels) == 4 && offsetof(MirrorHistoryCall, radius_pixels) == 4);
    CHECK(offsetof(srt_mirror_history_params, flags) == 8 && offsetof(MirrorHistoryCall, flags) == 8);
    CHECK(offsetof(srt_mirror_history_params, reserved) == 12 && offsetof(MirrorHistoryCall, reserved) == 12);
    CHECK(MIRROR_TAG_SHIFT == 32768 && MIRROR_MAX_BOUNCES == 64);

    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const char* why = nullptr;

    // the defaults, and the state before any call
    const MirrorHistoryCall def = mirror_history_defaults();
    CHECK(def.enabled == 1 && def.radius_pixels == 2.0f && def.flags == 0 && def.reserved == 0);
    CHECK(mirror_history_check(def, &why) == RAYS_OK && mirror_history_check(def, nullptr) == RAYS_OK);
    MirrorHistoryState s;
    CHECK(!s.enabled && s.radius_pixels == 2.0f);

    // every refusal, in the struct's order: each error hides the later ones
    {
        MirrorHistoryCall v{2, nan, 1u, 1u};
        CHECK(mirror_history_check(v, &why) == RAYS_INVALID_ARG && std::strstr(why, "enabled"));
        v.enabled = 1;
        CHECK(mirror_history_check(v, &why) == RAYS_INVALID_ARG && std::strstr(why, "radius_pixels"));
        v.radius_pixels = inf;
        CHECK(mirror_history_check(v, &why) == RAYS_INVALID_ARG && std::strstr(why, "flags"));
        v.flags = 0;
        CHECK(mirror_history_check(v, &why) == RAYS_INVALID_ARG && std::strstr(why, "reserved"));
        v.reserved = 0;
        CHECK(mirror_history_check(v, &why) == RAYS_OK);
    }
    for (int e : {-1, 2, 3, std::numeric_limits<int>::max(), std::numeric_limits<int>::min()}) {
        MirrorHistoryCall v = def;
        v.enabled = e;
        CHECK(mirror_history_check(v, &why) == RAYS_INVALID_ARG && std::strstr(why, "enabled"));
    }
    for (int e : {0, 1}) {
        MirrorHistoryCall v = def;
        v.enabled = e;
        CHECK(mirror_history_check(v, &why) == RAYS_OK);
    }
    for (float r : {0.0f, -0.0f, -1.0f, -inf, nan, -nan, -std::numeric_limits<float>::denorm_min()}) {
        MirrorHistoryCall v = def;
        v.radius_pixels = r;
        CHECK(mirror_history_check(v, &why) == RAYS_INVALID_ARG && std::strstr(why, "radius_pixels"));
        v.enabled = 0;  // (also when switching off)
        CHECK(mirror_history_check(v, &why) == RAYS_INVALID_ARG);
    }
    for (float r : {std::numeric_limits<float>::denorm_min(), 1e-30f, 0.5f, 1.0f, 2.0f, 8.0f, 1e30f, inf}) {
        MirrorHistoryCall v = def;
        v.radius_pixels = r;
        CHECK(mirror_history_check(v, &why) == RAYS_OK);
    }
    for (uint32_t f : {1u, 2u, 0x80000000u, ~0u}) {
        MirrorHistoryCall v = def;
        v.flags = f;
        CHECK(mirror_history_check(v, &why) == RAYS_INVALID_ARG && std::strstr(why, "flags"));
        v = def, v.reserved = f;
        CHECK(mirror_history_check(v, &why) == RAYS_INVALID_ARG && std::strstr(why, "reserved"));
    }

    // the toggle rule: a change of `enabled` drops the history, a change of the radius alone keeps it; a refused call is never
    // applied, so the previous setting stands
    {
        MirrorHistoryState t;
        MirrorHistoryCall v = def;
        v.enabled = 0, v.radius_pixels = 3.0f;
        CHECK(!mirror_history_set(t, v) && !t.enabled && t.radius_pixels == 3.0f);  // off -> off
        v.enabled = 1;
        CHECK(mirror_history_set(t, v) && t.enabled && t.radius_pixels == 3.0f);  // off -> on
        CHECK(!mirror_history_set(t, v) && t.enabled);                            // on -> on, nothing changed
        v.radius_pixels = inf;
        CHECK(!mirror_history_set(t, v) && t.enabled && t.radius_pixels == inf);  // the radius alone
        MirrorHistoryCall bad = v;
        bad.enabled = 0, bad.radius_pixels = nan;
        CHECK(mirror_history_check(bad, &why) == RAYS_INVALID_ARG && t.enabled && t.radius_pixels == inf);
        v.enabled = 0, v.radius_pixels = 1.0f;
        CHECK(mirror_history_set(t, v) && !t.enabled && t.radius_pixels == 1.0f);  // on -> off (with another radius)
    }

    // rho against a long-double evaluation: one rounding of the double result, so within half an ulp of binary32 plus the double's
    // own error (relative 2^-23 covers both)
    {
        const long double pi = 3.14159265358979323846264338327950288L;
        for (float radius : {0.25f, 1.0f, 2.0f, 4.0f, 8.0f, 1000.0f})
            for (float fov : {1.0f, 30.0f, 55.0f, 90.0f, 120.0f, 179.0f})
                for (int H : {1, 3, 21, 270, 1080, 2160}) {
                    const long double want = (long double)radius * 2.0L * tanl((long double)fov * pi / 360.0L) / (long double)H;
                    const float got = mirror_rho(radius, fov, H);
                    CHECK(got > 0.0f && std::fabs((long double)got - want) <= want * 1.2e-7L);
                    CHECK(got == (float)((double)radius * 2.0 * tan((double)fov * 3.14159265358979323846 / 360.0) / (double)H));
                }
        CHECK(mirror_rho(inf, 55.0f, 21) == inf);  // the distance test then always passes
        CHECK(mirror_rho(2.0f, 55.0f, 21) < mirror_rho(4.0f, 55.0f, 21) && mirror_rho(2.0f, 55.0f, 42) < mirror_rho(2.0f, 55.0f, 21));
    }

    // tags: 0 without a mirror, else unique per (J, m) over J in 1..64 and m in 0..32766, positive, and they round-trip
    {
        for (int m : {0, 1, 77, 32766}) CHECK(mirror_tag(0, m) == 0 && mirror_tag(-1, m) == 0);
        int32_t last = 0;
        bool ok = true;
        for (int J = 1; J <= MIRROR_MAX_BOUNCES; ++J)
            for (int m = 0; m <= 32766; ++m) {
                const int32_t t = mirror_tag(J, m);
                ok = ok && t > last && mirror_tag_bounces(t) == J && mirror_tag_object(t) == m;
                last = t;
            }
        CHECK(ok);
        CHECK(mirror_tag(1, 0) == 32768 && mirror_tag(64, 32766) == 64 * 32768 + 32766 && mirror_tag(2, 5) != mirror_tag(1, 5) && mirror_tag(2, 5) != mirror_tag(2, 6));
    }

    if (failures) return 1;
    std::printf("ok mirror history host rules\n");
    return 0;
}
