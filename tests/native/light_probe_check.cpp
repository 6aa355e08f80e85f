// light_probe_check.cpp — the host-side rules of the light probes (software-raytracer_amd/csrc/srt_light_probes_host.h) as a
// stand-alone program: the header's constants and struct layouts, the defaults, binding and writing the two inputs,
// srt_trace_light_probes' checks in their order — every refusal the header lists — with the state untouched by each, the K and
// P*K limits, the rule that continuing without RESET needs the RADIANCE output and a previous trace of the same P and K into the
// same buffer, the record of the last trace and what srt_read_light_probe_output may report, the size of the partial buffer, the
// grid, the Fibonacci set and the irradiance sum.  Built with -fsanitize=address,undefined and run on the CPU.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "srt_pathtrace.h"
#include "srt_light_probes_host.h"

using namespace srt;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

// srt_read_light_probe_output's rule as srt_capi.hip composes it: the slot, the shared record's read, the byte count of the last trace
static RaysStatus read_light_probe_output(const LightProbeState& s, uint32_t output, const void** src, size_t* bytes) {
    const int i = light_probe_slot(output);
    if (i < 0) return RAYS_INVALID_ARG;
    if (!(*src = s.last.read(output, i))) return RAYS_STATE;
    *bytes = light_probe_elems(i, s.last_probes, s.last_directions) * (4 * sizeof(float));
    return RAYS_OK;
}

static bool same(const LightProbeState& a, const LightProbeState& b) {
    auto in = [](const InputArray& x, const InputArray& y) { return x.bound == y.bound && x.bound_count == y.bound_count && x.own_count == y.own_count; };
    return in(a.positions, b.positions) && in(a.directions, b.directions) && a.call.ran == b.call.ran && a.call.counted == b.call.counted && a.last_probes == b.last_probes &&
           a.last_directions == b.last_directions && a.last.outputs == b.last.outputs && a.last.dst[0] == b.last.dst[0] && a.last.dst[1] == b.last.dst[1];
}

static LightProbeCall call(uint32_t f0, uint32_t n, int32_t bounces, uint32_t flags, uint32_t outputs = LIGHT_PROBE_OUT_COEFFICIENTS, uint32_t reserved = 0) {
    return LightProbeCall{f0, n, bounces, 0u, 0u, flags, outputs, reserved};
}

int main() {
    // the header's constants and layouts are the ones the rules use
    CHECK(SRT_LIGHT_PROBE_RESET == LIGHT_PROBE_FLAG_RESET && SRT_LIGHT_PROBE_NORMALIZE == LIGHT_PROBE_FLAG_NORMALIZE && SRT_LIGHT_PROBE_COUNT_WORK == LIGHT_PROBE_FLAG_COUNT_WORK);
    CHECK((SRT_LIGHT_PROBE_RESET | SRT_LIGHT_PROBE_NORMALIZE | SRT_LIGHT_PROBE_COUNT_WORK) == LIGHT_PROBE_FLAG_ALL && SRT_LIGHT_PROBE_RESET == SRT_RENDER_RESET);
    CHECK(SRT_LIGHT_PROBE_COEFFICIENTS == LIGHT_PROBE_OUT_COEFFICIENTS && SRT_LIGHT_PROBE_RADIANCE == LIGHT_PROBE_OUT_RADIANCE &&
          (SRT_LIGHT_PROBE_COEFFICIENTS | SRT_LIGHT_PROBE_RADIANCE) == LIGHT_PROBE_OUT_ALL && SRT_LIGHT_PROBE_MAX_DIRECTIONS == LIGHT_PROBE_MAX_DIRECTIONS);
    CHECK(sizeof(srt_light_probe_params) == 32 && sizeof(LightProbeCall) == 32 && offsetof(srt_light_probe_params, first_sample) == 0 &&
          offsetof(srt_light_probe_params, sample_count) == 4 && offsetof(srt_light_probe_params, max_bounces) == 8 && offsetof(srt_light_probe_params, seed) == 12 &&
          offsetof(srt_light_probe_params, id_base) == 16 && offsetof(srt_light_probe_params, flags) == 20 && offsetof(srt_light_probe_params, outputs) == 24 &&
          offsetof(srt_light_probe_params, reserved) == 28);
    CHECK(offsetof(LightProbeCall, max_bounces) == 8 && offsetof(LightProbeCall, id_base) == 16 && offsetof(LightProbeCall, flags) == 20 &&
          offsetof(LightProbeCall, outputs) == 24 && offsetof(LightProbeCall, reserved) == 28);
    CHECK(sizeof(srt_light_probe_work) == 56 && offsetof(srt_light_probe_work, valid) == 0 && offsetof(srt_light_probe_work, reserved) == 4 &&
          offsetof(srt_light_probe_work, probes) == 8 && offsetof(srt_light_probe_work, rays) == 16 && offsetof(srt_light_probe_work, samples) == 24 &&
          offsetof(srt_light_probe_work, closest_calls) == 32 && offsetof(srt_light_probe_work, wave_calls) == 40 && offsetof(srt_light_probe_work, waves) == 48);
    {
        LightProbeCall d = call(9, 9, -9, ~0u, ~0u, 9);
        d.seed = 9, d.id_base = 9;
        light_probe_call_default(d);
        CHECK(d.first_sample == 1 && d.sample_count == 16 && d.max_bounces == 8 && d.seed == 0 && d.id_base == 0 && d.flags == LIGHT_PROBE_FLAG_RESET &&
              d.outputs == LIGHT_PROBE_OUT_COEFFICIENTS && d.reserved == 0);
    }
    CHECK(light_probe_slot(1) == 0 && light_probe_slot(2) == 1 && light_probe_slot(0) == -1 && light_probe_slot(3) == -1 && light_probe_slot(4) == -1);

    // the inputs: bind and write
    std::vector<float> a(8), b(8);
    LightProbeState s;
    const char* why = nullptr;
    const void* src = nullptr;
    size_t bytes = 0;
    int rad_own = 0, rad_other = 0, coeff_own = 0;
    CHECK(s.positions.count() == 0 && s.directions.count() == 0);
    CHECK(input_bind(s.directions, a.data(), 0, LIGHT_PROBE_MAX_DIRECTIONS) == RAYS_INVALID_ARG);
    CHECK(input_bind(s.directions, a.data(), 4097, LIGHT_PROBE_MAX_DIRECTIONS) == RAYS_INVALID_ARG);
    CHECK(input_bind(s.directions, nullptr, 5, LIGHT_PROBE_MAX_DIRECTIONS) == RAYS_INVALID_ARG && s.directions.count() == 0);
    CHECK(input_bind(s.directions, a.data(), 4096, LIGHT_PROBE_MAX_DIRECTIONS) == RAYS_OK && s.directions.count() == 4096);
    CHECK(input_bind(s.directions, nullptr, 0, LIGHT_PROBE_MAX_DIRECTIONS) == RAYS_OK && s.directions.count() == 0);
    CHECK(input_bind(s.positions, a.data(), ((size_t)1 << 30) + 1, LIGHT_PROBE_MAX_RAYS) == RAYS_INVALID_ARG);
    CHECK(input_bind(s.positions, a.data(), (size_t)1 << 30, LIGHT_PROBE_MAX_RAYS) == RAYS_OK && s.positions.count() == ((size_t)1 << 30));
    input_written(s.positions, 3);  // a write ends the binding
    CHECK(s.positions.count() == 3 && !s.positions.bound);
    CHECK(input_bind(s.positions, nullptr, 0, LIGHT_PROBE_MAX_RAYS) == RAYS_OK && s.positions.count() == 3);
    s = LightProbeState();

    // the checks: the scene, the arguments, the inputs, the continuation
    CHECK(s.call.work() == RAYS_STATE && read_light_probe_output(s, 1, &src, &bytes) == RAYS_STATE && read_light_probe_output(s, 3, &src, &bytes) == RAYS_INVALID_ARG);
    const LightProbeCall ok = call(1, 16, 8, LIGHT_PROBE_FLAG_RESET);
    CHECK(light_probe_check_trace(s, false, ok, nullptr, &why) == RAYS_STATE && std::strstr(why, "srt_set_scene"));
    CHECK(light_probe_check_trace(s, false, call(0, 0, -1, 8, 0, 1), nullptr, &why) == RAYS_STATE);                                         // the scene comes first
    CHECK(light_probe_check_trace(s, true, call(1, 16, 8, 8), nullptr, &why) == RAYS_INVALID_ARG && std::strstr(why, "flags"));  // the arguments before the inputs
    CHECK(light_probe_check_trace(s, true, ok, nullptr, &why) == RAYS_STATE && std::strstr(why, "positions"));
    CHECK(light_probe_check_trace(s, true, ok, nullptr, nullptr) == RAYS_STATE);  // (a NULL reason is allowed)
    input_written(s.positions, 3);
    CHECK(light_probe_check_trace(s, true, ok, nullptr, &why) == RAYS_STATE && std::strstr(why, "directions"));
    input_written(s.directions, 100);
    {
        const LightProbeState before = s;
        for (uint32_t f : {1u, 3u, 5u, 7u}) CHECK(light_probe_check_trace(s, true, call(1, 16, 8, f), nullptr, &why) == RAYS_OK);
        for (uint32_t f : {8u, 16u, 15u, 0x80000000u, ~0u}) CHECK(light_probe_check_trace(s, true, call(1, 16, 8, f), nullptr, &why) == RAYS_INVALID_ARG && std::strstr(why, "flags"));
        for (uint32_t o : {0u, 4u, 7u, ~0u}) CHECK(light_probe_check_trace(s, true, call(1, 16, 8, 1, o), nullptr, &why) == RAYS_INVALID_ARG && std::strstr(why, "outputs"));
        for (uint32_t o : {1u, 2u, 3u}) CHECK(light_probe_check_trace(s, true, call(1, 16, 8, 1, o), nullptr, &why) == RAYS_OK);
        CHECK(light_probe_check_trace(s, true, call(0, 16, 8, 1), nullptr, &why) == RAYS_INVALID_ARG && std::strstr(why, "first_sample"));
        for (uint32_t n : {0u, 4097u, 0x80000000u, ~0u}) CHECK(light_probe_check_trace(s, true, call(1, n, 8, 1), nullptr, &why) == RAYS_INVALID_ARG && std::strstr(why, "sample_count"));
        for (uint32_t n : {1u, 2u, 64u, 65u, 4096u}) CHECK(light_probe_check_trace(s, true, call(1, n, 8, 1), nullptr, &why) == RAYS_OK);
        CHECK(light_probe_check_trace(s, true, call(0xFFFFFFFFu, 1, 8, 1), nullptr, &why) == RAYS_OK);
        CHECK(light_probe_check_trace(s, true, call(0xFFFFFFFFu, 2, 8, 1), nullptr, &why) == RAYS_INVALID_ARG && std::strstr(why, "2^32"));
        CHECK(light_probe_check_trace(s, true, call(0xFFFFF001u, 4096, 8, 1), nullptr, &why) == RAYS_INVALID_ARG && std::strstr(why, "2^32"));
        for (int32_t bnc : {-1, -8, (int32_t)0x80000000}) CHECK(light_probe_check_trace(s, true, call(1, 16, bnc, 1), nullptr, &why) == RAYS_INVALID_ARG && std::strstr(why, "max_bounces"));
        for (int32_t bnc : {0, 1, 8, 0x7FFFFFFF}) CHECK(light_probe_check_trace(s, true, call(1, 16, bnc, 1), nullptr, &why) == RAYS_OK);
        for (uint32_t r : {1u, ~0u}) CHECK(light_probe_check_trace(s, true, call(1, 16, 8, 1, 1, r), nullptr, &why) == RAYS_INVALID_ARG && std::strstr(why, "reserved"));
        CHECK(same(s, before));
    }
    // K outside 1..4096 (a state no bind or write produces, refused all the same) and P*K > 2^30
    s.directions.own_count = 4097;
    CHECK(light_probe_check_trace(s, true, ok, nullptr, &why) == RAYS_INVALID_ARG && std::strstr(why, "4096"));
    s.directions.own_count = 4096;
    CHECK(input_bind(s.positions, a.data(), (size_t)1 << 18, LIGHT_PROBE_MAX_RAYS) == RAYS_OK);
    CHECK(light_probe_check_trace(s, true, ok, nullptr, &why) == RAYS_OK);  // 2^18 * 2^12 = 2^30
    CHECK(input_bind(s.positions, a.data(), ((size_t)1 << 18) + 1, LIGHT_PROBE_MAX_RAYS) == RAYS_OK);
    CHECK(light_probe_check_trace(s, true, ok, nullptr, &why) == RAYS_INVALID_ARG && std::strstr(why, "2^30"));
    s.directions.own_count = 1;
    CHECK(input_bind(s.positions, a.data(), (size_t)1 << 30, LIGHT_PROBE_MAX_RAYS) == RAYS_OK && light_probe_check_trace(s, true, ok, nullptr, &why) == RAYS_OK);
    s.directions.own_count = 2;
    CHECK(light_probe_check_trace(s, true, ok, nullptr, &why) == RAYS_INVALID_ARG && std::strstr(why, "2^30"));
    CHECK(input_bind(s.positions, nullptr, 0, LIGHT_PROBE_MAX_RAYS) == RAYS_OK && s.positions.count() == 3);
    s.directions.own_count = 100;

    // continuing without RESET: needs the RADIANCE output, and a previous trace of the same P and K into the current buffer
    const LightProbeCall cont = call(4, 6, 8, 0, LIGHT_PROBE_OUT_ALL), cont_only = call(4, 6, 8, 0, LIGHT_PROBE_OUT_RADIANCE);
    CHECK(light_probe_check_trace(s, true, call(4, 6, 8, 0, LIGHT_PROBE_OUT_COEFFICIENTS), &rad_own, &why) == RAYS_STATE && std::strstr(why, "RADIANCE"));
    CHECK(light_probe_check_trace(s, true, cont, &rad_own, &why) == RAYS_STATE && std::strstr(why, "previous trace"));  // no trace yet
    {
        void* dst[LIGHT_PROBE_SLOTS] = {&coeff_own, nullptr};
        light_probe_traced(s, 3, 100, LIGHT_PROBE_OUT_COEFFICIENTS, dst, LIGHT_PROBE_FLAG_RESET);
    }
    CHECK(light_probe_check_trace(s, true, cont, &rad_own, &why) == RAYS_STATE);  // the last trace had no RADIANCE output
    CHECK(read_light_probe_output(s, 1, &src, &bytes) == RAYS_OK && src == &coeff_own && bytes == 3 * 9 * 16);
    CHECK(read_light_probe_output(s, 2, &src, &bytes) == RAYS_STATE && s.call.work() == RAYS_STATE);
    {
        void* dst[LIGHT_PROBE_SLOTS] = {&coeff_own, &rad_own};
        light_probe_traced(s, 3, 100, LIGHT_PROBE_OUT_ALL, dst, LIGHT_PROBE_FLAG_RESET | LIGHT_PROBE_FLAG_COUNT_WORK);
    }
    CHECK(s.call.work() == RAYS_OK);
    CHECK(read_light_probe_output(s, 2, &src, &bytes) == RAYS_OK && src == &rad_own && bytes == 300 * 16);
    CHECK(light_probe_check_trace(s, true, cont, &rad_own, &why) == RAYS_OK && light_probe_check_trace(s, true, cont_only, &rad_own, &why) == RAYS_OK);
    CHECK(light_probe_check_trace(s, true, cont, &rad_other, &why) == RAYS_STATE);  // another buffer is bound now
    CHECK(light_probe_check_trace(s, true, cont, nullptr, &why) == RAYS_STATE);
    input_written(s.positions, 4);  // P changed
    CHECK(light_probe_check_trace(s, true, cont, &rad_own, &why) == RAYS_STATE && light_probe_check_trace(s, true, ok, &rad_own, &why) == RAYS_OK);
    input_written(s.positions, 3);
    input_written(s.directions, 99);  // K changed
    CHECK(light_probe_check_trace(s, true, cont, &rad_own, &why) == RAYS_STATE);
    input_written(s.directions, 100);
    CHECK(light_probe_check_trace(s, true, cont, &rad_own, &why) == RAYS_OK);
    // a later write changes the current inputs, not what the last trace wrote
    input_written(s.positions, 7);
    CHECK(read_light_probe_output(s, 2, &src, &bytes) == RAYS_OK && bytes == 300 * 16);
    input_written(s.positions, 3);
    // the own buffer is re-allocated: the result goes with it, and so does the continuation
    s.last.released(1, &rad_other);
    CHECK(read_light_probe_output(s, 2, &src, &bytes) == RAYS_OK);
    s.last.released(1, nullptr);
    CHECK(read_light_probe_output(s, 2, &src, &bytes) == RAYS_OK);
    s.last.released(1, &rad_own);
    CHECK(read_light_probe_output(s, 2, &src, &bytes) == RAYS_STATE && read_light_probe_output(s, 1, &src, &bytes) == RAYS_OK);
    CHECK(light_probe_check_trace(s, true, cont, &rad_own, &why) == RAYS_STATE);
    {
        void* dst[LIGHT_PROBE_SLOTS] = {nullptr, &rad_own};
        light_probe_traced(s, 3, 100, LIGHT_PROBE_OUT_RADIANCE, dst, LIGHT_PROBE_FLAG_RESET);  // a trace without the flag ends the work record
    }
    CHECK(s.call.work() == RAYS_STATE && read_light_probe_output(s, 1, &src, &bytes) == RAYS_STATE);

    // blocks, units, output sizes, the partial buffer [P][J][9] float4 (none for one block)
    CHECK(light_probe_blocks(1) == 1 && light_probe_blocks(64) == 1 && light_probe_blocks(65) == 2 && light_probe_blocks(100) == 2 && light_probe_blocks(4096) == 64);
    CHECK(light_probe_units(3, 100) == 6 && light_probe_units((size_t)1 << 30, 1) == ((size_t)1 << 30));
    CHECK(light_probe_elems(0, 3, 100) == 27 && light_probe_elems(1, 3, 100) == 300);
    CHECK(light_probe_partial_bytes(3, 1) == 0 && light_probe_partial_bytes(3, 64) == 0 && light_probe_partial_bytes(1000000, 64) == 0);
    CHECK(light_probe_partial_bytes(3, 65) == (size_t)3 * 2 * 9 * 16 && light_probe_partial_bytes(3, 100) == (size_t)3 * 2 * 9 * 16 &&
          light_probe_partial_bytes(4096, 256) == (size_t)4096 * 4 * 9 * 16 && light_probe_partial_bytes(1, 4096) == (size_t)64 * 9 * 16);
    // the grid: units (probe, block), four to a workgroup, at most the resident workgroups, never none; the scratch is radiance's
    const long long resident = 1024;
    CHECK(light_probe_grid(1, 1, 4, resident) == 1 && light_probe_grid(1, 64, 4, resident) == 1 && light_probe_grid(1, 65, 4, resident) == 1 &&
          light_probe_grid(1, 256, 4, resident) == 1 && light_probe_grid(1, 257, 4, resident) == 2 && light_probe_grid(3, 100, 4, resident) == 2);
    CHECK(light_probe_grid(4096, 256, 4, resident) == 1024 && light_probe_grid(4096, 256, 4, (long long)1 << 40) == 4096 && light_probe_grid(1, 1, 4, 0) == 1);
    CHECK(light_probe_grid((size_t)1 << 30, 1, 4, resident) == 1024 && light_probe_grid((size_t)1 << 18, 4096, 4, resident) == 1024);
    CHECK(light_probe_scratch_bytes(1024, 4) == radiance_scratch_bytes(1024, 4) && light_probe_scratch_bytes(1, 4) == (size_t)4 * 64 * 64 * 16);

    // the Fibonacci set: unit directions, z as stated, every weight (float)(4 pi / count); writes count float4 and no more
    for (size_t n : {(size_t)1, (size_t)64, (size_t)100}) {
        std::vector<float> d(4 * n);
        light_probe_sphere(n, d.data());
        const float w = (float)(4.0 * 3.14159265358979323846 / (double)n);
        for (size_t i = 0; i < n; ++i) {
            const double len = std::sqrt((double)d[4 * i] * d[4 * i] + (double)d[4 * i + 1] * d[4 * i + 1] + (double)d[4 * i + 2] * d[4 * i + 2]);
            CHECK(std::fabs(len - 1.0) < 1e-6 && d[4 * i + 3] == w && d[4 * i + 2] == (float)(1.0 - (2.0 * (double)i + 1.0) / (double)n));
        }
    }
    // the irradiance: the constant term alone, then one band-1 term; the fourth lanes are not read
    {
        float c[36] = {0}, rgb[3] = {-1, -1, -1};
        const float up[3] = {0, 0, 1};
        c[0] = 1.0f, c[1] = 2.0f, c[2] = 3.0f, c[3] = NAN;
        light_probe_irradiance(c, up, rgb);
        CHECK(rgb[0] == (3.14159274f * 1.0f) * 0.282095f && rgb[1] == (3.14159274f * 2.0f) * 0.282095f && rgb[2] == (3.14159274f * 3.0f) * 0.282095f);
        c[4 * 2 + 0] = 0.5f;
        light_probe_irradiance(c, up, rgb);
        CHECK(rgb[0] == (3.14159274f * 1.0f) * 0.282095f + (2.09439516f * 0.5f) * (0.488603f * 1.0f));
        float b9[9];
        light_probe_basis(0.0f, 0.0f, 1.0f, b9);
        CHECK(b9[0] == 0.282095f && b9[2] == 0.488603f && b9[6] == 0.315392f * 2.0f && b9[1] == 0.0f && b9[8] == 0.0f);
    }

    if (failures) return 1;
    std::printf("ok light probe host rules\n");
    return 0;
}
