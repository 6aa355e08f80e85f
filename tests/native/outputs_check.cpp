// outputs_check.cpp — the host-side rules the image and ray passes share (software-raytracer_amd/csrc/srt_outputs_host.h) as a
// stand-alone program.  An output slot goes through bind, write, re-bind, grow and read sequences under each of its read rules.
// The ray outputs, whose last-write record is RaysState's (srt_rays_host.h), go through the same sequences under "last write
// covered this output".  The two records every ray and probe pass keeps are checked exhaustively: LastOutputs for 1, 2 and 5
// slots (written, released, read), CallRecord for all four bool combinations.  The grid of persistent workgroups is compared
// with the two formulas it replaced, over every input of the ranges below.  Built with -fsanitize=address,undefined and run on
// the CPU.
#include <algorithm>
#include <cstdio>

#include "srt_outputs_host.h"
#include "srt_rays_host.h"

using namespace srt;

#include "read_ray_output.h"

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

// the grid of srt_render_gbuffer, srt_render_visibility and srt_render_subsamples as it was written there (tiles >= 1: a band has rows)
static long long old_tile_grid(long long tiles, long long resident) {
    const long long need = (tiles + 2 * 2 - 1) / (2 * 2);
    return std::min<long long>(need, resident);
}

// LastOutputs<N>, exhaustively: every mask of written outputs, then for every slot a release of a buffer that is not the one last
// written (another one, NULL: the first allocation) and of the one that is, and a read of every single bit and of every slot
// under a bit that is not its own.
template <int N>
static void check_last_outputs() {
    char own[N], bound[N], other;  // own[i]: the handle's own buffer of slot i; bound[i]: a caller's
    for (uint32_t written = 0; written < (1u << N); ++written)
        for (uint32_t from_bound = 0; from_bound < (1u << N); ++from_bound) {  // which of the slots were written into a bound buffer
            const void* to[N];
            for (int i = 0; i < N; ++i) to[i] = (from_bound >> i & 1) ? &bound[i] : &own[i];
            LastOutputs<N> fresh;
            for (int i = 0; i < N; ++i) CHECK(fresh.read(1u << i, i) == nullptr && fresh.dst[i] == nullptr);  // a bit never written
            CHECK(fresh.outputs == 0);
            fresh.wrote(written, to);
            CHECK(fresh.outputs == written);
            for (int i = 0; i < N; ++i) {
                const bool w = (written >> i & 1) != 0;
                CHECK(fresh.dst[i] == (w ? to[i] : nullptr));            // an output left out has no buffer, whatever to[i] says
                CHECK(fresh.read(1u << i, i) == (w ? to[i] : nullptr));  // written into an own or into a bound buffer: that buffer
                for (int j = 0; j < N; ++j)
                    if (j != i) CHECK(fresh.read(1u << j, i) == ((written >> j & 1) ? fresh.dst[i] : nullptr));  // (the bit gates, the slot picks)
            }
            for (int slot = 0; slot < N; ++slot) {
                const void* const not_last[] = {&other, nullptr, (from_bound >> slot & 1) ? (const void*)&own[slot] : (const void*)&bound[slot]};
                for (const void* p : not_last) {  // a buffer that is not the one last written: nothing goes
                    LastOutputs<N> s = fresh;
                    s.released(slot, p);
                    CHECK(s.outputs == fresh.outputs);
                    for (int i = 0; i < N; ++i) CHECK(s.dst[i] == fresh.dst[i]);
                }
                LastOutputs<N> s = fresh;  // the one last written: that output goes, and no other
                s.released(slot, to[slot]);
                const bool w = (written >> slot & 1) != 0;
                CHECK(s.outputs == (written & ~(1u << slot)) && s.dst[slot] == nullptr && s.read(1u << slot, slot) == nullptr);
                for (int i = 0; i < N; ++i)
                    if (i != slot) CHECK(s.dst[i] == fresh.dst[i] && s.read(1u << i, i) == fresh.read(1u << i, i));
                if (!w) CHECK(s.outputs == fresh.outputs);  // (releasing to[slot] of an output left out releases nothing)
                LastOutputs<N> f = fresh;  // forget: as released of whatever buffer it is
                f.forget(slot);
                CHECK(f.outputs == s.outputs);
                for (int i = 0; i < N; ++i) CHECK(f.dst[i] == s.dst[i]);
                s.wrote(written, to);  // written, released, written again: readable again
                CHECK(s.read(1u << slot, slot) == (w ? to[slot] : nullptr));
            }
        }
}

// srt::rays_grid as it was, on blocks of 64 rays
static unsigned old_rays_grid(long long blocks, int waves, long long resident) {
    const long long need = (blocks + waves - 1) / waves;
    const long long g = need < resident ? need : resident;
    return (unsigned)(g < 1 ? 1 : g);
}

int main() {
    int own_mem[4], other_mem[4], regrown_mem[4];
    const void *own = own_mem, *t = other_mem, *regrown = regrown_mem;

    {  // nothing written, nothing bound: every rule refuses, with or without an own buffer
        OutputSlot s;
        CHECK(s.current(nullptr) == nullptr && s.current(own) == own);
        CHECK(!s.read_any(nullptr) && !s.read_any(own) && !s.read_last_only(nullptr) && !s.read_last_only(own));
        s.bind(t);  // a bound buffer nobody wrote is no more readable
        CHECK(s.current(own) == t && !s.read_any(own) && !s.read_last_only(own));
    }
    {  // "any buffer once written" (denoised, upsampled, antialiased, variance)
        OutputSlot s;
        s.wrote(own);
        CHECK(s.read_any(own) == own);
        s.bind(t);  // a write to own, then a bind, then a read: the bound buffer, though nothing wrote it
        CHECK(s.read_any(own) == t);
        s.wrote(t);
        CHECK(s.read_any(own) == t);
        s.bind(nullptr);  // a bind to NULL after a write: back to the own buffer and what it held
        CHECK(s.read_any(own) == own);
        OutputSlot b;  // written into a bound buffer only: un-bound, there is no own buffer to read
        b.bind(t);
        b.wrote(t);
        b.bind(nullptr);
        CHECK(b.written && b.read_any(nullptr) == nullptr);
    }
    {  // "only the buffer last written" (motion)
        OutputSlot s;
        s.wrote(own);
        CHECK(s.read_last_only(own) == own);
        s.bind(t);  // a write to own, then a bind, then a read: refused
        CHECK(s.read_last_only(own) == nullptr);
        s.wrote(t);
        CHECK(s.read_last_only(own) == t);
        s.bind(nullptr);  // a bind to NULL after a write: the own buffer is not the one last written
        CHECK(s.read_last_only(own) == nullptr);
        s.bind(t);  // ... and binding the written buffer again makes it readable again: a re-bind leaves the record alone
        CHECK(s.read_last_only(own) == t);
        s.bind(nullptr);
        s.wrote(own);
        CHECK(s.read_last_only(own) == own);
    }
    {  // targets and growth
        OutputSlot s;
        CHECK(s.target(0, 16).own && s.target(0, 16).grow);    // no own buffer yet
        CHECK(s.target(16, 16).own && !s.target(16, 16).grow);  // large enough
        CHECK(s.target(16, 17).own && s.target(16, 17).grow);   // too small
        s.bind(t);
        CHECK(!s.target(0, 16).own && !s.target(0, 16).grow && !s.target(16, 17).grow);  // a bound buffer is the caller's business
        s.bind(nullptr);
        s.wrote(own, 8);
        s.own_released(own);  // a grow drops the record of a last write into the own buffer ...
        CHECK(s.last == nullptr && s.read_last_only(regrown) == nullptr && s.last_count == 8);  // (the count is the last write's, wherever it went)
        CHECK(s.read_any(regrown) == regrown);  // (... which "any buffer once written" never looks at)
        s.wrote(t, 8);
        s.own_released(own);  // ... and no other
        CHECK(s.last == t && s.read_last_only(regrown) == nullptr && s.last_count == 8);
        OutputSlot e;
        e.own_released(nullptr);  // the first allocation releases nothing
        CHECK(e.last == nullptr && !e.written);
    }
    {  // "last write covered this output" (ray outputs; visibility has the same shape): the slot holds the bound buffer, RaysState
       // the record of the last trace
        RaysState r;
        OutputSlot object, occluded;
        rays_written(r, 33);
        const void* src = nullptr;
        size_t bytes = 0;
        CHECK(read_ray_output(r, RAYS_OUT_OBJECT, &src, &bytes) == RAYS_STATE);  // nothing traced
        void* dst[RAYS_SLOTS] = {const_cast<void*>(object.current(own)), nullptr, nullptr, nullptr, const_cast<void*>(occluded.current(regrown))};
        rays_traced(r, RAYS_OUT_OBJECT | RAYS_OUT_OCCLUDED, dst);
        CHECK(read_ray_output(r, RAYS_OUT_OBJECT, &src, &bytes) == RAYS_OK && src == own && bytes == 33 * 4);
        object.bind(t);  // a write to own, then a bind, then a read: still the own buffer, the one the last trace wrote
        CHECK(read_ray_output(r, RAYS_OUT_OBJECT, &src, &bytes) == RAYS_OK && src == own);
        dst[0] = const_cast<void*>(object.current(own));
        rays_traced(r, RAYS_OUT_OBJECT | RAYS_OUT_OCCLUDED, dst);
        object.bind(nullptr);  // a bind to NULL after a write: still the buffer the last trace wrote
        CHECK(read_ray_output(r, RAYS_OUT_OBJECT, &src, &bytes) == RAYS_OK && src == t);
        r.last.released(0, own);  // the own OBJECT buffer grows: the last trace did not write it, nothing goes
        CHECK(read_ray_output(r, RAYS_OUT_OBJECT, &src, &bytes) == RAYS_OK && src == t);
        r.last.released(4, regrown);  // the own OCCLUDED buffer grows: the last trace's copy goes with it, and no other
        CHECK(read_ray_output(r, RAYS_OUT_OCCLUDED, &src, &bytes) == RAYS_STATE);
        CHECK(read_ray_output(r, RAYS_OUT_OBJECT, &src, &bytes) == RAYS_OK && src == t);
        r.last.released(1, nullptr);  // the first allocation of an output the last trace left out
        CHECK(read_ray_output(r, RAYS_OUT_NORMAL_DEPTH, &src, &bytes) == RAYS_STATE && r.last.outputs == RAYS_OUT_OBJECT);
        rays_traced(r, RAYS_OUT_ALBEDO, dst);  // a later trace that leaves the output out
        CHECK(read_ray_output(r, RAYS_OUT_OBJECT, &src, &bytes) == RAYS_STATE);
    }

    // the record of the last call's outputs, for the slot counts in use: radiance and the probe list (1), visibility and the probe
    // passes (2), the ray outputs (5)
    check_last_outputs<1>();
    check_last_outputs<2>();
    check_last_outputs<5>();
    {  // the record of the last call: the work query passes only after a call that ran and counted
        CHECK(CallRecord{}.work() == RAYS_STATE);
        for (int ran = 0; ran < 2; ++ran)
            for (int counted = 0; counted < 2; ++counted) {
                const CallRecord c{ran != 0, counted != 0};  // (ran = false with counted = true: the probe tail with the mode off never makes it, and it would not pass)
                CHECK(c.work() == (ran && counted ? RAYS_OK : RAYS_STATE));
                for (int with_count = 0; with_count < 2; ++with_count) {  // done() after any of the four: only its own argument counts
                    CallRecord d = c;
                    d.done(with_count != 0);
                    CHECK(d.ran && d.counted == (with_count != 0) && d.work() == (with_count ? RAYS_OK : RAYS_STATE));
                }
            }
    }

    // The grid.  The tile passes never have zero tiles (a band has at least one row and one column), where their formula gave 0
    // workgroups, which is no launch; the ray formula gives 1 there, and so does persistent_grid.
    const long long residents[] = {1, 2, 255, 256, 1024};
    for (long long units = 0; units <= 5000; ++units)
        for (int per : {1, 4})
            for (long long resident : residents) {
                const unsigned g = persistent_grid(units, per, resident);
                CHECK(g == old_rays_grid(units, per, resident));
                if (per == 4 && units >= 1) CHECK((long long)g == old_tile_grid(units, resident));
                CHECK(g >= 1 && (long long)g <= resident && (units == 0 || (long long)(g - 1) * per < units));
            }
    CHECK(persistent_grid(0, 4, 1024) == 1 && old_tile_grid(0, 1024) == 0);  // (the one input at which the two old formulas differ)
    CHECK(persistent_grid(1, 4, 1024) == 1 && persistent_grid(4, 4, 1024) == 1 && persistent_grid(5, 4, 1024) == 2);
    for (long long resident : residents) {  // one more workgroup's worth than is resident
        CHECK(persistent_grid(4 * resident, 4, resident) == resident && persistent_grid(4 * resident + 1, 4, resident) == resident);
        CHECK(persistent_grid(4 * resident - 4, 4, resident) == (resident > 1 ? resident - 1 : 1));
    }
    for (size_t n : {(size_t)1, (size_t)33, (size_t)64, (size_t)65, (size_t)257, (size_t)4099, (size_t)1 << 30})
        CHECK(rays_grid(n, 4, 1024) == old_rays_grid((long long)((n + 63) / 64), 4, 1024));
    for (int w = 1; w <= 40; ++w)
        for (int rows = 1; rows <= 40; ++rows) CHECK(band_tiles(w, rows) == (long long)((w + 8 - 1) / 8) * ((rows + 8 - 1) / 8));
    CHECK(band_tiles(24, 16) == 6 && persistent_grid(band_tiles(24, 16), OUT_WG_UNITS, 1024) == 2);  // one full workgroup and one partial
    CHECK(band_tiles(1920, 1080) == 240 * 135 && band_tiles(1, 1) == 1);

    if (failures) return 1;
    std::printf("ok output slots and the persistent grid\n");
    return 0;
}
