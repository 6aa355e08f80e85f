// srt_outputs_host.h — host-side rules every image, ray and probe pass shares and that need no device: the record behind an output a
// caller may bind or read back (srt_bind_* / srt_read_*; the table in DESIGN.md §4.21 says which pass reads under which rule),
// the record of a pass's last call (has it run, did it count its work), the record of which outputs that call wrote and where,
// the record of an input array a caller may write or bind, and the grid of persistent workgroups.  The ray, visibility and probe
// outputs use an OutputSlot for the bound buffer and the target only: what their last call wrote, and the rule "last write
// covered this output", are the LastOutputs in their pass's state.  Plain C++ without HIP, shared by srt_capi.hip, the *_host.h
// rule headers and tests/native/outputs_check.cpp, which runs it under the address and undefined-behaviour sanitizers on the CPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace srt {

enum RaysStatus { RAYS_OK = 0, RAYS_INVALID_ARG = 1, RAYS_STATE = 4 };  // the values of SRT_OK / SRT_ERR_INVALID_ARG / SRT_ERR_STATE

// One output.  The handle's own buffer is device memory the context owns; the slot is told its address (and size) where a rule
// needs it and never keeps it.
struct OutputSlot {
    const void* bound = nullptr;  // the caller's buffer (srt_bind_*); NULL: the handle's own
    const void* last = nullptr;   // the buffer the last write went to; NULL: none, or it was the own one and has been re-allocated
    size_t last_count = 0;        // what the last write covered, in the pass's unit (k of the sub-samples; 1 where a write is always a frame)
    bool written = false;         // some call has written this output, into whichever buffer

    // srt_bind_*: later calls write (and the reads look at) `p`; NULL returns to the own buffer.  The records stay as they are.
    void bind(const void* p) { bound = p; }
    // the buffer a call writes and a consumer reads: the bound one, else the own one (NULL before its first use)
    const void* current(const void* own) const { return bound ? bound : own; }

    // What a call that writes `bytes` has to do first: it writes the own buffer unless one is bound, and an own buffer of
    // own_bytes (0: none yet) that is too small must be allocated or grown.
    struct Target {
        bool own, grow;
    };
    Target target(size_t own_bytes, size_t bytes) const { return Target{!bound, !bound && own_bytes < bytes}; }
    // ... the own buffer at `own` is about to be re-allocated: it is no longer the buffer last written (the count stays)
    void own_released(const void* own) {
        if (own && last == own) last = nullptr;
    }
    // a call of the pass is enqueued: it wrote this output to dst
    void wrote(const void* dst, size_t count = 1) { last = dst, last_count = count, written = true; }

    // The read rules: the buffer to copy from, NULL for SRT_ERR_STATE.
    // "any buffer once written": the current buffer, once any call has written the output anywhere
    const void* read_any(const void* own) const { return written ? current(own) : nullptr; }
    // "only the buffer last written": the current buffer, if it is the one the last write went to
    const void* read_last_only(const void* own) const {
        const void* c = current(own);
        return c && c == last ? c : nullptr;
    }
};

// The last call of a pass: has there been one, and did it count its work (the pass's *_COUNT_WORK flag)?
struct CallRecord {
    bool ran = false, counted = false;
    // a call of the pass is enqueued
    void done(bool with_count) { ran = true, counted = with_count; }
    // srt_get_*_work: only the record of a last call that counted
    RaysStatus work() const { return ran && counted ? RAYS_OK : RAYS_STATE; }
};

// Which of a pass's N outputs (bit i of the mask: slot i) its last call wrote, and where.  The sizes that go with them (the
// last P, K, R or ray count) stay in the pass's state.
template <int N>
struct LastOutputs {
    uint32_t outputs = 0;
    const void* dst[N] = {};

    // a call of the pass is enqueued: it wrote `written`, output of slot i to to[i], and nothing else
    void wrote(uint32_t written, const void* const* to) {
        outputs = written;
        for (int i = 0; i < N; ++i) dst[i] = (written & (1u << i)) ? to[i] : nullptr;
    }
    // the last call's copy of output `slot` counts as not written
    void forget(int slot) { dst[slot] = nullptr, outputs &= ~(1u << slot); }
    // The handle's own buffer of output `slot`, at `own`, is about to be re-allocated: the last call's copy of that output goes with it.
    void released(int slot, const void* own) {
        if (own && dst[slot] == own) forget(slot);
    }
    // srt_read_*_output: the buffer the last call wrote the single output `output_bit` (of slot `slot`) to, NULL for SRT_ERR_STATE
    const void* read(uint32_t output_bit, int slot) const { return (outputs & output_bit) ? dst[slot] : nullptr; }
};

// One input array (probe positions, directions, coefficients, a list ...): the caller's bound array, when there is one, comes
// first; the handle's own buffer holds own_count elements (0: never written).
struct InputArray {
    const void* bound = nullptr;
    size_t bound_count = 0;
    size_t own_count = 0;
    size_t count() const { return bound ? bound_count : own_count; }  // 0: none
};

// srt_bind_* of an input: NULL, 0 returns to the own buffer; otherwise an array and a count in 1 .. limit.  On an error the state
// is left as it was.
inline RaysStatus input_bind(InputArray& in, const void* d_ptr, size_t count, size_t limit) {
    if (!d_ptr && count == 0) return in.bound = nullptr, in.bound_count = 0, RAYS_OK;
    if (!d_ptr || count < 1 || count > limit) return RAYS_INVALID_ARG;
    in.bound = d_ptr, in.bound_count = count;
    return RAYS_OK;
}
// srt_write_* of an input once the copy has succeeded: a binding ends
inline void input_written(InputArray& in, size_t count) { in.own_count = count, in.bound = nullptr, in.bound_count = 0; }

// The tile geometry of the persistent image passes (srt_kernel.hip.h: TILE_W x TILE_H pixels per wave, WG_TILES_X * WG_TILES_Y waves
// per workgroup; srt_capi.hip asserts that they agree).
constexpr int OUT_TILE = 8, OUT_WG_UNITS = 4;

// 8 x 8 tiles that meet a band of `rows` rows of a frame `width` pixels wide
inline long long band_tiles(int width, int rows) { return (long long)((width + OUT_TILE - 1) / OUT_TILE) * ((rows + OUT_TILE - 1) / OUT_TILE); }

// Persistent workgroups that each take `units_per_workgroup` units (tiles, blocks of 64 rays) at a time: as many as there are
// units for, at most `resident`, never none.
inline unsigned persistent_grid(long long units, int units_per_workgroup, long long resident) {
    const long long need = (units + units_per_workgroup - 1) / units_per_workgroup;
    const long long g = need < resident ? need : resident;
    return (unsigned)(g < 1 ? 1 : g);
}

}  // namespace srt
