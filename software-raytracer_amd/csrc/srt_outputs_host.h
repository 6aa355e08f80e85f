// srt_outputs_host.h — host-side rules every image and ray pass shares and that need no device: the record behind an output a
// caller may bind or read back (srt_bind_* / srt_read_*; the table in DESIGN.md §4.21 says which pass reads under which rule),
// and the grid of persistent workgroups.  The ray outputs and the visibility outputs use a slot for the bound buffer and the
// target only: what their last call wrote, and the rule "last write covered this output", are RaysState's and VisibilityState's
// (srt_rays_host.h, srt_visibility_host.h).  Plain C++ without HIP, shared by srt_capi.hip, srt_rays_host.h (for rays_grid)
// and tests/native/outputs_check.cpp, which runs it under the address and undefined-behaviour sanitizers on the CPU.
#pragma once

#include <stddef.h>

namespace srt {

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
