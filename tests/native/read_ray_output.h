// read_ray_output.h — for the stand-alone checks that read a ray output (rays, outputs, occlusion, radiance): srt_read_ray_output's
// rule as srt_capi.hip composes it from srt_rays_host.h — the slot, the shared record's read, the byte count of the last trace.
// Included after `using namespace srt;`.
#pragma once

#include "srt_rays_host.h"

static RaysStatus read_ray_output(const RaysState& s, uint32_t output, const void** src, size_t* bytes) {
    const int i = rays_slot(output);
    if (i < 0) return RAYS_INVALID_ARG;
    if (!(*src = s.last.read(output, i))) return RAYS_STATE;
    *bytes = s.last_count * rays_elem_bytes(i);
    return RAYS_OK;
}
