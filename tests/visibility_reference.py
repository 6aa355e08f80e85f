"""numpy helpers of the per-pixel visibility tests (srt_render_visibility): the reference answer as a composition of what the
library already pins.  From the three guides (OBJECT, NORMAL_DEPTH, POSITION) every segment of the pass is built in numpy
binary32 by the rules of include/srt_pathtrace.h — origin x + n * .00001f, the hemisphere direction from draws 1..3 of
srt_rng_key(seed, pixel, f), the sun segment where n . -sun_direction > 0 — to be sent through srt_write_rays +
srt_trace_occlusion (or asked of the oracle one by one), counted and divided in np.float32.  srt_mix32, srt_rng_key and
srt_rng_draw are ported with uint32 arithmetic; tests/test_visibility_abi.py checks the port against include/srt_defs.h."""
import ctypes as C

import numpy as np

F = np.float32
GOLDEN = np.uint32(0x9E3779B9)


def mix32(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def rng_key(seed, pixel, sample):
    with np.errstate(over="ignore"):
        k = mix32(np.uint32(seed) ^ np.uint32(0xA511E9B3))
        k = mix32(k + np.asarray(pixel, np.uint32))
        return mix32(k + np.asarray(sample, np.uint32))


def rng_draw(key, draw):
    with np.errstate(over="ignore"):
        return mix32(np.asarray(key, np.uint32) + np.uint32(draw) * GOLDEN) >> np.uint32(17)


def unit(v):
    """float3::Normalized in binary32: v / sqrt((x*x + y*y) + z*z)."""
    v = np.asarray(v, F).reshape(-1, 3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return (v / np.sqrt((x * x + y * y) + z * z)[:, None]).astype(F)


def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def rays(o, d, tmax):
    """(N, 3) origins and directions -> the two (N, 4) float32 arrays of srt_write_rays (direction w = t_max)."""
    O4, D4 = np.zeros((len(o), 4), F), np.zeros((len(o), 4), F)
    O4[:, :3], D4[:, :3], D4[:, 3] = o, d, tmax
    return O4, D4


def hit_pixels(obj, rows=None):
    """Flat indices x + y * W (scene rows) of the hit pixels, in index order; `rows`: a band of MEMORY rows."""
    H = obj.shape[0]
    flat = np.flatnonzero(obj.reshape(-1) != -1)
    if rows is not None:
        y = flat // obj.shape[1]
        flat = flat[(y >= H - rows[1]) & (y < H - rows[0])]
    return flat


def origins(nd, pos, pix):
    n, x = nd.reshape(-1, 4)[pix, :3].astype(F), pos.reshape(-1, 4)[pix, :3].astype(F)
    return (x + n * F(.00001)).astype(F), n


def ao_segments(obj, nd, pos, n, first_sample=1, seed=0, radius=np.inf, pix=None):
    """The AO segments of pixels `pix` (default: every hit pixel), pixel-major, `n` per pixel: (pix, O4, D4)."""
    pix = hit_pixels(obj) if pix is None else np.asarray(pix)
    o, nrm = origins(nd, pos, pix)
    p = np.repeat(pix.astype(np.uint32), n)
    with np.errstate(over="ignore"):
        f = np.tile(np.arange(n, dtype=np.uint32), len(pix)) + np.uint32(first_sample)
    key = rng_key(seed, p, f)
    sr = np.stack([(rng_draw(key, k).astype(F) / F(32767) - F(0.5)) * F(2) for k in (1, 2, 3)], axis=1).astype(F)
    d = unit(sr)
    nn = np.repeat(nrm, n, axis=0)
    flip = dot(d, nn) < 0
    d[flip] = d[flip] * F(-1)
    O4, D4 = rays(np.repeat(o, n, axis=0), d, F(radius))
    return pix, O4, D4


def sun_segments(obj, nd, pos, sun_direction, pix=None):
    """c = n . -sun_direction per pixel of `pix` (default: every hit pixel) and the segments of those with c > 0:
    (pix, c, lit, O4, D4)."""
    pix = hit_pixels(obj) if pix is None else np.asarray(pix)
    o, nrm = origins(nd, pos, pix)
    s = -np.asarray(sun_direction, F).reshape(1, 3)
    c = ((nrm[:, 0] * s[:, 0] + nrm[:, 1] * s[:, 1]) + nrm[:, 2] * s[:, 2]).astype(F)
    lit = c > 0
    O4, D4 = rays(o[lit], np.repeat(s, int(lit.sum()), axis=0), F(np.inf))
    return pix, c, lit, O4, D4


def occluded_by_tracer(pt, O4, D4):
    """The segments through srt_write_rays + srt_trace_occlusion: 1 = occluded."""
    if len(O4) == 0:
        return np.zeros(0, np.int32)
    pt.write_rays(O4, D4)
    pt.trace_occlusion()
    return pt.ray_output("occluded")


def occluded_by_closest(pt, O4, D4):
    """The segments through srt_trace_rays' OCCLUDED output (the closest hit's distance < t_max)."""
    if len(O4) == 0:
        return np.zeros(0, np.int32)
    pt.write_rays(O4, D4)
    pt.trace_rays(outputs="occluded")
    return pt.ray_output("occluded")


def occluded_by_oracle(oracle, oarr, n, O4, D4, om=None):
    """srt_oracle_closest (with om: srt_oracle_closest_m) per segment: `hit and t < t_max` in binary32."""
    L = oracle.lib()
    nn, pp, t = (C.c_float * 3)(), (C.c_float * 3)(), C.c_float()
    out = np.zeros(len(O4), np.int32)
    for i in range(len(O4)):
        o, d = (C.c_float * 3)(*O4[i, :3]), (C.c_float * 3)(*D4[i, :3])
        idx = L.srt_oracle_closest_m(oarr, n, om[0], om[1], o, d, nn, pp, C.byref(t)) if om else L.srt_oracle_closest(oarr, n, o, d, nn, pp, C.byref(t))
        out[i] = 1 if idx >= 0 and F(t.value) < D4[i, 3] else 0
    return out


def ao_image(obj, pix, occluded, n):
    """ao = (float)open / (float)n on `pix`, 1 elsewhere."""
    ao = np.ones(obj.size, F)
    open_count = (1 - occluded.reshape(len(pix), n)).sum(axis=1)
    ao[pix] = open_count.astype(F) / F(n)
    return ao.reshape(obj.shape)


def sun_image(obj, pix, c, lit, occluded):
    """sun = c where c > 0 and the segment is open, 0 elsewhere."""
    sun = np.zeros(obj.size, F)
    v = np.zeros(len(pix), F)
    v[lit] = np.where(occluded == 0, c[lit], F(0))
    sun[pix] = v
    return sun.reshape(obj.shape)


def reference(pt, obj, nd, pos, sun_direction, n, first_sample=1, seed=0, radius=np.inf, trace=occluded_by_tracer):
    """(ao, sun, open AO segments, open sun segments) of the whole frame, the segments answered by `trace`."""
    pix, O4, D4 = ao_segments(obj, nd, pos, n, first_sample, seed, radius)
    occ = trace(pt, O4, D4)
    spix, c, lit, SO4, SD4 = sun_segments(obj, nd, pos, sun_direction)
    socc = trace(pt, SO4, SD4)
    return ao_image(obj, pix, occ, n), sun_image(obj, spix, c, lit, socc), int((occ == 0).sum()), int((socc == 0).sum())


def work_formula(obj, c_image, n, ao=True, sun=True, rows=None):
    """(segments, wave_trips) of a call by the header's rule 11: per 8 x 8 tile of the band (tiles start at the band's first
    scene row) with h hit pixels, ceil(h * n / 64) AO trips and one sun trip when some pixel has c > 0; n segments per hit
    pixel and one per pixel with c > 0.  c_image: (H, W) n . -sun_direction (any value on miss pixels)."""
    H, W = obj.shape
    rb, re = rows if rows is not None else (0, H)
    y0, y1 = H - re, H - rb
    hit = obj != -1
    with np.errstate(invalid="ignore"):
        lit = hit & (c_image > 0)
    segments = trips = 0
    for ty in range(y0, y1, 8):
        for tx in range(0, W, 8):
            h = int(hit[ty:min(ty + 8, y1), tx:tx + 8].sum())
            l = int(lit[ty:min(ty + 8, y1), tx:tx + 8].sum())
            if ao:
                segments += h * n
                trips += (h * n + 63) // 64
            if sun:
                segments += l
                trips += 1 if l else 0
    return segments, trips


def c_of(nd, sun_direction):
    """(H, W) n . -sun_direction in binary32."""
    s = -np.asarray(sun_direction, F)
    n = nd.astype(F)
    return ((n[..., 0] * s[0] + n[..., 1] * s[1]) + n[..., 2] * s[2]).astype(F)


def oracle_gbuffer(oracle, oarr, n, cam, w, h, om=None):
    """The three guides from the oracle on the CPU (GetRayDirection + GetClosestObject per pixel): what srt_render_gbuffer is
    pinned to.  (object (H, W) int32, normal_depth (H, W, 4), position (H, W, 4)), miss values as the header's table."""
    L = oracle.lib()
    d, nn, pp, t = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)(), C.c_float()
    origin = (C.c_float * 3)(*cam.position)
    obj = np.full((h, w), -1, np.int32)
    nd, pos = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
    nd[..., 3] = np.inf
    for y in range(h):
        for x in range(w):
            L.srt_oracle_ray_direction(C.byref(cam), w, h, x, y, d)
            i = L.srt_oracle_closest_m(oarr, n, om[0], om[1], origin, d, nn, pp, C.byref(t)) if om else L.srt_oracle_closest(oarr, n, origin, d, nn, pp, C.byref(t))
            if i >= 0:
                obj[y, x], nd[y, x], pos[y, x] = i, (nn[0], nn[1], nn[2], t.value), (pp[0], pp[1], pp[2], 1.0)
    return obj, nd, pos
