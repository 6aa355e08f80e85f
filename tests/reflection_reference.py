"""The definition of the reflection guides (srt_render_reflection_gbuffer, include/srt_pathtrace.h), restated in Python.

Hits come from the CPU oracle (srt_oracle_ray_direction, srt_oracle_closest / srt_oracle_closest_m); the reflect, normalize,
offset, path-length and albedo steps are numpy float32 scalars, ONE IEEE operation per line, so that no intermediate is kept in
double.  Colours are clamped at 0 like Color's constructor, as the scene image holds them."""
import ctypes as C

import numpy as np

F = np.float32
OFS = F(.00001)
DISSIPATION = F(0.8)


def c0(v):
    v = F(v)
    return F(0.0) if v < F(0.0) else v


def reflect(d, n):
    """float3::Reflect (Common.hpp:163-165) of float32 triples: d - n * (2 * dot(d, n))."""
    a = F(d[0] * n[0])
    b = F(d[1] * n[1])
    ab = F(a + b)
    c = F(d[2] * n[2])
    dot = F(ab + c)
    k = F(F(2.0) * dot)
    nx = F(n[0] * k)
    ny = F(n[1] * k)
    nz = F(n[2] * k)
    return (F(d[0] - nx), F(d[1] - ny), F(d[2] - nz))


def normalized(v):
    """float3::Normalized: sqrtf((x*x + y*y) + z*z) and three IEEE divisions."""
    xx = F(v[0] * v[0])
    yy = F(v[1] * v[1])
    s = F(xx + yy)
    zz = F(v[2] * v[2])
    s = F(s + zz)
    with np.errstate(invalid="ignore", divide="ignore"):
        length = F(np.sqrt(s))
        return (F(v[0] / length), F(v[1] / length), F(v[2] / length))


def offset(p, n):
    """The bounce origin of Raytracer.cpp:177: p + n * .00001f."""
    ox = F(n[0] * OFS)
    oy = F(n[1] * OFS)
    oz = F(n[2] * OFS)
    return (F(p[0] + ox), F(p[1] + oy), F(p[2] + oz))


def follows(material, min_smoothness, min_specular):
    """smoothness >= min_smoothness && specular_amount >= min_specular in binary32 (a NaN comparison fails)."""
    return bool(F(material.smoothness) >= F(min_smoothness)) and bool(F(material.specular_amount) >= F(min_specular))


class Tracer:
    """GetClosestObject of one ray by the oracle: (index or -1, normal, point, distance) as float32."""

    def __init__(self, oracle, oarr, n, om=None):
        self.L, self.oarr, self.n, self.om = oracle.lib(), oarr, n, om
        self.nn, self.pp, self.t = (C.c_float * 3)(), (C.c_float * 3)(), C.c_float()

    def __call__(self, o, d):
        oo, dd = (C.c_float * 3)(*[float(v) for v in o]), (C.c_float * 3)(*[float(v) for v in d])
        if self.om:
            i = self.L.srt_oracle_closest_m(self.oarr, self.n, self.om[0], self.om[1], oo, dd, self.nn, self.pp, C.byref(self.t))
        else:
            i = self.L.srt_oracle_closest(self.oarr, self.n, oo, dd, self.nn, self.pp, C.byref(self.t))
        return i, tuple(F(v) for v in self.nn), tuple(F(v) for v in self.pp), F(self.t.value)


def chain(trace, oarr, o, d, max_bounces=8, min_smoothness=1.0, min_specular=1.0):
    """One pixel's chain from ray (o, d): (object, normal_depth[4], position[4], albedo[4], J) by the header's definition."""
    J = 0
    D = F(0.0)
    T = [F(0.0), F(0.0), F(0.0)]
    while True:
        i, n, p, t = trace(o, d)
        if i < 0:  # the chain leaves the scene
            return -1, (F(0), F(0), F(0), F(np.inf)), (F(0),) * 4, (F(0),) * 4, J
        m = oarr[i].material
        base = [c0(v) for v in m.base_color]
        D = t if J == 0 else F(D + t)
        if J >= 2:
            T = [F(T[k] * DISSIPATION) for k in range(3)]
        if J < max_bounces and follows(m, min_smoothness, min_specular):
            if J == 0:
                T = base
            else:
                spec = [c0(v) for v in m.specular_color]
                T = [F(T[k] * spec[k]) for k in range(3)]
            d = normalized(reflect(d, n))
            o = offset(p, n)
            J += 1
            continue
        albedo = base if J == 0 else [F(T[k] * base[k]) for k in range(3)]
        return i, (n[0], n[1], n[2], D), (p[0], p[1], p[2], F(1.0)), (albedo[0], albedo[1], albedo[2], F(0.0)), J


def reference(oracle, oarr, n, cam, w, h, om=None, max_bounces=8, min_smoothness=1.0, min_specular=1.0):
    """The five outputs of the whole frame as a dict of arrays in the layout of PathTracer.read_reflection (rows = scene rows)."""
    L = oracle.lib()
    trace = Tracer(oracle, oarr, n, om)
    out = {"object": np.empty((h, w), np.int32), "normal_depth": np.empty((h, w, 4), F), "position": np.empty((h, w, 4), F),
           "albedo": np.empty((h, w, 4), F), "bounces": np.empty((h, w), np.int32)}
    d = (C.c_float * 3)()
    origin = tuple(F(v) for v in cam.position)
    for y in range(h):
        for x in range(w):
            L.srt_oracle_ray_direction(C.byref(cam), w, h, x, y, d)
            i, nd, pos, alb, J = chain(trace, oarr, origin, tuple(F(v) for v in d), max_bounces, min_smoothness, min_specular)
            out["object"][y, x], out["normal_depth"][y, x], out["position"][y, x], out["albedo"][y, x], out["bounces"][y, x] = i, nd, pos, alb, J
    return out


def histogram(ref):
    """(J -> pixels whose chain ends on an object, J -> pixels whose chain leaves the scene)."""
    on, off = {}, {}
    for i, J in zip(ref["object"].reshape(-1), ref["bounces"].reshape(-1)):
        side = on if i != -1 else off
        side[int(J)] = side.get(int(J), 0) + 1
    return on, off


def same_bits(a, b):
    """Bit for bit, NaN as its bits."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    u = np.uint32 if a.dtype.itemsize == 4 else np.uint8
    return np.array_equal(a.view(u), b.view(u))
