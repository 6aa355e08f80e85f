"""The definition of sun sampling at diffuse bounces (SRT_RADIANCE_SUN_SAMPLING, include/srt_pathtrace.h rules S1 - S9), restated in
Python.

path_sun() is probe_tail_reference.path() — the path loop of srt_trace_radiance for ONE (ray, sample) in numpy float32 scalars, one
IEEE operation per expression — restated with S2 - S7: hits, "open" (the closest hit reporting no object) and the sky come from
the CPU oracle, E0 from the oracle's environment call with a copy of the environment whose sun colour is zero.  With sun=False it
is path() itself.  It also returns the number of sun segments traced.  tests/test_sun_sampling_reference.py pins it."""
import ctypes as C

import numpy as np

from probe_tail_reference import RAND_MAX, c0, fold, radiance  # noqa: F401  (fold and radiance: for the tests that fold paths)
from reflection_reference import normalized, offset, reflect
from visibility_reference import GOLDEN, mix32, rng_draw, rng_key

F = np.float32
FLAG = 16  # SRT_RADIANCE_SUN_SAMPLING == SRT_LIGHT_PROBE_SUN_SAMPLING
CAP = np.array([0x3F7D70A4], np.uint32).view(F)[0]  # c: environment()'s threshold as a float compare
K = F(F(1.0) - CAP)
W0 = F(3.14159265358979323846 / 6.0 * float(K))
SUN_STREAM = 0x53554E21
INF = F(np.inf)


def rand_unit(key, draw):
    return F(F(rng_draw(key, draw)) / RAND_MAX)


def dot3(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def cross(a, b):
    return (F(F(a[1] * b[2]) - F(a[2] * b[1])), F(F(a[2] * b[0]) - F(a[0] * b[2])), F(F(a[0] * b[1]) - F(a[1] * b[0])))


def frame(sun_direction):
    """S5: (s, t1, t2) float32 triples from the environment's sun_direction."""
    s = tuple(F(F(v) * F(-1.0)) for v in sun_direction)
    e = (F(1), F(0), F(0)) if abs(s[0]) < F(0.5) else (F(0), F(1), F(0))
    t1 = normalized(cross(e, s))
    return s, t1, cross(s, t1)


def frame_ok(sun_direction):
    """S5's first refusal: every component of s finite and |s|^2 in [0.9999, 1.0001]."""
    s = tuple(F(F(v) * F(-1.0)) for v in sun_direction)
    if not all(np.isfinite(v) for v in s):
        return False
    with np.errstate(over="ignore"):
        ll = dot3(s, s)
    return bool(ll >= F(0.9999)) and bool(ll <= F(1.0001))


def sun_key(key, draws_after_bounce):
    """S3: the key of the sun stream of a vertex; `draws_after_bounce` = i + 3, the main stream's position after the bounce's draws."""
    with np.errstate(over="ignore"):
        k = np.uint32(key) + np.uint32(draws_after_bounce) * GOLDEN
    return mix32(k ^ np.uint32(SUN_STREAM))


def cap_sample(ks, fr):
    """S4: the direction of the vertex whose sun stream is ks (a key, or an array of keys: the same operations element by element)."""
    s, t1, t2 = fr
    ks = np.asarray(ks, np.uint32)
    a = b = q = np.zeros(ks.shape, F)
    undecided = np.ones(ks.shape, bool)
    for J in range(8):
        aa = F(F(rand_unit(ks, 2 * J) - F(0.5)) * F(2.0))
        bb = F(F(rand_unit(ks, 2 * J + 1) - F(0.5)) * F(2.0))
        qq = F(F(aa * aa) + F(bb * bb))
        take = undecided & (qq <= F(1.0))
        a, b, q = np.where(take, aa, a), np.where(take, bb, b), np.where(take, qq, q)
        undecided = undecided & ~take
        if not undecided.any():
            break
    z = F(F(1.0) - F(q * K))
    h = F(np.sqrt(F(K * F(F(1.0) + z))))
    ah, bh = F(a * h), F(b * h)
    w = tuple(F(F(F(t1[l] * ah) + F(t2[l] * bh)) + F(s[l] * z)) for l in range(3))
    return normalized(w)


def weight(w):
    """S6: W0 / ((m*m)*m), m the largest component of the direction in size."""
    m = np.maximum(np.maximum(np.abs(w[0]), np.abs(w[1])), np.abs(w[2]))
    return F(W0 / F(F(m * m) * m))


class SunScene:
    """A probe_tail_reference.Scene with what S6 and S7 add: the frame, the clamped sun colour and E0."""

    def __init__(self, scene):
        self.scene = scene
        self.frame = frame(scene.env.sun_direction)
        self.sun = [c0(v) for v in scene.env.sun_color]
        self.env0 = type(scene.env).from_buffer_copy(scene.env)
        self.env0.sun_color[:] = (0.0, 0.0, 0.0)
        self._rgb = (C.c_float * 3)()

    def e0(self, d):
        """GetEnvironmentColor with SunColor = (0, 0, 0)."""
        dd = (C.c_float * 3)(*[float(v) for v in d])
        sc = self.scene
        sc.oracle.lib().srt_oracle_environment(C.byref(self.env0), dd, sc.oracle.POW_SHARED, self._rgb)
        return [F(v) for v in self._rgb]


def path_sun(sun_scene, o, d, max_bounces, seed, ray_id, frame_no, sun=True):
    """(colour [r, g, b, a], segments, open segments) of sample `frame_no` of the ray (o, d): probe_tail_reference.path()'s loop
    with S2 - S7 when `sun`."""
    scene = sun_scene.scene
    o, d = tuple(F(v) for v in o), tuple(F(v) for v in d)
    i, n, p, _ = scene.trace(o, d)
    if i < 0:
        rgb, a = scene.environment(d)  # :143-145
        return rgb + [a], 0, 0
    m = scene.mat[i]
    if max_bounces == 0:
        return list(m["emissive"]) + [F(0.0)], 0, 0
    key = rng_key(seed, ray_id, frame_no)
    draws = 0
    L = list(m["emissive"])  # :162
    T = list(m["base"])      # :163
    sray = d                 # :164
    spec = F(1.0) if m["specular"] >= rand_unit(key, draws) else F(0.0)  # :165
    draws += 1
    alpha = F(0.0)
    segments = opened = 0
    s = sun_scene.frame[0]
    for b in range(max_bounces):
        if b != 0:
            T = [F(t * F(0.8)) for t in T]  # :169-171
        refl = reflect(sray, n)  # :172
        sr = tuple(F(F(rand_unit(key, draws + k) - F(0.5)) * F(2.0)) for k in range(3))  # :90-98
        draws += 3
        sr = normalized(sr)
        if dot3(sr, n) < 0:  # :99-105
            sr = tuple(F(v * F(-1.0)) for v in sr)
        tt = F(m["smoothness"] * spec)
        om = F(F(1.0) - tt)
        sray = normalized(tuple(F(F(sr[k] * om) + F(refl[k] * tt)) for k in range(3)))  # :175-176
        origin = offset(p, n)
        diffuse = sun and bool(tt == F(0.0))  # S2
        if diffuse:  # S3 - S6, before the bounce's own result
            w = cap_sample(sun_key(key, draws), sun_scene.frame)
            if dot3(w, s) >= CAP and dot3(w, n) > 0:
                segments += 1
                if scene.trace(origin, w)[0] < 0:
                    opened += 1
                    wt = weight(w)
                    L = [F(L[k] + F(F(sun_scene.sun[k] * wt) * T[k])) for k in range(3)]
        i, n2, p2, _ = scene.trace(origin, sray)  # :177
        if i < 0:  # :178-181
            e, ea = scene.environment(sray)
            if diffuse:
                e = sun_scene.e0(sray)  # S7
            L = [F(L[k] + F(e[k] * T[k])) for k in range(3)]
            with np.errstate(invalid="ignore"):
                alpha = F(ea * F(0.0))
            return L + [alpha], segments, opened
        n, p, m = n2, p2, scene.mat[i]
        spec = F(1.0) if m["specular"] >= rand_unit(key, draws) else F(0.0)  # :182
        draws += 1
        L = [F(L[k] + F(m["emissive"][k] * T[k])) for k in range(3)]  # :183
        ns = F(F(1.0) - spec)
        f = [F(F(m["base"][k] * ns) + F(m["spec_color"][k] * spec)) for k in range(3)]  # :184
        T = [F(T[k] * f[k]) for k in range(3)]
    return L + [alpha], segments, opened


def trace(sun_scene, origins, directions, samples, max_bounces, seed=0, first_sample=1, id_base=0, sun=True):
    """Every (ray, sample) of a batch: colours (N, samples, 4) float32, the segments traced and how many of them were open."""
    N = len(origins)
    colours = np.zeros((N, samples, 4), F)
    segments = opened = 0
    for i in range(N):
        for k in range(samples):
            colour, sg, op = path_sun(sun_scene, origins[i][:3], directions[i][:3], max_bounces, seed, (id_base + i) & 0xFFFFFFFF, first_sample + k, sun)
            colours[i, k] = colour
            segments += sg
            opened += op
    return colours, segments, opened
