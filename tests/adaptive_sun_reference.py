"""The definition of sun sampling in adaptive renders (SRT_ADAPTIVE_SUN_SAMPLING, include/srt_pathtrace.h rules AS1 - AS8),
restated in Python.

path_sun_tail() is sun_sampling_reference.path_sun() — the path loop for ONE (ray, sample) with S2 - S7 — with the path end of
probe_tail_reference.path(): when the path ends because the bounce limit was reached on a surface it also returns the terminal
state (x, n, T, g) of rule T2, which probe_tail_reference.tails() turns into the addend of T3 - T5.  Rule AS4 in this form: every
vertex a bounce is taken from gets its segment (S2 - S6), the bounce that leads to the last hit sees the environment under its own
no_sun (S7), and the vertex at the limit takes no bounce, so it gets the lookup and no segment.  With sun=False it is path() under
the tail, with tail=False it is path_sun(): tests/test_adaptive_sun_reference.py pins both, bit for bit.

pixels() runs it over a frame's camera rays (id = the pixel index, AS1) and folds every pixel's samples in frame order."""
import numpy as np

import probe_tail_reference as PT
from reflection_reference import normalized, offset, reflect
from sun_sampling_reference import CAP, cap_sample, dot3, rand_unit, sun_key, weight
from visibility_reference import rng_key

F = np.float32
FLAG = 16  # SRT_ADAPTIVE_SUN_SAMPLING


def path_sun_tail(sun_scene, o, d, max_bounces, seed, ray_id, frame_no, sun=True, tail=True):
    """(colour [r, g, b, a], terminal, segments, open segments) of sample `frame_no` of the ray (o, d).  terminal: None, or
    dict(x, n, T, g) when `tail` and the path ended because bounce >= max_bounces after a surface hit (rule T1)."""
    scene = sun_scene.scene
    o, d = tuple(F(v) for v in o), tuple(F(v) for v in d)
    i, n, p, _ = scene.trace(o, d)
    if i < 0:
        rgb, a = scene.environment(d)  # :143-145
        return rgb + [a], None, 0, 0
    m = scene.mat[i]
    if max_bounces == 0:
        return list(m["emissive"]) + [F(0.0)], None, 0, 0
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
                e = sun_scene.e0(sray)  # S7 (AS4: also for the bounce that would have led to the last hit)
            L = [F(L[k] + F(e[k] * T[k])) for k in range(3)]
            with np.errstate(invalid="ignore"):
                alpha = F(ea * F(0.0))
            return L + [alpha], None, segments, opened
        n, p, m = n2, p2, scene.mat[i]
        spec = F(1.0) if m["specular"] >= rand_unit(key, draws) else F(0.0)  # :182
        draws += 1
        L = [F(L[k] + F(m["emissive"][k] * T[k])) for k in range(3)]  # :183
        ns = F(F(1.0) - spec)
        f = [F(F(m["base"][k] * ns) + F(m["spec_color"][k] * spec)) for k in range(3)]  # :184
        T = [F(T[k] * f[k]) for k in range(3)]
    if not tail:
        return L + [alpha], None, segments, opened
    g = F(F(1.0) - F(m["smoothness"] * spec))  # T3: the vertex at the limit takes no bounce: the lookup, no segment
    return L + [alpha], dict(x=p, n=n, T=T, g=g), segments, opened


def trace(sun_scene, origins, directions, samples, max_bounces, seed=0, first_sample=1, id_base=0, sun=True, tail=True):
    """Every (ray, sample) of a batch: colours (N, samples, 4) float32, the flat list of terminal states (ray-major), the
    segments traced and how many of them were open."""
    N = len(origins)
    colours = np.zeros((N, samples, 4), F)
    terminals = []
    segments = opened = 0
    for i in range(N):
        for k in range(samples):
            colour, t, sg, op = path_sun_tail(sun_scene, origins[i][:3], directions[i][:3], max_bounces, seed, (id_base + i) & 0xFFFFFFFF,
                                              first_sample + k, sun, tail)
            colours[i, k] = colour
            terminals.append(t)
            segments += sg
            opened += op
    return colours, terminals, segments, opened


def pixels(sun_scene, origins, directions, samples, max_bounces, seed, grid=None, coefficients=None, sun=True, **tail_kw):
    """The accumulator elements (N, 4) float32 of srt_render_adaptive[_tail] with the flag after a uniform budget of `samples`
    from n = 0 on the camera rays (origins, directions), ray index = pixel index.  grid None: no tail (AS1); else the tail of
    probe_tail_reference.tails(terminals, grid, coefficients, **tail_kw) (AS4).  Also returns the tail's work dict (or None)."""
    colours, terminals, _, _ = trace(sun_scene, origins, directions, samples, max_bounces, seed, sun=sun, tail=grid is not None)
    if grid is None:
        return PT.radiance(colours), None
    add, adds, work = PT.tails(terminals, grid, coefficients, **tail_kw)
    return PT.radiance(colours, add=(add, adds)), work
