"""The definition of the probe tail (srt_probe_tail, include/srt_pathtrace.h rules T1 - T6), restated in Python.

path() is the path loop of srt_trace_radiance (Raytracer.cpp:141-146, 162-185, 212) for ONE (ray, sample) in numpy float32 scalars,
one IEEE operation per expression: hits and sky come from the CPU oracle (srt_oracle_closest[_m], srt_oracle_environment with
POW_SHARED), the random stream is visibility_reference's port of srt_rng_key / srt_rng_draw, reflect and normalize are
reflection_reference's.  It returns the sample's colour and, when the path ended at the bounce limit on a surface, the terminal
state (x, n, T, g) of rule T2.  tests/test_probe_tail_reference.py pins it against the oracle's accumulator with the tail off.

tails() is rules T3 - T5 for the terminal states of many paths at once.  The lookup is NOT restated: (M, a) comes from the shading
references that are pinned bit for bit against the three shading calls (probe_grid_reference.shade, probe_depth_reference.shade,
probe_states_reference.shade), called with the terminal points and normals as the guides of a one-row frame."""
import ctypes as C

import numpy as np

import probe_depth_reference as PD
import probe_grid_reference as PG
import probe_states_reference as PS
from reflection_reference import Tracer, normalized, offset, reflect
from visibility_reference import rng_draw, rng_key

F = np.float32
NORMAL_WEIGHT, DEPTH, STATES, COUNT_WORK = 1, 2, 4, 8  # SRT_PROBE_TAIL_*
HEMISPHERE_MEAN = PG.HEMISPHERE                          # the default band weights: (1, 0.5, 0)
RAND_MAX = F(32767)


def c0(v):
    v = F(v)
    return F(0.0) if v < F(0.0) else v


class Scene:
    """What path() needs of a scene: the oracle's closest hit and environment, and the materials as the scene image holds them
    (colours clamped at 0 like Color's constructor)."""

    def __init__(self, oracle, oarr, n, om=None, env=None):
        self.oracle, self.oarr, self.n = oracle, oarr, n
        self.trace = Tracer(oracle, oarr, n, om)
        self.env = env if env is not None else oracle.default_environment()
        self._rgb = (C.c_float * 3)()
        self.mat = []
        for i in range(n):
            m = oarr[i].material
            self.mat.append(dict(smoothness=F(m.smoothness), specular=F(m.specular_amount), base=[c0(v) for v in m.base_color],
                                 emissive=[c0(v) for v in m.emissive_color], spec_color=[c0(v) for v in m.specular_color]))

    def environment(self, d):
        """(rgb, alpha): GetEnvironmentColor; the alpha is +0, or NaN for a non-finite direction (upd - upd)."""
        dd = (C.c_float * 3)(*[float(v) for v in d])
        self.oracle.lib().srt_oracle_environment(C.byref(self.env), dd, self.oracle.POW_SHARED, self._rgb)
        with np.errstate(invalid="ignore"):
            upd = F(F(F(d[0] * F(0.0)) + F(d[1] * F(1.0))) + F(d[2] * F(0.0)))
            return [F(v) for v in self._rgb], F(upd - upd)


def rand_unit(key, draw):
    return F(F(rng_draw(key, draw)) / RAND_MAX)


def path(scene, o, d, max_bounces, seed, ray_id, frame):
    """(colour [r, g, b, a], terminal) of sample `frame` of the ray (o, d) whose stream is srt_rng_key(seed, ray_id, frame).
    terminal: None, or dict(x, n, T, g) when the path ended because bounce >= max_bounces after a surface hit (rule T1)."""
    o, d = tuple(F(v) for v in o), tuple(F(v) for v in d)
    i, n, p, _ = scene.trace(o, d)
    if i < 0:
        rgb, a = scene.environment(d)  # :143-145
        return rgb + [a], None
    m = scene.mat[i]
    if max_bounces == 0:
        return list(m["emissive"]) + [F(0.0)], None
    key = rng_key(seed, ray_id, frame)
    draws = 0
    L = list(m["emissive"])  # :162
    T = list(m["base"])      # :163
    sray = d                 # :164
    spec = F(1.0) if m["specular"] >= rand_unit(key, draws) else F(0.0)  # :165
    draws += 1
    alpha = F(0.0)
    for b in range(max_bounces):
        if b != 0:
            T = [F(t * F(0.8)) for t in T]  # :169-171
        refl = reflect(sray, n)  # :172
        sr = tuple(F(F(rand_unit(key, draws + k) - F(0.5)) * F(2.0)) for k in range(3))  # :90-98
        draws += 3
        sr = normalized(sr)
        if F(F(F(sr[0] * n[0]) + F(sr[1] * n[1])) + F(sr[2] * n[2])) < 0:  # :99-105
            sr = tuple(F(v * F(-1.0)) for v in sr)
        tt = F(m["smoothness"] * spec)
        om = F(F(1.0) - tt)
        sray = normalized(tuple(F(F(sr[k] * om) + F(refl[k] * tt)) for k in range(3)))  # :175-176
        i, n2, p2, _ = scene.trace(offset(p, n), sray)  # :177
        if i < 0:  # :178-181
            e, ea = scene.environment(sray)
            L = [F(L[k] + F(e[k] * T[k])) for k in range(3)]
            with np.errstate(invalid="ignore"):
                alpha = F(ea * F(0.0))
            return L + [alpha], None
        n, p, m = n2, p2, scene.mat[i]
        spec = F(1.0) if m["specular"] >= rand_unit(key, draws) else F(0.0)  # :182
        draws += 1
        L = [F(L[k] + F(m["emissive"][k] * T[k])) for k in range(3)]  # :183
        ns = F(F(1.0) - spec)
        f = [F(F(m["base"][k] * ns) + F(m["spec_color"][k] * spec)) for k in range(3)]  # :184
        T = [F(T[k] * f[k]) for k in range(3)]
    g = F(F(1.0) - F(m["smoothness"] * spec))  # T3
    return L + [alpha], dict(x=p, n=n, T=T, g=g)


def lookup(grid, coefficients, x, n, flags=0, band_weight=HEMISPHERE_MEAN, depth=None, R=None, records=None, bias=0.0, min_variance=1e-4):
    """Rule T4 for points x (N, 3) and normals n (N, 3): ((N, 4) float32 of (M, a), corners, open), from the shading reference the
    flags select, with the points as the POSITION guide of a frame of one row of hits."""
    N = len(x)
    obj = np.zeros((1, N), np.int32)
    nd, pos = np.zeros((1, N, 4), F), np.zeros((1, N, 4), F)
    nd[0, :, :3], pos[0, :, :3] = n, x
    pgf = PG.NORMAL_WEIGHT if flags & NORMAL_WEIGHT else 0
    if flags & STATES:
        out, c = PS.shade(grid, coefficients, records, obj, nd, pos, flags=pgf, band_weight=band_weight, depth=depth if flags & DEPTH else None,
                          R=R, bias=bias, min_variance=min_variance)
        return out.reshape(N, 4), c["corners"], c["open"] if flags & DEPTH else c["corners"]
    if flags & DEPTH:
        out, c = PD.shade(grid, coefficients, depth, R, obj, nd, pos, flags=pgf, band_weight=band_weight, bias=bias, min_variance=min_variance)
        return out.reshape(N, 4), c["corners"], c["open"]
    out = PG.shade(grid, coefficients, obj, nd, pos, flags=pgf, band_weight=band_weight)
    live = int(PG.corners(grid, x, n, pgf)["live"].sum())
    return out.reshape(N, 4), live, live


def tails(terminals, grid, coefficients, **kw):
    """Rules T3 - T5 for a list of terminal states (None: no tail).  (addends (len, 3) float32 — k * M, zero where nothing is
    added —, adds (len,) bool, work dict(tails, corners, open, dark, mirror_ends))."""
    K = len(terminals)
    add, adds = np.zeros((K, 3), F), np.zeros(K, bool)
    term = [k for k, t in enumerate(terminals) if t is not None]
    look = [k for k in term if terminals[k]["g"] > 0]
    work = dict(tails=len(look), corners=0, open=0, dark=0, mirror_ends=len(term) - len(look))
    if not look:
        return add, adds, work
    x = np.array([terminals[k]["x"] for k in look], F)
    n = np.array([terminals[k]["n"] for k in look], F)
    Ma, work["corners"], work["open"] = lookup(grid, coefficients, x, n, **kw)
    for j, k in enumerate(look):
        if not Ma[j, 3] > 0:  # T4
            work["dark"] += 1
            continue
        t = terminals[k]
        for l in range(3):
            M = Ma[j, l] if Ma[j, l] > 0 else F(0.0)
            add[k, l] = F(F(F(t["T"][l] * F(0.8)) * t["g"]) * M)  # T5
        adds[k] = True
    return add, adds, work


def fold(acc, colour, frame, overwrite):
    """SetScreenPixel's running mean (radiance rule 3) of one float4 accumulator: weight = (float)(1.0 / frame)."""
    if overwrite:
        return [F(v) for v in colour]
    w = F(1.0 / float(int(frame)))
    om = F(F(1.0) - w)
    with np.errstate(invalid="ignore"):
        return [F(c0(F(F(acc[k]) * om)) + F(F(colour[k]) * w)) for k in range(4)]


def trace(scene, origins, directions, samples, max_bounces, seed=0, first_sample=1, id_base=0):
    """Every (ray, sample) of a batch: colours (N, samples, 4) float32 and the flat list of terminal states, ray-major."""
    N = len(origins)
    colours = np.zeros((N, samples, 4), F)
    terminals = []
    for i in range(N):
        for s in range(samples):
            colour, t = path(scene, origins[i][:3], directions[i][:3], max_bounces, seed, (id_base + i) & 0xFFFFFFFF, first_sample + s)
            colours[i, s] = colour
            terminals.append(t)
    return colours, terminals


def radiance(colours, first_sample=1, reset=True, acc=None, add=None):
    """The running means (N, 4) of colours (N, samples, 4), `add` (N * samples, 3) added to the colour lanes first (rule T5; rows
    where nothing is added are not touched: pass the `adds` mask with it as a tuple)."""
    N, S = colours.shape[:2]
    out = np.zeros((N, 4), F) if acc is None else np.array(acc, F)
    for i in range(N):
        a = list(out[i])
        for s in range(S):
            c = [F(v) for v in colours[i, s]]
            if add is not None and add[1][i * S + s]:
                c = [F(c[l] + add[0][i * S + s, l]) for l in range(3)] + [c[3]]
            a = fold(a, c, first_sample + s, reset and s == 0)
        out[i] = a
    return out
