"""Probe depth moments and the filtered probe-grid shading as the header defines them (include/srt_pathtrace.h, the probe-depth
block's rules 1-4 and the filtered-shading block's rule 7b), in numpy float32 with one rounding per operation: the texel table,
the clamp of a distance, the accumulation in ascending k, the texel, the octahedral encode, the Chebyshev weight, and shade() on
top of tests/probe_grid_reference.py.  The distances are an INPUT (srt_trace_rays answers them).  moments64() is the same sum in
float64 for the error-bound test.  Not a test: tests/test_probe_depth_reference.py, tests/test_probe_depth_abi.py and the GPU
tests import it."""
import numpy as np

import probe_grid_reference as PG

F = np.float32
MOMENTS, DISTANCES = 1, 2
NORMALIZE, COUNT_WORK = 1, 2
RESOLUTIONS = (4, 8, 16)


def sgn(x):
    """+1 for a number >= 0, otherwise -1 (a NaN gives -1)."""
    return np.where(x >= 0, 1.0, -1.0).astype(np.asarray(x).dtype)


def texels(R):
    """Rule 1: (R*R, 4) float32, texel (i, j) at index j*R + i; computed in double, each component rounded once."""
    j, i = np.meshgrid(np.arange(R, dtype=np.float64), np.arange(R, dtype=np.float64), indexing="ij")
    u = (2.0 * i + 1.0) / R - 1.0
    v = (2.0 * j + 1.0) / R - 1.0
    z = 1.0 - np.abs(u) - np.abs(v)
    x = np.where(z < 0, (1.0 - np.abs(v)) * sgn(u), u)
    y = np.where(z < 0, (1.0 - np.abs(u)) * sgn(v), v)
    n = np.sqrt(x * x + y * y + z * z)
    out = np.zeros((R * R, 4), dtype=F)
    out[:, 0], out[:, 1], out[:, 2] = (x / n).reshape(-1), (y / n).reshape(-1), (z / n).reshape(-1)
    return out


def clamp_distance(t, max_distance):
    """Rule 2: r = !(t > 0) ? 0 : (t > max_distance ? max_distance : t)."""
    t = np.asarray(t, dtype=F)
    m = F(max_distance)
    with np.errstate(invalid="ignore"):
        return np.where(~(t > 0), F(0), np.where(t > m, m, t)).astype(F)


def moments(directions, r, R, sharpness, max_distance):
    """Rules 3 and 4: (P, R*R, 4) float32 from the directions AS TRACED (K, 4) (weight in w) and the clamped distances r (P, K)."""
    d = np.asarray(directions, dtype=F)
    r = np.asarray(r, dtype=F)
    e = texels(R)
    P, K = r.shape
    T = R * R
    m = F(max_distance)
    M1 = np.zeros((P, T), dtype=F)
    M2 = np.zeros((P, T), dtype=F)
    Wt = np.zeros((P, T), dtype=F)
    Ft = np.zeros((P, T), dtype=F)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for k in range(K):
            c = ((e[:, 0] * d[k, 0]).astype(F) + (e[:, 1] * d[k, 1]).astype(F)).astype(F)
            c = (c + (e[:, 2] * d[k, 2]).astype(F)).astype(F)
            on = c > 0  # (T,)
            w = c.copy()
            for _ in range(int(sharpness)):
                w = (w * w).astype(F)
            w = (w * d[k, 3]).astype(F)
            rk = r[:, k]  # (P,)
            rr = (rk * rk).astype(F)
            wr = (w[None, :] * rk[:, None]).astype(F)
            wrr = (w[None, :] * rr[:, None]).astype(F)
            M1 = np.where(on[None, :], (M1 + wr).astype(F), M1)
            M2 = np.where(on[None, :], (M2 + wrr).astype(F), M2)
            Wt = np.where(on[None, :], (Wt + w[None, :]).astype(F), Wt)
            far = on[None, :] & (rk >= m)[:, None]
            Ft = np.where(far, (Ft + w[None, :]).astype(F), Ft)
        out = np.empty((P, T, 4), dtype=F)
        good = Wt > 0
        safe = np.where(good, Wt, F(1))
        out[..., 0] = np.where(good, (M1 / safe).astype(F), m)
        out[..., 1] = np.where(good, (M2 / safe).astype(F), F(m * m))
        out[..., 2] = np.where(good, Wt, F(0))
        out[..., 3] = np.where(good, (Ft / safe).astype(F), F(1))
    return out


def moments64(directions, r, R, sharpness, max_distance):
    """The same sums in float64 on the same float32 inputs: (M1/Wt, M2/Wt, Wt, Ft/Wt) and the sum of |terms| per lane, for the bound."""
    d = np.asarray(directions, dtype=F).astype(np.float64)
    r = np.asarray(r, dtype=F).astype(np.float64)
    e = texels(R).astype(np.float64)
    c = e[:, :3] @ d[:, :3].T  # (T, K)
    w = np.where(c > 0, c, 0.0) ** (2 ** int(sharpness)) * d[None, :, 3]
    Wt = w.sum(axis=1)
    M1 = r @ w.T
    M2 = (r * r) @ w.T
    Ft = (r >= float(F(max_distance))).astype(np.float64) @ w.T
    return M1 / Wt, M2 / Wt, Wt[None, :].repeat(r.shape[0], 0), Ft / Wt


def encode(d, R):
    """Rule 7b's texel lookup for the direction d (N, 3) from the point to the probe (q = -d): tau (N,) int64."""
    d = np.asarray(d, dtype=F).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = (-d).astype(F)
        s = ((np.abs(q[:, 0]) + np.abs(q[:, 1])).astype(F) + np.abs(q[:, 2])).astype(F)
        u = (q[:, 0] / s).astype(F)
        v = (q[:, 1] / s).astype(F)
        u2 = ((F(1) - np.abs(v)).astype(F) * sgn(u)).astype(F)
        v2 = ((F(1) - np.abs(u)).astype(F) * sgn(v)).astype(F)
        fold = q[:, 2] < 0
        u, v = np.where(fold, u2, u).astype(F), np.where(fold, v2, v).astype(F)
        idx = []
        for g in (u, v):
            a = (((g * F(0.5)).astype(F) + F(0.5)).astype(F) * F(R)).astype(F)
            a = np.where(~(a > 0), F(0), np.where(a > F(R - 1), F(R - 1), a)).astype(F)
            idx.append(a.astype(np.int64))
    return idx[1] * R + idx[0]


def chebyshev(t, L, m1, m2, bias, min_variance):
    """Rule 7b's weight on arrays of one shape: (t after the rule, whether the branch L > m1 + bias was taken)."""
    t, L, m1, m2 = (np.asarray(a, dtype=F) for a in (t, L, m1, m2))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        taken = L > (m1 + F(bias)).astype(F)
        var = np.abs((m2 - (m1 * m1).astype(F)).astype(F)).astype(F)
        var = np.where(var > F(min_variance), var, F(min_variance)).astype(F)
        dl = (L - m1).astype(F)
        ch = (var / (var + (dl * dl).astype(F)).astype(F)).astype(F)
        t2 = (t * ((ch * ch).astype(F) * ch).astype(F)).astype(F)
    return np.where(taken, t2, t).astype(F), taken


def shade(grid, coefficients, depth, R, obj, nd, pos, albedo=None, flags=0, band_weight=PG.IRRADIANCE, bias=0.0, min_variance=1e-4, rows=None):
    """srt_shade_probe_grid_depth over a whole frame: ((H, W, 4) float32, counts).  `depth`: (P, R*R, 4) moments.  counts: a dict of
    pixels, corners, segments, open, wave_trips for the band `rows` of MEMORY rows (default: the frame), and `taken`, the corners
    of the band that took the L > m1 + bias branch."""
    assert not flags & PG.VISIBILITY
    obj = np.asarray(obj)
    H, W = obj.shape
    depth = np.asarray(depth, dtype=F).reshape(grid.probes, R * R, 4)
    out = np.zeros(obj.shape + (4,), dtype=F)
    pix = np.flatnonzero(obj.reshape(-1) != -1)
    y0, y1 = (0, H) if rows is None else (H - rows[1], H - rows[0])
    hit = (obj != -1)[y0:y1]
    trips = sum((int(hit[ty:ty + 8, tx:tx + 8].sum()) + 7) // 8 for ty in range(0, y1 - y0, 8) for tx in range(0, W, 8))
    counts = dict(pixels=int(hit.sum()), corners=0, segments=0, open=0, wave_trips=trips, taken=0)
    if len(pix) == 0:
        return out, counts
    x = np.asarray(pos, dtype=F).reshape(-1, 4)[pix, :3]
    n = np.asarray(nd, dtype=F).reshape(-1, 4)[pix, :3]
    c = PG.corners(grid, x, n, flags)
    live = c["live"]
    tau = encode(c["d"].reshape(-1, 3), R).reshape(live.shape)
    mo = depth[c["probe"], tau]  # (N, 8, 4)
    t, taken = chebyshev(c["t"], c["L"], mo[..., 0], mo[..., 1], bias, min_variance)
    with np.errstate(invalid="ignore"):
        ok = live & (t > 0)
    in_band = ((pix // W >= y0) & (pix // W < y1))[:, None]
    counts["corners"] = counts["segments"] = int((live & in_band).sum())
    counts["open"] = int((ok & in_band).sum())
    counts["taken"] = int((live & taken & in_band).sum())
    e = PG.corner_irradiance(coefficients, c["probe"], n, band_weight)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        E = np.zeros((len(pix), 3), dtype=F)
        T = np.zeros(len(pix), dtype=F)
        for k in range(8):
            term = np.where(ok[:, k, None], (t[:, k, None] * e[:, k, :]).astype(F), F(0.0)).astype(F)
            E = (E + term).astype(F)
            T = (T + np.where(ok[:, k], t[:, k], F(0.0)).astype(F)).astype(F)
        good = T > 0
        rgba = np.zeros((len(pix), 4), dtype=F)
        rgba[good, :3] = (E[good] / T[good, None]).astype(F)
        rgba[good, 3] = T[good]
        if flags & PG.ALBEDO:
            a = np.asarray(albedo, dtype=F).reshape(-1, 4)[pix, :3]
            rgba[good, :3] = (rgba[good, :3] * a[good]).astype(F)
    out.reshape(-1, 4)[pix] = rgba
    return out, counts


def work_formula(P, K, r, max_distance):
    """(probes, rays, far_rays, wave_calls) of a trace by rule 8."""
    return P, P * K, int((np.asarray(r, dtype=F) >= F(max_distance)).sum()), P * ((K + 63) // 64)
