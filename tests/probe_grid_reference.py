"""Probe-grid shading as the header defines it (include/srt_pathtrace.h, the probe-grid block, rules 1-9), in numpy float32 with
one rounding per operation: the cell of a point, the eight corner weights, the probe positions, the segments to the probes, the
normal weight, the corner irradiance (light_probe_reference.basis, the band weights as arguments) and the sum.  The visibility
answers are an INPUT: segments() says which segments (O, d, L) the rule wants answered, in (pixel, corner) order, and shade()
takes one occluded flag per segment.  Not a test: tests/test_probe_grid_reference.py and tests/test_gpu_probe_grid.py import it."""
import numpy as np

import light_probe_reference as LP

F = np.float32
VISIBILITY, NORMAL_WEIGHT, ALBEDO, COUNT_WORK = 1, 2, 4, 8
IRRADIANCE = (F(3.14159274), F(2.09439516), F(0.785398185))
HEMISPHERE = (F(1.0), F(0.5), F(0.0))
CORNER_BITS = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], dtype=np.int64)  # (8, 3): cx, cy, cz


class Grid:
    def __init__(self, origin, spacing, counts):
        self.origin = np.asarray(origin, dtype=F)
        self.spacing = np.asarray(spacing, dtype=F)
        self.counts = tuple(int(c) for c in counts)

    @property
    def probes(self):
        return self.counts[0] * self.counts[1] * self.counts[2]


def positions(grid):
    """(nx*ny*nz, 4) float32: p_a = origin_a + (float)i_a * spacing_a, index ix + nx*(iy + ny*iz), w = 0 (rule 4)."""
    nx, ny, nz = grid.counts
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    out = np.zeros((grid.probes, 4), dtype=F)
    for a, i in enumerate((ix, iy, iz)):
        out[:, a] = grid.origin[a] + (i.reshape(-1).astype(F) * grid.spacing[a]).astype(F)
    return out


def cells(grid, x):
    """Rule 2 on points x (N, 3): (i (N, 3) int64, f (N, 3) float32)."""
    x = np.asarray(x, dtype=F).reshape(-1, 3)
    i = np.zeros(x.shape, dtype=np.int64)
    f = np.zeros(x.shape, dtype=F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for a in range(3):
            n = grid.counts[a]
            m = F(n - 1)
            u = ((x[:, a] - grid.origin[a]).astype(F) / grid.spacing[a]).astype(F)
            u = np.where(~(u > 0), F(0), np.where(u > m, m, u)).astype(F)
            ia = u.astype(np.int64)  # (truncation of a value in [0, n - 1])
            if n >= 2:
                ia = np.minimum(ia, n - 2)
            i[:, a] = ia
            f[:, a] = (u - ia.astype(F)).astype(F)
    return i, f


def corners(grid, x, n, flags=0):
    """Rules 3-6 for points x (N, 3) with normals n (N, 3).  A dict of (N, 8) arrays: t (the weight, after the normal weight with
    NORMAL_WEIGHT), live (not skipped by rules 3 and 5), probe (the index, clamped to the grid), and O (N, 3), d (N, 8, 3), L (N, 8)."""
    x = np.asarray(x, dtype=F).reshape(-1, 3)
    n = np.asarray(n, dtype=F).reshape(-1, 3)
    i, f = cells(grid, x)
    N = x.shape[0]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        w = np.empty((N, 8, 3), dtype=F)
        for a in range(3):
            one_minus = (F(1.0) - f[:, a]).astype(F)
            w[:, :, a] = np.where(CORNER_BITS[None, :, a] == 1, f[:, None, a], one_minus[:, None])
        t = ((w[:, :, 0] * w[:, :, 1]).astype(F) * w[:, :, 2]).astype(F)
        live = t > 0
        idx = i[:, None, :] + CORNER_BITS[None, :, :]  # (N, 8, 3)
        p = np.empty((N, 8, 3), dtype=F)
        for a in range(3):
            p[:, :, a] = grid.origin[a] + (idx[:, :, a].astype(F) * grid.spacing[a]).astype(F)
        O = (x + (n * F(.00001)).astype(F)).astype(F)
        v = (p - O[:, None, :]).astype(F)
        q = ((v[..., 0] * v[..., 0]).astype(F) + (v[..., 1] * v[..., 1]).astype(F)).astype(F)
        q = (q + (v[..., 2] * v[..., 2]).astype(F)).astype(F)
        L = np.sqrt(q).astype(F)
        live = live & (L > 0)
        d = (v / L[..., None]).astype(F)
        if flags & NORMAL_WEIGHT:
            dn = ((d[..., 0] * n[:, None, 0]).astype(F) + (d[..., 1] * n[:, None, 1]).astype(F)).astype(F)
            dn = (dn + (d[..., 2] * n[:, None, 2]).astype(F)).astype(F)
            h = ((dn + F(1.0)).astype(F) * F(0.5)).astype(F)
            t = (t * ((h * h).astype(F) + F(0.2)).astype(F)).astype(F)
    nx, ny, nz = grid.counts
    k = [np.clip(idx[:, :, a], 0, grid.counts[a] - 1) for a in range(3)]
    probe = k[0] + nx * (k[1] + ny * k[2])
    return dict(t=t, live=live, probe=probe, O=O, d=d, L=L)


def corner_irradiance(coefficients, probe, n, band_weight=IRRADIANCE):
    """Rule 8: e (N, 8, 3) float32 from coefficients (P, 9, 4), probe indices (N, 8) and normals (N, 3)."""
    c = np.asarray(coefficients, dtype=F).reshape(-1, LP.COEFFS, 4)
    b = LP.basis(np.asarray(n, dtype=F).reshape(-1, 3))  # (N, 9)
    A = [F(band_weight[0])] + [F(band_weight[1])] * 3 + [F(band_weight[2])] * 5
    k = c[probe]  # (N, 8, 9, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        e = ((A[0] * k[:, :, 0, :3]).astype(F) * b[:, None, 0, None]).astype(F)
        for j in range(1, LP.COEFFS):
            e = (e + ((A[j] * k[:, :, j, :3]).astype(F) * b[:, None, j, None]).astype(F)).astype(F)
    return e


def segments(grid, obj, nd, pos, flags=0):
    """The segments the rule wants answered, in (pixel index, corner) order: (pix (S,), corner (S,), O4 (S, 4), D4 (S, 4) with
    t_max = L in w) — the live corners of every hit pixel, whatever `flags` says about VISIBILITY."""
    pix = np.flatnonzero(np.asarray(obj).reshape(-1) != -1)
    x = np.asarray(pos, dtype=F).reshape(-1, 4)[pix, :3]
    n = np.asarray(nd, dtype=F).reshape(-1, 4)[pix, :3]
    c = corners(grid, x, n, flags)
    r, k = np.nonzero(c["live"])
    O4 = np.zeros((len(r), 4), dtype=F)
    D4 = np.zeros((len(r), 4), dtype=F)
    O4[:, :3] = c["O"][r]
    D4[:, :3] = c["d"][r, k]
    D4[:, 3] = c["L"][r, k]
    return pix[r], k, O4, D4


def shade(grid, coefficients, obj, nd, pos, albedo=None, flags=0, band_weight=IRRADIANCE, occluded=None):
    """Rules 1-9 over a whole frame: (H, W, 4) float32.  `occluded`: with VISIBILITY, one flag per segment of segments(), in its
    order (non-zero: occluded)."""
    obj = np.asarray(obj)
    out = np.zeros(obj.shape + (4,), dtype=F)
    pix = np.flatnonzero(obj.reshape(-1) != -1)
    if len(pix) == 0:
        return out
    x = np.asarray(pos, dtype=F).reshape(-1, 4)[pix, :3]
    n = np.asarray(nd, dtype=F).reshape(-1, 4)[pix, :3]
    c = corners(grid, x, n, flags)
    ok = c["live"].copy()
    if flags & VISIBILITY:
        occ = np.asarray(occluded).reshape(-1) != 0
        assert occ.shape[0] == int(c["live"].sum())
        r, k = np.nonzero(c["live"])
        ok[r[occ], k[occ]] = False
    e = corner_irradiance(coefficients, c["probe"], n, band_weight)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        E = np.zeros((len(pix), 3), dtype=F)
        T = np.zeros(len(pix), dtype=F)
        for k in range(8):
            term = np.where(ok[:, k, None], (c["t"][:, k, None] * e[:, k, :]).astype(F), F(0.0)).astype(F)
            E = (E + term).astype(F)
            T = (T + np.where(ok[:, k], c["t"][:, k], F(0.0)).astype(F)).astype(F)
        good = T > 0
        rgba = np.zeros((len(pix), 4), dtype=F)
        rgba[good, :3] = (E[good] / T[good, None]).astype(F)
        rgba[good, 3] = T[good]
        if flags & ALBEDO:
            a = np.asarray(albedo, dtype=F).reshape(-1, 4)[pix, :3]
            rgba[good, :3] = (rgba[good, :3] * a[good]).astype(F)
    out.reshape(-1, 4)[pix] = rgba
    return out


def work_formula(grid, obj, nd, pos, flags=0, occluded=None, rows=None):
    """(pixels, corners, segments, open, wave_trips) of a call by the header's rule 17; `rows`: a band of MEMORY rows (tiles start
    at the band's first scene row).  `occluded` as for shade()."""
    obj = np.asarray(obj)
    H, W = obj.shape
    y0, y1 = (0, H) if rows is None else (H - rows[1], H - rows[0])
    pix, _, _, _ = segments(grid, obj, nd, pos, flags)
    in_band = (pix // W >= y0) & (pix // W < y1)
    hit = (obj != -1)[y0:y1]
    trips = 0
    for ty in range(0, y1 - y0, 8):
        for tx in range(0, W, 8):
            trips += (int(hit[ty:ty + 8, tx:tx + 8].sum()) + 7) // 8
    n_corners = int(in_band.sum())
    if flags & VISIBILITY:
        occ = np.asarray(occluded).reshape(-1) != 0
        return int(hit.sum()), n_corners, n_corners, int((~occ[in_band]).sum()), trips
    return int(hit.sum()), n_corners, 0, 0, trips
