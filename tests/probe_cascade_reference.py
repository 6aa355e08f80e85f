"""Probe-cascade shading as the header defines it (include/srt_pathtrace.h, the probe-cascade block, rules C1-C5 and C8), in numpy
float32 with one rounding per operation, built by COMPOSITION: per level the single-grid references give (I_l, T_l) —
probe_states_reference.shade with the level's records, probe_depth_reference.shade with moments alone, probe_grid_reference.shade
without either — on the pixels
that evaluate that level, without albedo; this file adds rule C2 (the level weights), rule C3 (the combination), rule C5 (the work
formulas) and rule C8 (the grids helper).  Not a test: tests/test_probe_cascade_abi.py and tests/test_gpu_probe_cascade.py import it."""
import numpy as np

import probe_depth_reference as PD
import probe_grid_reference as PG
import probe_states_reference as PS

F = np.float32
NORMAL_WEIGHT, DEPTH, STATES, ALBEDO, COUNT_WORK = 1, 2, 4, 8, 16
MAX_LEVELS = 4
# the class of a hit pixel: SINGLE + k: one evaluation, level k, the point inside it; BLENDED + k: levels k and k + 1; OUTSIDE: no
# level holds the point (one evaluation, the coarsest level through rule 2's clamp)
SINGLE, BLENDED, OUTSIDE = 0, 16, 32


class Cascade:
    def __init__(self, grids, blend_cells=1.0, resolution=0):
        self.grids = [g if isinstance(g, PG.Grid) else PG.Grid(*g) for g in grids]
        self.blend_cells = F(blend_cells)
        self.resolution = int(resolution)

    @property
    def levels(self):
        return len(self.grids)


def grids(centre, base_spacing, counts, levels):
    """Rule C8: the `levels` grids of srt_probe_cascade_grids as a Cascade (blend_cells 1, resolution 0)."""
    out = []
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for l in range(levels):
            origin, spacing = np.zeros(3, dtype=F), np.zeros(3, dtype=F)
            for a in range(3):
                sp = F(np.ldexp(F(base_spacing[a]), l))
                k = np.floor(F(F(centre[a]) / sp)).astype(F)
                k = F(0) if np.isnan(k) else min(max(k, F(-1048576.0)), F(1048576.0))
                origin[a] = F(F(k - F((int(counts[a]) - 1) // 2)) * sp)
                spacing[a] = sp
            out.append(PG.Grid(origin, spacing, counts))
    return Cascade(out, 1.0, 0)


def level_weight(grid, blend_cells, x):
    """Rule C2's beta_l for points x (N, 3): (N,) float32."""
    x = np.asarray(x, dtype=F).reshape(-1, 3)
    e = np.full(x.shape[0], np.inf, dtype=F)
    inside = np.ones(x.shape[0], bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for a in range(3):
            n = grid.counts[a]
            if n < 2:
                continue
            m = F(n - 1)
            u = ((x[:, a] - grid.origin[a]).astype(F) / grid.spacing[a]).astype(F)
            inside &= (u >= 0) & (u <= m)
            g = (m - u).astype(F)
            ea = np.where(u < g, u, g)
            e = np.where(ea < e, ea, e).astype(F)
        beta = np.where(e >= F(blend_cells), F(1.0), (e / F(blend_cells)).astype(F)).astype(F)
    return np.where(inside, beta, F(0.0)).astype(F)


def weights(cascade, x):
    """Rule C2 for points x (N, 3): (first_level (N,) int64, evaluations (N,) int64, beta (N,) float32 = beta of the first level,
    0 where no level holds the point)."""
    x = np.asarray(x, dtype=F).reshape(-1, 3)
    N, Lv = x.shape[0], cascade.levels
    f = np.full(N, -1, dtype=np.int64)
    beta = np.zeros(N, dtype=F)
    for l in range(Lv):
        b = level_weight(cascade.grids[l], cascade.blend_cells, x)
        take = (f < 0) & (b > 0)
        f[take], beta[take] = l, b[take]
    f[f < 0] = Lv - 1
    k = np.where((f == Lv - 1) | (beta >= 1), 1, 2).astype(np.int64)
    return f, k, beta


def classes(cascade, x):
    """The class of every point (see SINGLE, BLENDED, OUTSIDE)."""
    f, k, beta = weights(cascade, x)
    return np.where(k == 2, BLENDED + f, np.where(beta > 0, SINGLE + f, OUTSIDE))


def _level(grid, coefficients, records, moments, R, obj, nd, pos, flags, band_weight, bias, min_variance, rows):
    """(I, T) of one level as an (H, W, 4) image over the pixels of `obj` that are not -1, and (corners, open) of the band."""
    pflags = PG.NORMAL_WEIGHT if flags & NORMAL_WEIGHT else 0
    if not flags & (STATES | DEPTH):
        out = PG.shade(grid, coefficients, obj, nd, pos, flags=pflags, band_weight=band_weight)
        return out, PG.work_formula(grid, obj, nd, pos, pflags, rows=rows)[1], 0
    if not flags & STATES:
        out, c = PD.shade(grid, coefficients, moments, R, obj, nd, pos, flags=pflags, band_weight=band_weight, bias=bias, min_variance=min_variance, rows=rows)
    else:
        out, c = PS.shade(grid, coefficients, records, obj, nd, pos, flags=pflags, band_weight=band_weight, depth=moments if flags & DEPTH else None, R=R,
                          bias=bias, min_variance=min_variance, rows=rows)
    return out, c["corners"], c["open"]


def shade(cascade, coefficients, obj, nd, pos, records=None, moments=None, albedo=None, flags=0, band_weight=PG.IRRADIANCE, bias=0.0, min_variance=1e-4,
          rows=None):
    """srt_shade_probe_cascade over a whole frame: ((H, W, 4) float32, work, info).  coefficients / records / moments: one array per
    level.  work: the counts of rule C5 over the band `rows` of MEMORY rows, without the waves.  info: per hit pixel (in index
    order) pix, first_level, evaluations, beta, cls (classes()), usable (N, 2) bool: whether the first and the second evaluation
    were usable (the second False where there is none)."""
    obj = np.asarray(obj)
    H, W = obj.shape
    Lv = cascade.levels
    out = np.zeros((H, W, 4), dtype=F)
    pix = np.flatnonzero(obj.reshape(-1) != -1)
    y0, y1 = (0, H) if rows is None else (H - rows[1], H - rows[0])
    x = np.asarray(pos, dtype=F).reshape(-1, 4)[pix, :3]
    f, k, beta = weights(cascade, x)
    in_band = (pix // W >= y0) & (pix // W < y1)
    # rule C5: the trips of the band's tiles
    Qimg = np.zeros(H * W, dtype=np.int64)
    Qimg[pix] = k
    Qimg = Qimg.reshape(H, W)[y0:y1]
    trips = sum((int(Qimg[ty:ty + 8, tx:tx + 8].sum()) + 7) // 8 for ty in range(0, y1 - y0, 8) for tx in range(0, W, 8))
    work = dict(pixels=int(in_band.sum()), evaluations=int(k[in_band].sum()), blended=int((k[in_band] == 2).sum()),
                first_level=[int((f[in_band] == l).sum()) for l in range(MAX_LEVELS)], corners=0, open=0, wave_trips=trips)
    # rule C1 per level, on the pixels that evaluate it
    I = np.zeros((len(pix), 2, 4), dtype=F)
    for l in range(Lv):
        uses = np.where(f == l, 0, np.where((k == 2) & (f + 1 == l), 1, -1))
        if not (uses >= 0).any():
            continue
        o = np.full(H * W, -1, dtype=np.int32)
        o[pix[uses >= 0]] = 0
        img, n_corners, n_open = _level(cascade.grids[l], coefficients[l], records[l] if records is not None else None,
                                        moments[l] if moments is not None else None, cascade.resolution, o.reshape(H, W), nd, pos, flags, band_weight, bias,
                                        min_variance, rows)
        work["corners"] += n_corners
        work["open"] += n_open
        sel = uses >= 0
        I[sel, uses[sel]] = img.reshape(-1, 4)[pix[sel]]
    # rule C3
    ua = I[:, 0, 3] > 0
    ub = (k == 2) & (I[:, 1, 3] > 0)
    with np.errstate(invalid="ignore", over="ignore"):
        gb = (F(1.0) - beta).astype(F)
        mix = ((beta[:, None] * I[:, 0]).astype(F) + (gb[:, None] * I[:, 1]).astype(F)).astype(F)
        rgba = np.where((ua & ub)[:, None], mix, np.where(ua[:, None], I[:, 0], np.where(ub[:, None], I[:, 1], F(0.0)))).astype(F)
        if flags & ALBEDO:
            a = np.asarray(albedo, dtype=F).reshape(-1, 4)[pix, :3]
            rgba[:, :3] = np.where((ua | ub)[:, None], (rgba[:, :3] * a).astype(F), rgba[:, :3])
    out.reshape(-1, 4)[pix] = rgba
    info = dict(pix=pix, first_level=f, evaluations=k, beta=beta, cls=np.where(k == 2, BLENDED + f, np.where(beta > 0, SINGLE + f, OUTSIDE)),
                usable=np.stack([ua, ub], axis=1), in_band=in_band)
    return out, work, info
