"""numpy reference of the scrolling probe grid (include/srt_pathtrace.h, the block "scrolling probe grids"): rule SC1's index map,
rules SC2 and SC3 on arrays (bits move, nothing is computed), rule SC4's origin and rule SC7's follow shift.  The float rules are
single binary32 operations on binary32 operands in the header's order, so the tests compare bit for bit."""
import numpy as np

F = np.float32
U = np.uint32

COEFFICIENTS, MOMENTS, STATES = 1, 2, 4
COUNT_WORK, SET_GRID = 1, 2
FOLLOW_LIMIT = F(1048576.0)


def source_map(counts, shift):
    """Rule SC1 for every destination probe in index order ix + nx*(iy + ny*iz): (retained, source), bool and int64 per probe; the
    source of an exposed probe is -1.  Python integers: no shift overflows."""
    nx, ny, nz = (int(c) for c in counts)
    sx, sy, sz = (int(s) for s in shift)
    i = np.arange(nx * ny * nz, dtype=np.int64)
    ix, iy, iz = i % nx, (i // nx) % ny, i // (nx * ny)
    # (int64 + a Python int of at most 2^31 in magnitude: exact)
    jx, jy, jz = ix + sx, iy + sy, iz + sz
    retained = (jx >= 0) & (jx < nx) & (jy >= 0) & (jy < ny) & (jz >= 0) & (jz < nz)
    source = np.where(retained, jx + nx * (jy + ny * jz), -1)
    return retained, source


def scroll_array(array, counts, shift):
    """Rules SC2 / SC3 on one per-probe array (P, ...) of 32-bit elements: a new array with the bits of probe j at a retained i and
    zero bits at an exposed i."""
    a = np.ascontiguousarray(array)
    retained, source = source_map(counts, shift)
    assert a.shape[0] == retained.shape[0] and a.dtype.itemsize == 4
    bits = a.view(U)
    out = np.zeros_like(bits)
    out[retained] = bits[source[retained]]
    return out.view(a.dtype)


def work(counts, shift):
    """Rule SC6's counts: probes, retained, exposed."""
    retained, _ = source_map(counts, shift)
    return dict(probes=int(retained.shape[0]), retained=int(retained.sum()), exposed=int((~retained).sum()))


def scroll(counts, shift, coefficients=None, moments=None, states=None):
    """srt_scroll_probes on numpy arrays: coefficients (P, 9, 4), moments (P, R*R, 4), states (P, 4) — None: not selected.  Returns a
    dict: coefficients, moments (the histories after the call), previous (the previous records after the call), work."""
    out = dict(work=work(counts, shift))
    out["coefficients"] = None if coefficients is None else scroll_array(coefficients, counts, shift)
    out["moments"] = None if moments is None else scroll_array(moments, counts, shift)
    out["previous"] = None if states is None else scroll_array(states, counts, shift)
    return out


def scrolled_origin(origin, spacing, shift):
    """Rule SC4: origin_a + ((float)shift_a * spacing_a) in binary32, the product rounded first."""
    o = np.asarray(origin, dtype=F)
    s = np.asarray(spacing, dtype=F)
    k = np.array([F(int(v)) for v in shift], dtype=F)  # (float)int32: round to nearest even, as numpy's conversion from a Python int
    with np.errstate(over="ignore", invalid="ignore"):
        step = (k * s).astype(F)
        return (o + step).astype(F)


def follow(origin, spacing, counts, point):
    """Rule SC7: per axis c = origin + (((float)(n - 1)) * 0.5f) * spacing, u = (point - c) / spacing, clamped to +-1048576 and
    truncated towards zero; a NaN gives 0."""
    o, s, p = (np.asarray(v, dtype=F) for v in (origin, spacing, point))
    n1 = np.array([F(int(c) - 1) for c in counts], dtype=F)
    with np.errstate(over="ignore", invalid="ignore"):
        half = (n1 * F(0.5)).astype(F)
        c = (o + (half * s).astype(F)).astype(F)
        u = ((p - c).astype(F) / s).astype(F)
    out = []
    for v in u:
        if np.isnan(v):
            out.append(0)
            continue
        v = min(max(v, -FOLLOW_LIMIT), FOLLOW_LIMIT)
        out.append(int(np.trunc(v)))
    return tuple(out)
