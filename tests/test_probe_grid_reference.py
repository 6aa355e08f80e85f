"""The numpy reference of probe-grid shading (tests/probe_grid_reference.py) against what the rule must give on inputs with known
answers, and its probe positions against srt_probe_grid_positions bit for bit.  No device.

The bound 16 * 2^-24 (relative) used below: a weight product is two roundings and t_c * e_c one more, E and T take seven
additions each after the first, and the quotient one division — at most 16 half-ulps when every term has the same sign, which the
cases arrange (positive coefficients, e_c > 0 in every lane)."""
import ctypes as C

import numpy as np
import pytest

import light_probe_reference as LP
import probe_grid_reference as PG

F = np.float32
EPS = 2.0 ** -24
BOUND = 16 * EPS


def frame(points, normals):
    """A 1 x N frame of hit pixels at `points` with `normals`: (obj, nd, pos)."""
    p = np.asarray(points, F).reshape(-1, 3)
    n = np.asarray(normals, F).reshape(-1, 3)
    obj = np.zeros((1, len(p)), np.int32)
    nd = np.zeros((1, len(p), 4), F)
    pos = np.ones((1, len(p), 4), F)
    nd[0, :, :3], pos[0, :, :3] = n, p
    return obj, nd, pos


def positive_probe(rng):
    """Nine coefficients with a dominant band 0, so that the irradiance is positive in every lane at every normal."""
    c = rng.uniform(-0.05, 0.05, (9, 4)).astype(F)
    c[0] = rng.uniform(1.0, 2.0, 4).astype(F)
    return c


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


GRID = PG.Grid((-2.0, -1.0, 0.5), (0.75, 1.25, 0.5), (4, 3, 5))


def interior(rng, count):
    lo = GRID.origin.astype(np.float64) + 0.01
    hi = GRID.origin.astype(np.float64) + GRID.spacing.astype(np.float64) * (np.array(GRID.counts) - 1) - 0.01
    return rng.uniform(lo, hi, (count, 3)).astype(F)


def test_the_weights_of_an_interior_point_sum_to_one():
    rng = np.random.default_rng(1)
    x = interior(rng, 500)
    c = PG.corners(GRID, x, unit(rng.normal(size=(500, 3))))
    assert c["live"].all()
    total = c["t"].astype(np.float64).sum(axis=1)
    assert np.abs(total - 1.0).max() <= 8 * EPS
    # ... and the fourth lane of the output is that sum, added in ascending c
    obj, nd, pos = frame(x, unit(rng.normal(size=(500, 3))))
    out = PG.shade(GRID, np.ones((GRID.probes, 9, 4), F), obj, nd, pos)
    T = np.zeros(500, F)
    for k in range(8):
        T = (T + c["t"][:, k]).astype(F)
    assert np.array_equal(out[0, :, 3].view(np.uint32), T.view(np.uint32))


def test_equal_coefficients_at_all_probes_give_the_irradiance_of_one_probe():
    rng = np.random.default_rng(2)
    probe = positive_probe(rng)
    coeff = np.broadcast_to(probe, (GRID.probes, 9, 4)).copy()
    x, n = interior(rng, 300), unit(rng.normal(size=(300, 3)))
    obj, nd, pos = frame(x, n)
    for flags in (0, PG.NORMAL_WEIGHT):
        out = PG.shade(GRID, coeff, obj, nd, pos, flags=flags)
        for i in range(300):
            want = LP.irradiance(probe, n[i]).astype(np.float64)
            assert (want > 0).all()
            assert np.abs(out[0, i, :3].astype(np.float64) / want - 1.0).max() <= BOUND, (flags, i)


def test_an_affine_field_of_band_0_coefficients_is_reproduced():
    rng = np.random.default_rng(3)
    P = PG.positions(GRID)[:, :3].astype(np.float64)
    g = np.array([0.3, 0.2, 0.4])
    field = lambda p: 5.0 + p @ g  # positive over the grid
    coeff = np.zeros((GRID.probes, 9, 4), F)
    coeff[:, 0, :3] = field(P)[:, None].astype(F)
    x, n = interior(rng, 300), unit(rng.normal(size=(300, 3)))
    obj, nd, pos = frame(x, n)
    out = PG.shade(GRID, coeff, obj, nd, pos).astype(np.float64)
    a0 = float(F(3.14159274)) * float(F(0.282095))
    want = a0 * field(x.astype(np.float64))
    assert np.abs(out[0, :, 0] / want - 1.0).max() <= BOUND
    assert np.array_equal(out[0, :, 0], out[0, :, 1]) and np.array_equal(out[0, :, 0], out[0, :, 2])


def test_skipped_corners():
    n = unit([[0.0, 1.0, 0.0]])
    # a point exactly on a probe plane (x = origin + 1 * spacing): f_x = 0, the four corners with cx = 1 are skipped
    on_plane = [[-2.0 + 0.75, -0.3, 1.3]]
    c = PG.corners(GRID, on_plane, n)
    i, f = PG.cells(GRID, on_plane)
    assert tuple(i[0]) == (1, 0, 1) and f[0, 0] == 0.0
    assert list(c["live"][0]) == [k & 1 == 0 for k in range(8)]
    pix, corner, O4, D4 = PG.segments(GRID, *frame(on_plane, n))
    assert list(corner) == [0, 2, 4, 6] and len(O4) == 4
    # an axis with count 1: i = 0, f = 0, the corners with that bit do not exist
    flat = PG.Grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 4, 1))
    i, f = PG.cells(flat, [[0.4, 1.5, -3.0]])
    assert tuple(i[0]) == (0, 1, 0) and tuple(f[0]) == (0.0, 0.5, 0.0)
    c = PG.corners(flat, [[0.4, 1.5, -3.0]], n)
    assert list(np.flatnonzero(c["live"][0])) == [0, 2] and list(c["probe"][0, [0, 2]]) == [1, 2] and c["probe"].max() < flat.probes
    # clamping outside the grid: below gives cell 0 with f = 0, above the last cell with f = 1
    i, f = PG.cells(GRID, [[-50.0, 99.0, 0.6]])
    assert tuple(i[0]) == (0, 1, 0) and f[0, 0] == 0.0 and f[0, 1] == 1.0
    c = PG.corners(GRID, [[-50.0, 99.0, 0.6]], n)
    assert list(np.flatnonzero(c["live"][0])) == [2, 6] and c["probe"].min() >= 0 and c["probe"].max() < GRID.probes
    # a NaN position gives cell 0 with f = 0 on that axis
    i, f = PG.cells(GRID, [[np.nan, 0.0, np.nan]])
    assert tuple(i[0]) == (0, 0, 0) and f[0, 0] == 0.0 and f[0, 2] == 0.0
    # an occluded corner contributes nothing; all occluded gives (0, 0, 0, 0)
    obj, nd, pos = frame(on_plane, n)
    coeff = np.ones((GRID.probes, 9, 4), F)
    assert not PG.shade(GRID, coeff, obj, nd, pos, flags=PG.VISIBILITY, occluded=np.ones(4, np.int32)).view(np.uint32).any()
    some = PG.shade(GRID, coeff, obj, nd, pos, flags=PG.VISIBILITY, occluded=np.array([0, 1, 1, 0]))
    assert some[0, 0, 3] == c_sum(PG.corners(GRID, on_plane, n)["t"][0], [0, 6])
    # a miss pixel is (0, 0, 0, 0) whatever its other guides hold
    obj[0, 0] = -1
    pos[...] = np.nan
    assert not PG.shade(GRID, coeff, obj, nd, pos).view(np.uint32).any()


def c_sum(t, which):
    s = F(0.0)
    for k in range(8):
        s = F(s + (t[k] if k in which else F(0.0)))
    return s


def test_albedo_multiplies_after_the_division_and_hemisphere_weights_drop_band_2():
    rng = np.random.default_rng(4)
    coeff = np.stack([positive_probe(rng) for _ in range(GRID.probes)])
    x, n = interior(rng, 50), unit(rng.normal(size=(50, 3)))
    obj, nd, pos = frame(x, n)
    alb = rng.uniform(0.1, 0.9, (1, 50, 4)).astype(F)
    plain = PG.shade(GRID, coeff, obj, nd, pos)
    with_albedo = PG.shade(GRID, coeff, obj, nd, pos, albedo=alb, flags=PG.ALBEDO)
    assert np.array_equal(with_albedo[..., :3].view(np.uint32), (plain[..., :3] * alb[..., :3]).astype(F).view(np.uint32))
    assert np.array_equal(with_albedo[..., 3], plain[..., 3])
    no_band_2 = coeff.copy()
    no_band_2[:, 4:] = 7.0
    a = PG.shade(GRID, coeff, obj, nd, pos, band_weight=PG.HEMISPHERE)
    b = PG.shade(GRID, no_band_2, obj, nd, pos, band_weight=PG.HEMISPHERE)
    assert np.allclose(a, b, rtol=1e-6) and not np.array_equal(a, plain)


@pytest.mark.parametrize("grid", [GRID, PG.Grid((0.1, -0.7, 3.3), (0.3, 0.7, 1.1), (1, 4, 1)), PG.Grid((-1e3, 2.5, 1e-3), (1e-2, 3.0, 17.0), (7, 2, 3))])
def test_reference_positions_equal_the_library_s_bit_for_bit(srt, grid):
    got = srt.probe_grid_positions(grid.origin, grid.spacing, grid.counts)
    want = PG.positions(grid)
    assert got.shape == want.shape == (grid.probes, 4) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not got[:, 3].any()
    # probe (ix, iy, iz) sits at index ix + nx * (iy + ny * iz)
    nx, ny, nz = grid.counts
    k = (nx - 1) + nx * ((ny - 1) + ny * (nz - 1))
    for a, i in enumerate((nx - 1, ny - 1, nz - 1)):
        assert got[k, a] == F(grid.origin[a] + F(F(i) * grid.spacing[a]))
    g = srt.capi.ProbeGrid((C.c_float * 3)(*grid.origin), (C.c_float * 3)(*grid.spacing), (C.c_int32 * 3)(*grid.counts))
    assert np.array_equal(srt.capi.probe_grid_positions(g).view(np.uint32), want.view(np.uint32))
