"""tests/probe_depth_reference.py against itself and against float64: the octahedral encode inverts the texel table, the binary32
accumulation stays within a derived rounding bound of a float64 evaluation, the Fibonacci direction set leaves no texel without
weight, the texel rule's empty case, and rule 7b's weight on hand-made moments.  No GPU, no library."""
import numpy as np
import pytest

import light_probe_reference as LP
import probe_depth_reference as PD
import probe_grid_reference as PG

F = np.float32
EPS = float(np.finfo(F).eps) / 2  # unit roundoff of binary32


@pytest.mark.parametrize("R", PD.RESOLUTIONS)
def test_encode_of_a_texel_direction_is_the_texel(R):
    e = PD.texels(R)
    # rule 7b looks up q = -d: the direction from the probe towards the point
    tau = PD.encode(-e[:, :3], R)
    assert np.array_equal(tau, np.arange(R * R)), "%d mismatches" % int((tau != np.arange(R * R)).sum())


def test_encode_clamps_and_survives_values_that_are_not_finite():
    d = np.array([[0, 0, -1], [0, 0, 1], [-1, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [np.inf, 1, 1], [0, 0, 0]], dtype=F)
    for R in PD.RESOLUTIONS:
        tau = PD.encode(d, R)
        assert ((tau >= 0) & (tau < R * R)).all()
        assert tau[0] == (R // 2) * R + R // 2  # q = +z: u = v = 0 lies on the upper edge of texel R/2 - 1 ... it rounds into R/2


@pytest.mark.parametrize("R,s", [(4, 0), (8, 3), (16, 5), (16, 6)])
def test_the_reference_stays_within_the_rounding_bound_of_float64(R, s):
    """The bound, with u = 2^-24.  Every term w, w*r and w*(r*r) is >= 0, so a left-to-right binary32 sum of K terms adds a relative
    error of at most (K - 1) u.  A term: c is a three-term dot product of unit vectors, absolute error <= 3u, relative <= 6u where
    c >= 1/2 (directions with smaller c weigh c^(2^s) and do not matter in the sums); s squarings turn that into 2^s * 6u and add
    2^s - 1 roundings, so c^(2^s) carries 2^s * 7u; the weight, r*r and the product add three more.  A moment is a quotient of two
    such sums: twice the above and one rounding.  2 * (K + 7 * 2^s + 3) u + u, which the expression below covers."""
    K = 256
    d = LP.sphere(K)
    rng = np.random.default_rng(4)
    r = PD.clamp_distance(rng.uniform(-0.5, 9.0, (3, K)).astype(F), 6.0)
    got = PD.moments(d, r, R, s, 6.0).astype(np.float64)
    m1, m2, wt, ft = PD.moments64(d, r, R, s, 6.0)
    bound = 2.0 * (K + 2 * 7 * (2 ** s) + 6) * EPS
    for name, a, b in (("m1", got[..., 0], m1), ("m2", got[..., 1], m2), ("wt", got[..., 2], wt), ("ft", got[..., 3], ft)):
        err = np.abs(a - b) / np.maximum(np.abs(b), 1e-30)
        err = np.where(b == 0, np.abs(a), err)
        print("R %d s %d %s: max relative error %.3g, bound %.3g" % (R, s, name, err.max(), bound))
        assert err.max() <= bound, name


@pytest.mark.parametrize("s", range(7))
def test_every_texel_of_the_256_direction_set_has_weight(s):
    d = LP.sphere(256)
    r = np.full((1, 256), 1.0, F)
    for R in PD.RESOLUTIONS:
        m = PD.moments(d, r, R, s, 10.0)
        assert (m[..., 2] > 0).all()
        if s == 6 and R == 16:
            assert m[..., 2].min() * 256 / (4 * np.pi) > 1.0  # more than one direction's worth: the issue's prototype found 1.74
        # a constant distance has mean r, mean square r*r up to rounding, and nothing at max_distance
        assert np.allclose(m[..., 0], 1.0, rtol=1e-5) and np.allclose(m[..., 1], 1.0, rtol=1e-5) and not m[..., 3].any()


def test_one_direction_leaves_the_far_hemisphere_empty_and_far_rays_are_counted():
    d = LP.sphere(1)  # (1, 0, 0)
    m = PD.moments(d, np.array([[2.0], [7.0]], F), 8, 2, 5.0)
    e = PD.texels(8)
    empty = ~(e[:, 0] > 0)
    assert empty.any() and (~empty).any()
    assert (m[:, empty] == np.array([5.0, 25.0, 0.0, 1.0], F)).all()
    assert (m[0, ~empty, 0] == 2.0).all() and (m[0, ~empty, 1] == 4.0).all() and (m[0, ~empty, 3] == 0.0).all()
    r = PD.clamp_distance(np.array([[2.0], [7.0]], F), 5.0)
    m = PD.moments(d, r, 8, 2, 5.0)
    assert (m[1, ~empty, 0] == 5.0).all() and (m[1, ~empty, 3] == 1.0).all()
    assert PD.work_formula(2, 1, r, 5.0) == (2, 2, 1, 2)


def test_clamp_distance():
    t = np.array([-1.0, -0.0, 0.0, 1e-30, 3.0, 5.0, 5.5, np.inf, -np.inf, np.nan], F)
    assert PD.clamp_distance(t, 5.0).tolist() == [0.0, 0.0, 0.0, float(F(1e-30)), 3.0, 5.0, 5.0, 5.0, 0.0, 0.0]


def test_the_chebyshev_weight():
    t = np.full(5, 0.5, F)
    L = np.array([1.0, 2.0, 2.0, 3.0, 2.0], F)
    m1 = np.array([2.0, 2.0, 1.0, 1.0, 1.0], F)
    m2 = np.array([4.0, 4.0, 1.5, 1.0, 1.5], F)
    out, taken = PD.chebyshev(t, L, m1, m2, 0.0, 1e-4)
    assert taken.tolist() == [False, False, True, True, True]
    assert out[0] == out[1] == F(0.5)
    ch = F(0.5) / F(1.5)  # var 0.5, D 1
    assert out[2] == out[4] == F(F(0.5) * F(F(ch * ch) * ch))
    ch = F(1e-4) / F(F(1e-4) + F(4.0))  # var 0 -> the floor, D 2
    assert out[3] == F(F(0.5) * F(F(ch * ch) * ch))
    # a bias that covers the difference switches the test off
    out, taken = PD.chebyshev(t, L, m1, m2, 1.0, 1e-4)
    assert taken.tolist() == [False, False, False, True, False]


def test_shade_with_far_moments_is_the_untested_shading_and_near_moments_darken():
    grid = PG.Grid((-1.0, -1.0, 3.0), (2.0, 2.0, 2.0), (2, 2, 2))
    rng = np.random.default_rng(8)
    H, W = 4, 6
    obj = np.where(rng.random((H, W)) < 0.8, 0, -1).astype(np.int32)
    pos = np.ones((H, W, 4), F)
    pos[..., :3] = rng.uniform((-0.9, -0.9, 3.1), (0.9, 0.9, 4.9), (H, W, 3))
    n = rng.normal(size=(H, W, 3))
    nd = np.zeros((H, W, 4), F)
    nd[..., :3] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    coeff = rng.uniform(0.0, 2.0, (8, 9, 4)).astype(F)
    far = np.zeros((8, 16, 4), F)
    far[..., 0], far[..., 1] = 1e4, 1e8
    for flags in (0, PG.NORMAL_WEIGHT):
        plain = PG.shade(grid, coeff, obj, nd, pos, flags=flags)
        got, counts = PD.shade(grid, coeff, far, 4, obj, nd, pos, flags=flags)
        assert np.array_equal(got.view(np.uint32), plain.view(np.uint32))
        assert counts["taken"] == 0 and counts["open"] == counts["segments"] == counts["corners"] > 0 and counts["pixels"] == int((obj != -1).sum())
        near = np.zeros((8, 16, 4), F)
        near[..., 0], near[..., 1] = 0.1, 0.0101
        dark, counts = PD.shade(grid, coeff, near, 4, obj, nd, pos, flags=flags)
        hit = obj != -1
        assert counts["taken"] == counts["corners"] and (dark[hit][:, 3] < plain[hit][:, 3]).all() and (dark[hit][:, 3] > 0).all()
    with pytest.raises(AssertionError):
        PD.shade(grid, coeff, far, 4, obj, nd, pos, flags=PG.VISIBILITY)
