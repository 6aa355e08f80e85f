"""The numpy reference of the light probes' projection (tests/light_probe_reference.py) and the two pure-host entries
(srt_light_probe_sphere, srt_light_probe_irradiance) against it.  No device: runs without a GPU."""
import numpy as np

import light_probe_reference as R

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def test_the_tree_is_order_sensitive():
    """1 + 2^-24 rounds back to 1 (ties to even), so a left-to-right sum of 1, 2^-24, 2^-24, ... never leaves 1; the pairwise tree
    first adds the small terms to each other.  The reference must give the tree's bits, not the loop's."""
    v = np.full((1, 64), F(2.0 ** -24), dtype=F)
    v[0, 0] = F(1.0)
    tree, loop = R.tree_sum(v), R.left_to_right_sum(v)
    assert loop[0] == F(1.0)
    assert tree[0] == F(1.0 + 62 * 2.0 ** -24) and tree[0] != loop[0]
    # across blocks the fold is ascending: B_0 = 1, then 64 * 2^-24 = 2^-18 per further block
    v = np.full((1, 130), F(2.0 ** -24), dtype=F)
    v[0, 0] = F(1.0)
    assert R.tree_sum(v)[0] == F(F(F(1.0 + 62 * 2.0 ** -24) + F(2.0 ** -18)) + F(2.0 ** -23))
    # positions past K contribute +0: K = 1 gives the value itself, -0 becomes +0
    assert bits(R.tree_sum(np.array([[F(-0.0)]], dtype=F)))[0] == 0
    assert R.tree_sum(np.array([[F(3.5)]], dtype=F))[0] == F(3.5)


def test_the_sphere_set_is_the_numpy_formula(srt):
    for k in (1, 64, 100):
        got, want = srt.light_probe_sphere(k), R.sphere(k)
        assert got.dtype == F and got.shape == (k, 4)
        assert np.abs(got[:, :3].astype(np.float64) - want[:, :3].astype(np.float64)).max() <= 2.0 ** -23
        assert np.array_equal(bits(got[:, 3]), bits(np.full(k, F(4.0 * np.pi / k), dtype=F)))
        assert np.abs(np.linalg.norm(got[:, :3].astype(np.float64), axis=1) - 1.0).max() < 1e-6


def test_the_irradiance_entry_gives_the_reference_bits(srt):
    rng = np.random.RandomState(7)
    for _ in range(50):
        c = (rng.standard_normal((9, 4)) * 3.0).astype(F)
        n = rng.standard_normal(3)
        n = (n / np.linalg.norm(n)).astype(F)
        got, want = srt.light_probe_irradiance(c, n), R.irradiance(c, n)
        assert np.array_equal(bits(got), bits(want)), (c, n, got, want)


def test_constant_radiance_projects_onto_the_constant_term(srt):
    k = 4096
    d = srt.light_probe_sphere(k)
    L = np.ones((1, k, 4), dtype=F)
    c = R.project(L, d)
    assert c.shape == (1, 9, 4) and c.dtype == F
    want = float(np.sum(d[:, 3].astype(np.float64) * float(F(0.282095))))
    assert abs(float(c[0, 0, 0]) - want) <= k * 2.0 ** -24 * abs(want)
    # L = 1: every rgb lane is 1 * t = t, so it equals the fourth lane bit for bit, in every coefficient
    for lane in range(3):
        assert np.array_equal(bits(c[0, :, lane]), bits(c[0, :, 3]))
    # the irradiance of constant radiance 1 is pi at any normal, up to the quadrature error of the Fibonacci set
    e = srt.light_probe_irradiance(c[0], d[17, :3])
    assert np.abs(e.astype(np.float64) - np.pi).max() < 1e-2
