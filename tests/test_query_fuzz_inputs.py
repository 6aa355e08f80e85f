"""What the inputs of the ray-query sweep (tests/query_fuzz_inputs.py) reach, counted on the CPU with the oracle alone over the
default seeds of tests/test_gpu_query_fuzz.py: a sweep whose rays all miss, never start inside a sphere or never meet a triangle
would pass without testing the bounds it is there for.  No GPU.

The counts at SEED_BASE = 7200 (20 seeds, four per kind, 1910 rays each) are printed by the tests; the bounds asserted are the
conditions the sweep was specified with, not these counts.  Every condition can be met.  Two of them decided the recipe of
family E and the seed base.  A scene has a mesh with probability 1/2 and its triangles are slivers: with E aimed at the
positions of mesh objects `unit` had 78 triangle hits at base 7000, so E aims at triangle centres.  Sphere::Raytrace reports a
hit, at a negative distance, wherever the foot of the perpendicular lies inside the sphere, so a 300x sphere is the closest hit
of every ray that passes it: `mixed` hits something else only in scenes whose enlarged spheres are small (18 such hits at base
7000, 14 at 7400, 819 at 7200)."""
import numpy as np
import pytest

import query_fuzz_inputs as q


@pytest.fixture(scope="module")
def cases(oracle):
    return [q.case(oracle, seed) for seed in range(q.DEFAULT_SEEDS)]


@pytest.fixture(scope="module")
def counts(cases):
    tot = {}

    def add(kind, what, n):
        tot[kind, what] = tot.get((kind, what), 0) + int(n)

    for c in cases:
        idx, _, _, t = c.ref
        hit, k = idx >= 0, c.kind
        occluded, opened = np.zeros(len(idx), bool), np.zeros(len(idx), bool)
        for name in q.FINITE_SETS:
            if name in c.tmax:
                w = q.want(c, name)
                occluded |= w == 1
                opened |= w == 0
        triangle = hit & np.isin(idx, c.mesh_objects)
        add(k, "hit", hit.sum()), add(k, "miss", (~hit).sum()), add(k, "negative", (hit & (t < 0)).sum())
        add(k, "occluded", occluded.sum()), add(k, "open", opened.sum()), add(k, "triangle", triangle.sum())
        if "segment" in c.tmax:
            add(k, "C triangle occluder", (triangle & (c.family == 2) & (q.want(c, "segment") == 1)).sum())
        add(k, "E hit", (hit & (c.family == 4)).sum()), add(k, "E miss", (~hit & (c.family == 4)).sum())
        add(k, "window hit", (hit & (c.tag == q.WINDOW)).sum())
        add(k, "not enlarged", (hit & ~np.isin(idx, c.enlarged)).sum())
    for key in sorted(tot):
        print("%-8s %-22s %d" % (key + (tot[key],)))
    return tot


def test_seed_bases_are_apart_and_the_cases_have_their_shape(cases):
    assert q.DEFAULT_SEEDS == 20 and [c.kind for c in cases[:5]] == q.KINDS
    for base in (1000, 5000, 9000):  # the render sweep, the blocks sweep, the environments
        assert not set(range(q.SEED_BASE, q.SEED_BASE + 1000)) & set(range(base, base + 1000))
    for c in cases:
        n = len(c.O4)
        assert 1500 <= n <= 2500 and c.O4.shape == c.D4.shape == (n, 4) and c.O4.dtype == c.D4.dtype == np.float32
        assert np.isfinite(c.O4).all() and np.abs(c.O4).max() < 1e29
        assert any(int((c.family == f).sum()) % 64 for f in range(5))
        assert set(c.tmax) >= {"+inf", "t", "above t", "below t", "0", "-0", "t/2", "NaN", "-inf", "uniform"}
        assert all(v.dtype == np.float32 and v.shape == (n,) for v in c.tmax.values())
        assert np.signbit(c.tmax["-0"]).all() and not np.signbit(c.tmax["0"]).any()
        d = c.D4[:, :3]
        assert not np.isinf(d).any() and (np.isnan(d) | (d != 0)).any(axis=1).all()  # no infinite component, no all-zero direction


def test_direction_edges_of_every_family(cases):
    for c in cases:
        d, dd = c.D4[:, :3], q.dd64(c.D4[:, :3])
        for f in np.unique(c.family):
            rows = c.family == f
            k = int(rows.sum()) // 10
            assert (c.tag[rows] == q.WINDOW).sum() == k and (c.tag[rows] == q.ZERO).sum() == k and (c.tag[rows] == q.NAN).sum() == 2
            assert (c.tag[rows] == q.OUTSIDE).sum() == (0 if c.triangles else k)
            assert (c.tag[rows] == q.LENGTH).sum() == (0 if c.triangles else 6)
        assert np.all(np.abs(dd[c.tag == q.PLAIN] - 1) < 4e-7)
        w = dd[c.tag == q.WINDOW] - 1
        assert np.all((np.abs(w) > 0.65e-6) & (np.abs(w) < 0.95e-6)) and (w > 0).any() and (w < 0).any()  # inside |d.d - 1| <= 1e-6
        o = dd[c.tag == q.OUTSIDE] - 1
        assert np.all((np.abs(o) > 1.3e-6) & (np.abs(o) < 1.7e-6))  # outside it
        z = d[c.tag == q.ZERO]
        zeros = (z == 0).sum(axis=1)
        assert np.all((zeros >= 1) & (zeros <= 2)) and np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
        assert np.all(np.isnan(d[c.tag == q.NAN]).sum(axis=1) == 1) and not np.isnan(d[c.tag != q.NAN]).any()
        for i in np.flatnonzero(c.tag == q.NAN):  # a healthy lane in the same 64-ray block
            block = np.arange(i // 64 * 64, min(i // 64 * 64 + 64, len(d)))
            assert (c.tag[block] != q.NAN).sum() >= 32
        if not c.triangles:
            lengths = np.sqrt(dd[c.tag == q.LENGTH])
            assert np.all((np.abs(lengths - 0.5) < 1e-6) | (np.abs(lengths - 3) < 1e-5)) and (lengths < 1).any() and (lengths > 1).any()


def test_family_c_starts_on_surfaces_and_family_d_inside_spheres(cases, oracle):
    for c in cases:
        if "segment" in c.tmax:
            seg = c.tmax["segment"][c.family == 2]
            assert np.isfinite(seg).all() and (seg > 0).all() and c.p2p.sum() > 150 and (~c.p2p).sum() > 150
        rows = np.flatnonzero(c.family == 3)
        if len(rows):  # inside some sphere, |o - centre| < |r| (in `offset` binary32 origins move by up to a sixth of the smallest radius)
            sph = [o for o in c.objs if o.get("type") == oracle.OBJ_SPHERE]
            cen, rad = np.array([o["position"] for o in sph], np.float32), np.array([abs(o["radius"]) for o in sph])
            dist = np.linalg.norm(c.O4[rows, None, :3].astype(np.float64) - cen[None].astype(np.float64), axis=2)
            assert (dist < rad[None]).any(axis=1).mean() > 0.97


def test_every_kind_hits_misses_and_starts_inside_a_sphere(counts):
    for k in q.KINDS:
        for what in ("hit", "miss", "negative", "occluded", "open"):
            assert counts[k, what] >= 100, (k, what)


def test_triangles_are_closest_hits_and_occluders_of_family_c(counts, cases):
    for k in ("unit", "tiny", "offset"):  # (`far`: the triangle window ends at t = 10 000, a few rays of C and D alone meet one)
        assert counts[k, "triangle"] >= 100 and counts[k, "C triangle occluder"] >= 20, k
    assert any(c.broken_mesh for c in cases) and any(c.has_none for c in cases)


def test_the_shell_family_hits_and_misses_far_from_the_origin(counts):
    for k in ("far", "offset"):
        assert counts[k, "E hit"] >= 100 and counts[k, "E miss"] >= 100 and counts[k, "window hit"] >= 50, k


def test_mixed_scenes_have_misses_and_hits_beside_the_enlarged_spheres(counts, cases):
    assert counts["mixed", "miss"] >= 100 and counts["mixed", "not enlarged"] >= 50
    # the enlarged and the negative-radius spheres are among the origins of D
    assert any(len(c.enlarged) for c in cases if c.kind == "mixed")
    assert any(o.get("radius", 0) < 0 for c in cases if c.kind == "mixed" for o in c.objs)


def test_the_large_cases(oracle):
    for key in q.LARGE:
        c = q.case(oracle, key)
        idx, _, _, t = c.ref
        hit = idx >= 0
        assert c.n == 3461 + (key == "large-mesh") and c.triangles == (key == "large-mesh") and 1500 <= len(idx) <= 2500
        assert hit.sum() >= 100 and (~hit).sum() >= 100 and (hit & (t < 0)).sum() >= 100
        if c.triangles:
            assert np.isin(idx, c.mesh_objects).sum() >= 100
