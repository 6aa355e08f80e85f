"""What the inputs of the probe sweep (tests/probe_fuzz_inputs.py) reach, counted on the CPU with the references alone over the default
keys of tests/test_gpu_probe_fuzz.py (two seeds per kind, "large", "large-mesh"): a sweep whose chains never reflect, whose probes
are all CLEAR, whose segments are all open or whose paths never end on a surface would pass without testing the edges it is there
for.  No GPU.  The tests print the counts; the bounds asserted are the conditions the sweep was specified with, not these counts.

The scenes are the query sweep's at seeds 7200 + 375 + key.  The shift was found by a scan of the scene seeds 0 .. 699 (140 per kind)
with this file's camera draws: 375 is the only multiple of five there at which the ten seeds meet every condition below at once.

Conditions that a kind cannot meet, and what is asserted instead:
  - `mixed`, reflection at thresholds 0.5: the issue excuses it.  A 30x or 300x sphere is the closest hit of every ray that passes
    it (Sphere::Raytrace reports the foot of the perpendicular, at a negative distance too), and few of them are smooth and specular
    at once: 2 of 140 `mixed` scenes have a chain of depth >= 2.  At thresholds 0 a `mixed` scene whose enlarged spheres are small
    does have them (21 of 140; key 3 is one), so that condition is asserted for `mixed` like for every other kind.
  - hit points outside `grid`, and pixels with a skipped corner, in `unit`, `far` and `tiny` (and `offset`): the objects are drawn
    within off +- 4 * scale with sizes up to 3 * scale and the grid spans off +- 6 * scale, so a primary hit point leaves it only on
    the far part of a large box: 8 of 420 scenes of the three kinds, 5 of 140 `offset` ones, none among the ten default seeds.
    A longer range of seeds would have to be a hundred scenes long per kind, so instead the shading and the tail test of the GPU
    sweep take five more keys, one per kind (probe_fuzz_inputs.CLAMP_KEYS, scene seeds 535, 501, 507, 698 and 389 of the scan), and the
    conditions are asserted over the default keys and these: every kind clamps on `grid`, and all six sides occur (the far side
    z > hi, which needs a hit beyond the volume along the camera's view, at `mixed` seed 698 alone of the 700).  On `flat`, which
    spans off +- 2.5 * scale, the default keys of every kind have hit points outside in x or z, and every hit pixel has skipped
    corners (n_y = 1 gives f_y = 0).
  - `large`: its kind has the two large keys; the 3400-sphere scene reflects, buries and occludes plenty.
  - the tail in `mixed`: excused by the issue (inside a 300x sphere next to nothing is diffuse-lit: the paths end in a sphere's
    negative-distance hit and go on); the mixed key with small enlarged spheres has terminal states all the same."""
import numpy as np
import pytest

import probe_fuzz_inputs as pf
import probe_grid_reference as PG
import probe_states_reference as PS

KEYS = list(range(pf.DEFAULT_SEEDS)) + list(pf.LARGE)
KINDS = pf.KINDS + ["large"]
NAMES = {PS.CLEAR: "CLEAR", PS.MOVED: "MOVED", PS.MOVED | PS.INSIDE: "MOVED|INSIDE", PS.BURIED | PS.INSIDE: "BURIED|INSIDE", PS.IDLE: "IDLE"}
SIDES = ("x<lo", "y<lo", "z<lo", "x>hi", "y>hi", "z>hi")


@pytest.fixture(scope="module")
def cases(oracle):
    return [pf.case(oracle, key) for key in KEYS]


def outside(c, grid):
    """Per side of `grid`, the number of the frame's hit points beyond it; and the number of hit pixels with a skipped corner."""
    x = c.pos[c.hit][:, :3]
    lo = grid.origin
    hi = lo + grid.spacing * (np.array(grid.counts, np.float32) - 1)
    sides = [int((x[:, a] < lo[a]).sum()) for a in range(3)] + [int((x[:, a] > hi[a]).sum()) for a in range(3)]
    live = PG.corners(grid, x, c.nd[c.hit][:, :3])["live"] if c.hits else np.ones((0, 8), bool)
    return sides, int((~live).any(axis=1).sum())


def by_kind(cases):
    return {k: [c for c in cases if c.kind == k] for k in KINDS}


def test_the_cases_have_their_shape(cases):
    assert [c.kind for c in cases[:5]] == pf.KINDS and [k % 5 for k in pf.CLAMP_KEYS] == [0, 1, 2, 3, 4]
    for base in (1000, 5000, 7200, 9000):  # the render sweep, the blocks sweep, the query sweep and the environments
        assert not set(pf.generator_of(key) for key in KEYS + list(pf.CLAMP_KEYS) + list(range(100))) & set(range(base, base + 1000))
    assert pf.SCENE_SHIFT % 5 == 0 and pf.SCENE_SHIFT + max(pf.CLAMP_KEYS) < 1000  # (the scenes stay the query sweep's)
    for c in cases:
        assert c.O4.shape == c.D4.shape == (pf.W * pf.H, 4) and pf.W % 8 and c.obj.shape == (pf.H, pf.W)
        assert c.grid.counts == (5, 4, 6) and c.flat.counts == (7, 1, 3) and len(set(c.grid.spacing.tolist())) == 3
        half = (c.grid.spacing * (np.array(c.grid.counts, np.float32) - 1)) / 2
        assert np.allclose(half, 6 * c.scale, rtol=1e-5) and np.allclose(c.grid.origin + half, c.off, rtol=1e-5, atol=1e-5 * c.scale)
        assert c.dirs.shape == c.scaled.shape == (65, 4)
        lengths = np.sqrt(pf.q.dd64(c.scaled[:, :3]))
        assert np.allclose(lengths[0::2], 0.5, atol=1e-6) and np.allclose(lengths[1::2], 3.0, atol=1e-5)
        assert c.probes.shape == (5, 4) and np.isfinite(c.probes).all()
        for grid, co, mo, rec in ((c.grid, c.co, c.mo, c.rec), (c.flat, c.flat_co, c.flat_mo, c.flat_rec)) + tuple(zip(c.cascade.grids, c.cas_co, c.cas_mo, c.cas_rec)):
            P = grid.probes
            assert co.shape == (P, 9, 4) and mo.shape == (P, 16, 4) and rec.shape == (P, 4) and np.isfinite(co).all()
            assert 1 <= int((~np.isfinite(mo[..., :2])).sum()) <= 6
            bits, moved = PS.state_bits(rec), np.abs(rec[:, :3]).max(axis=1) > 0
            assert np.isfinite(rec[:, :3]).all() and (np.abs(rec[:, :3]) <= 0.4501 * grid.spacing[None, :]).all()
            if P >= 100:  # records that are BURIED and MOVED, both with offsets that are not zero
                assert (((bits & PS.BURIED) != 0) & moved).sum() >= 5 and (((bits & PS.MOVED) != 0) & moved).sum() >= 10
                assert (((bits & PS.BURIED) != 0) & ~moved).sum() >= 5 and (bits == PS.CLEAR).sum() >= 10
        assert set(np.unique(c.budget)) <= set(pf.BUDGETS.tolist()) and len(np.unique(c.budget)) == 6
        assert c.cascade.levels == 2 and c.cascade.resolution == pf.R and float(c.cascade.blend_cells) == 1.0


def test_reflection_chains(cases, oracle):
    depth = {}
    for c in cases:
        for thr in ((0.5, 0.5), (0.0, 0.0)):
            J = pf.reflection(oracle, c, thr)["bounces"]
            depth[c.key, thr] = (int(J.max()), int((J >= 2).sum()))
            print("%-10s %-6s thresholds %.1f: deepest chain %d, %3d pixels of depth >= 2 (%d hit)" % ((c.key, c.kind, thr[0]) + depth[c.key, thr] + (c.hits,)))
    for k, cs in by_kind(cases).items():
        if k != "mixed":
            assert any(depth[c.key, (0.5, 0.5)][1] > 0 for c in cs), k
        if any(c.hits for c in cs):
            assert any(depth[c.key, (0.0, 0.0)][1] > 0 for c in cs), k
    assert any(d[0] == pf.MAX_BOUNCES for d in depth.values())


def test_classification_with_relocate(cases):
    seen, steps, all_buried = set(), set(), []
    for c in cases:
        r = pf.classified(c, "grid", "relocate")
        st, count = np.unique(r["state"], return_counts=True)
        c.states = set(int(s) for s in st)
        seen |= c.states
        steps |= set(np.unique(r["step"][(r["state"] & PS.MOVED) != 0]).tolist())
        flat = pf.classified(c, "flat", "relocate")
        print("%-10s %-6s %s; winning steps %s; flat %s" % (c.key, c.kind, ", ".join("%s %d" % (NAMES.get(int(s), s), n) for s, n in zip(st, count)),
                                                             np.bincount(r["step"])[1:].tolist(), np.bincount(flat["state"], minlength=9).tolist()))
        if c.states == {PS.BURIED | PS.INSIDE}:
            g = PG.positions(c.grid)[:, :3].astype(np.float64)
            inside = np.zeros(len(g), bool)
            for o in c.enlarged:
                inside |= np.linalg.norm(g - np.array(o["position"])[None, :], axis=1) < abs(o["radius"])
            all_buried.append(bool(inside.all()))
    # |radius|: the middle probe of some `flat` grid is inside a negative-radius sphere and outside everything else
    by_abs = []
    for c in cases:
        if c.negative:
            middle = PG.positions(c.flat)[[3 + 7 * 1], :3]
            rest = PS.primitives([o for o in c.objs if o.get("type", 0) != 0 and o not in c.negative])
            flat = pf.classified(c, "flat", "relocate")
            by_abs.append(bool(flat["s0"][10] < 0 and PS.scene_distance(rest, middle)[0] > flat["margin"] and flat["state"][10] & PS.INSIDE))
            print("%-10s %-6s flat grid about a sphere of radius %.3f: middle probe s0 %.3f, without that sphere %.3f, state %d" % (
                c.key, c.kind, c.negative[0]["radius"], flat["s0"][10], PS.scene_distance(rest, middle)[0], flat["state"][10]))
    assert any(by_abs)
    assert seen >= set(NAMES), sorted(seen)
    assert len(steps) > 1
    for k, cs in by_kind(cases).items():
        assert any(len(c.states) >= 2 for c in cs), k
    assert any(all_buried)  # every probe of some case inside a 300x sphere


def test_probe_grid_segments_and_the_cell_clamp(cases, oracle):
    extra = [pf.case(oracle, key) for key in pf.CLAMP_KEYS]
    for c in cases + extra:
        sides, skipped = outside(c, c.grid)
        c.sides, c.skipped = sides, skipped
        line = "%-10s %-6s grid: outside %s, %3d pixels with a skipped corner" % (c.key, c.kind, sides, skipped)
        if c.key not in pf.CLAMP_KEYS:
            _, _, _, _, occ = pf.grid_segments(oracle, c)
            c.open, c.occluded = int((occ == 0).sum()), int((occ != 0).sum())
            c.flat_sides, c.flat_skipped = outside(c, c.flat)
            line += "; segments open %4d occluded %4d; flat: outside %s, skipped %3d" % (c.open, c.occluded, c.flat_sides, c.flat_skipped)
        print(line)
    for k, cs in by_kind(cases).items():
        assert any(c.open > 0 and c.occluded > 0 for c in cs), k
        assert any(any(c.flat_sides[i] > 0 for i in (0, 2, 3, 5)) for c in cs) and any(c.flat_skipped == c.hits > 0 for c in cs), k
    for k in pf.KINDS:  # with the keys the shading test adds: every kind clamps on `grid`
        cs = [c for c in cases + extra if c.kind == k]
        assert any(any(c.sides) and c.skipped > 0 for c in cs), k
    for i, side in enumerate(SIDES):
        assert any(c.sides[i] > 0 for c in cases + extra), side


def test_tails_and_light_probes(cases, oracle):
    for c in cases:
        c.ends = {}
        for bounces in (1, 3):
            _, terminals = pf.paths(oracle, c, bounces, 2, c.seeds["tail"])
            c.ends[bounces] = sum(t is not None for t in terminals)
        idx, _ = pf.closest(oracle, c, c.probes[3:4], c.dirs)
        c.inside_hits = int((idx >= 0).sum())
        print("%-10s %-6s paths that end on a surface: %3d of %3d at 1 bounce, %3d at 3; camera probe %3d hits of 416; probe inside a sphere %d of 65" % (
            c.key, c.kind, c.ends[1], 2 * c.hits, c.ends[3], c.hits, c.inside_hits))
        assert c.has_inside and c.inside_hits == 65 and c.has_lifted
    for k, cs in by_kind(cases).items():
        if k != "mixed":
            assert any(c.ends[1] >= 0.1 * 2 * c.hits > 0 for c in cs) and any(c.ends[3] > 0 for c in cs), k
            assert any(0 < c.hits < pf.W * pf.H for c in cs), k
