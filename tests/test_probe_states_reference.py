"""tests/probe_states_reference.py against float64 yardsticks: its INSIDE set is the containment test of tools/probe_depth_leak.py,
every MOVED probe clears the margin and stays within max_offset of the spacing, a probe stays BURIED only if a float64 search over
the same candidates finds none, IDLE probes are never used by the shading reference, and the synthetic room holds every state.
No compute on a device: runs without a GPU."""
import numpy as np
import pytest

import probe_grid_reference as PG
import probe_states_reference as PS

F = np.float32
SCENES = {
    "room": (PS.synthetic_room, PS.room_grid()),
    "room_coarse": (PS.synthetic_room, PS.room_grid(1.0, (5, 5, 5))),
    "mixed": (lambda: PS.synthetic_room()[6:] + [dict(type=PS.MESH, position=(0.0, 0.0, 0.0), mesh=0), dict(type=0, position=(0.0, 1.0, 3.0), radius=9.0)],
              PG.Grid((-3.0, -1.3, 1.9), (0.7, 0.45, 0.6), (8, 7, 6))),
}


@pytest.fixture(scope="module", params=sorted(SCENES))
def case(request):
    make, grid = SCENES[request.param]
    objs = make()
    d = PS.sphere_directions(256)
    return objs, grid, d, PS.classify(grid, objs), PS.classify(grid, objs, d, PS.RELOCATE)


def test_inside_is_the_float64_containment_test_away_from_surfaces(case):
    objs, grid, _, rest, moved = case
    prims = PS.primitives(objs)
    g = PG.positions(grid)[:, :3]
    far = np.abs(PS.scene_distance64(prims, g)) > 1e-4
    want = PS.inside64(prims, g)
    assert far.sum() > 0.9 * len(g) and want[far].any() and not want[far].all()
    for r in (rest, moved):
        got = (r["state"] & PS.INSIDE) != 0
        assert np.array_equal(got[far], want[far])
    # without relocation INSIDE and BURIED are the same set, nothing moves and every offset is 0
    assert np.array_equal((rest["state"] & PS.BURIED) != 0, (rest["state"] & PS.INSIDE) != 0)
    assert not (rest["state"] & PS.MOVED).any() and not rest["records"][:, :3].any() and rest["work"]["candidates"] == 0


def test_moved_probes_clear_the_margin_and_stay_in_their_neighbourhood(case):
    objs, grid, _, _, r = case
    prims = PS.primitives(objs)
    moved = (r["state"] & PS.MOVED) != 0
    assert moved.sum() >= 5
    x = r["positions"][moved, :3]
    assert (PS.scene_distance64(prims, x) >= float(r["margin"]) - 1e-5).all()
    o = r["records"][moved, :3].astype(np.float64)
    assert (np.abs(o) <= 0.45 * grid.spacing.astype(np.float64)[None, :] + 1e-6).all() and (np.abs(o).max(axis=1) > 0).all()
    still = ~moved
    assert not r["records"][still, :3].any() and np.array_equal(r["positions"][still, :3], PG.positions(grid)[still, :3])
    assert not r["positions"][:, 3].any()


def test_a_probe_stays_buried_only_if_no_candidate_clears_the_margin_in_float64(case):
    objs, grid, d, _, r = case
    prims = PS.primitives(objs)
    g = PG.positions(grid)[:, :3]
    buried = np.flatnonzero((r["state"] & PS.BURIED) != 0)
    assert len(buried) >= 1 and ((r["state"][buried] & PS.INSIDE) != 0).all() and not (r["state"][buried] & PS.MOVED).any()
    for m in range(1, 9):
        _, x = PS.candidates(grid, g[buried], d[:, :3], F(F(m) * r["dt"]))
        assert not (PS.scene_distance64(prims, x) >= float(r["margin"]) + 1e-5).any(), m
    # MOVED and BURIED exclude each other; IDLE stands alone
    st = r["state"]
    assert not ((st & PS.MOVED) != 0)[(st & PS.BURIED) != 0].any() and (st[(st & PS.IDLE) != 0] == PS.IDLE).all()


def test_the_room_holds_every_state_and_a_late_step():
    r = PS.classify(PS.room_grid(), PS.synthetic_room(), PS.sphere_directions(256), PS.RELOCATE)
    st = r["state"]
    for bit in (PS.MOVED, PS.BURIED, PS.INSIDE, PS.IDLE):
        assert int(((st & bit) != 0).sum()) >= 5, bit
    assert int((st == PS.CLEAR).sum()) >= 5 and int((r["step"] > 1).sum()) >= 1
    assert r["work"]["candidates"] % 256 == 0 and r["work"]["probes"] == 729


def test_a_mesh_switches_idle_off_and_contributes_no_distance():
    objs = PS.synthetic_room()
    grid = PS.room_grid()
    a = PS.classify(grid, objs)
    b = PS.classify(grid, objs + [dict(type=PS.MESH, position=(0.0, 1.0, 3.0), mesh=0)])
    assert (a["state"] & PS.IDLE).any() and not (b["state"] & PS.IDLE).any()
    assert np.array_equal(a["state"] & ~np.uint32(PS.IDLE), b["state"]) and np.array_equal(a["s0"].view(np.uint32), b["s0"].view(np.uint32))


def test_the_order_of_the_objects_and_a_nan_object_change_nothing():
    objs = PS.synthetic_room()
    grid = PS.room_grid()
    d = PS.sphere_directions(65)
    a = PS.classify(grid, objs, d, PS.RELOCATE)
    nan = dict(type=PS.SPHERE, position=(float("nan"), 0.0, 0.0), radius=1.0)
    b = PS.classify(grid, [nan] + objs[::-1], d, PS.RELOCATE)
    assert np.array_equal(a["records"].view(np.uint32), b["records"].view(np.uint32))
    # normalising unit directions scaled by two gives the offsets of the unit directions up to rounding; without it they double
    d2 = d.copy()
    d2[:, :3] *= 2
    c = PS.classify(grid, objs, d2, PS.RELOCATE | PS.NORMALIZE)
    assert np.allclose(c["records"][:, :3], PS.classify(grid, objs, d, PS.RELOCATE | PS.NORMALIZE)["records"][:, :3], atol=1e-6)


def test_no_corner_that_enters_a_sum_belongs_to_an_idle_probe():
    """IDLE says: no first-hit point on an analytic surface lies in one of the probe's eight cells.  Points on the room's surfaces,
    shaded with the records: no corner with weight > 0 is an IDLE probe."""
    objs, grid = PS.synthetic_room(), PS.room_grid()
    r = PS.classify(grid, objs, PS.sphere_directions(256), PS.RELOCATE)
    prims = PS.primitives(objs)
    rng = np.random.default_rng(5)
    lo = grid.origin.astype(np.float64)  # (points of the grid's own volume: beyond it the cell index is clamped, and a cell says nothing)
    x = rng.uniform(lo, lo + 8 * grid.spacing.astype(np.float64), (400000, 3)).astype(F)
    near = np.abs(PS.scene_distance64(prims, x)) < 2e-3  # points within 2 mm of a surface stand for the surface
    x = x[near]
    assert len(x) > 500
    n = np.tile(np.array([[0.0, 1.0, 0.0]], dtype=F), (len(x), 1))
    c = PS.corners(grid, r["records"], x, n)
    weighted = c["probe"][(c["weight"] > 0).all(axis=2)]
    idle = (r["state"] & PS.IDLE) != 0
    assert idle.sum() >= 5 and not idle[weighted].any()
