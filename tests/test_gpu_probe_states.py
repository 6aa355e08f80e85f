"""Probe classification and relocation (srt_classify_probes, ABI 7) on the MI355X.  Every comparison is bit for bit over the records
(offset and state bits), the positions and the work counts against tests/probe_states_reference.py, which measures every candidate
against every primitive in numpy float32: a synthetic room that holds every state, Scene1, the mesh scene (never IDLE); grids of
one probe, of odd counts and of more probes than resident waves; K around the wave width; bound outputs; errors in order; a scene
update; and the positions bound device to device as light-probe positions."""
import ctypes as C

import numpy as np
import pytest

import probe_grid_reference as PG
import probe_states_reference as PS
from test_gpu_probe_grid import SENTINEL, same
from test_gpu_visibility import mesh_scene, scene1

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 24, 20
KEYS = ("probes", "inside", "moved", "buried", "idle", "candidates")


def tracer(srt, oracle, scene):
    objs, meshes = scene
    pt = srt.PathTracer(W, H)
    keep = None
    if meshes:
        marr, mn, keep = oracle.make_meshes(meshes)
        pt.set_meshes(C.cast(marr, C.POINTER(srt.Mesh)), mn)
    oarr, n = oracle.make_objects(objs)
    pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
    pt._keep = (oarr, keep)
    return pt


def check(srt, pt, objs, grid, K=None, flags=0, directions=None, **kw):
    """One counting call with both outputs against the reference; returns the reference's dict."""
    relocate = bool(flags & PS.RELOCATE)
    d = directions if directions is not None else (srt.light_probe_sphere(K) if K else None)
    want = PS.classify(grid, objs, d, flags, **{k: (F(v) if k != "steps" else v) for k, v in kw.items()})
    pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
    pt.classify_probes(directions=d if relocate else None, relocate=relocate, normalize=bool(flags & PS.NORMALIZE), count_work=True, positions=True, **kw)
    rec, pos, work = pt.probe_states_output("records"), pt.probe_states_output("positions"), pt.probe_states_work()
    print("counts %s K %s flags %d %s: work %s, winning steps %s" % (grid.counts, K, flags, kw, work, np.bincount(want["step"]).tolist()))
    bad = (rec.view(np.uint32) != want["records"].view(np.uint32)).any(axis=1)
    assert same(rec, want["records"]), "records differ at %d probes, first %s" % (int(bad.sum()), np.flatnonzero(bad)[:5])
    assert same(pos, want["positions"])
    assert work["valid"] == 1 and work["waves"] > 0 and {k: work[k] for k in KEYS} == want["work"]
    return want


@pytest.fixture(scope="module")
def room(srt, oracle):
    objs = PS.synthetic_room()
    pt = tracer(srt, oracle, (objs, None))
    yield pt, objs
    pt.close()


# ---- the synthetic room: every state, K around the wave width, one step and eight ---------------------------------------------------
@pytest.mark.parametrize("K", [1, 63, 64, 65, 256])
@pytest.mark.parametrize("steps", [1, 8])
def test_the_room_with_relocation(srt, room, K, steps):
    pt, objs = room
    want = check(srt, pt, objs, PS.room_grid(), K, PS.RELOCATE, steps=steps)
    if K == 256 and steps == 8:  # the condition on the inputs: every state occurs, and a search that ends after the first step
        st = want["state"]
        for bit in (PS.MOVED, PS.BURIED, PS.INSIDE, PS.IDLE):
            assert int(((st & bit) != 0).sum()) >= 5, bit
        assert int((st == PS.CLEAR).sum()) >= 5 and int((want["step"] > 1).sum()) >= 1


def test_the_room_without_relocation_normalised_directions_and_other_parameters(srt, room):
    pt, objs = room
    grid = PS.room_grid()
    rest = check(srt, pt, objs, grid)
    assert rest["work"]["moved"] == 0 and rest["work"]["candidates"] == 0 and rest["work"]["buried"] == rest["work"]["inside"] >= 5
    d = srt.light_probe_sphere(65)
    d[:, :3] *= np.random.default_rng(3).uniform(0.25, 3.0, (65, 1)).astype(F)
    d[7, :3] = 0.0  # normalises to NaN: never accepted
    a = check(srt, pt, objs, grid, 65, PS.RELOCATE | PS.NORMALIZE, directions=d)
    b = check(srt, pt, objs, grid, 65, PS.RELOCATE, directions=d)
    assert not same(a["records"], b["records"])
    c = check(srt, pt, objs, grid, 256, PS.RELOCATE, clearance=0.3, max_offset=0.25, steps=3)
    assert c["work"]["moved"] != a["work"]["moved"]
    check(srt, pt, objs, grid, 256, PS.RELOCATE, clearance=0.5, max_offset=0.5, steps=64)


@pytest.mark.parametrize("counts,spacing,K", [((4, 3, 5), 0.9, 65), ((1, 1, 1), 0.5, 64), ((17, 18, 17), 0.24, 64)])
def test_other_grids(srt, room, counts, spacing, K):
    """(17, 18, 17): 5202 probes, more than the 4096 waves of 1024 resident workgroups: waves take a second probe."""
    pt, objs = room
    want = check(srt, pt, objs, PS.room_grid(spacing, counts), K, PS.RELOCATE)
    assert want["work"]["probes"] == counts[0] * counts[1] * counts[2]
    if counts == (1, 1, 1):
        pt.set_probe_grid((1.4, 0.4, 4.1), (0.5, 0.5, 0.5), counts)  # the centre of the big sphere: buried, whatever the directions
        pt.classify_probes(relocate=True, count_work=True)
        assert PS.state_bits(pt.probe_states_output())[0] == PS.BURIED | PS.INSIDE and pt.probe_states_work()["candidates"] == 8 * K


def test_a_table_too_large_for_lds_is_read_from_memory(srt, oracle):
    """2100 small spheres beyond the room's walls besides the room: more than the 2048 rows the kernel stages into LDS."""
    rng = np.random.default_rng(9)
    far = [dict(type=PS.SPHERE, position=tuple(float(v) for v in p), radius=0.05) for p in rng.uniform((-3.0, 4.0, 0.0), (3.0, 9.0, 6.0), (2100, 3))]
    objs = PS.synthetic_room() + far
    pt = tracer(srt, oracle, (objs, None))
    try:
        grid = PS.room_grid(0.9, (4, 3, 5))
        big = check(srt, pt, objs, grid, 65, PS.RELOCATE)
        small = PS.classify(grid, PS.synthetic_room(), srt.light_probe_sphere(65), PS.RELOCATE)
        assert same(big["records"], small["records"])  # (the far spheres decide nothing: both tables give the room's states)
    finally:
        pt.close()


# ---- the scenes of the other probe tests ----------------------------------------------------------------------------------------------
def test_scene1_and_the_mesh_scene_where_no_probe_is_idle(srt, oracle):
    objs, _ = scene1(oracle)
    pt = tracer(srt, oracle, (objs, None))
    try:
        grid = PG.Grid((-4.0, -1.5, 1.0), (0.5, 0.5, 0.5), (9, 9, 9))
        want = check(srt, pt, objs, grid, 256, PS.RELOCATE)
        assert want["work"]["inside"] >= 5 and want["work"]["moved"] >= 1
        check(srt, pt, objs, grid)
    finally:
        pt.close()
    objs, meshes = mesh_scene(oracle)
    pt = tracer(srt, oracle, (objs, meshes))
    try:
        grid = PG.Grid((-2.0, -2.2, 3.0), (0.5, 0.5, 0.5), (9, 9, 9))
        for flags in (0, PS.RELOCATE):
            want = check(srt, pt, objs, grid, 128, flags)
            assert want["work"]["idle"] == 0 and want["work"]["inside"] >= 5
        no_mesh = PS.classify(grid, objs[1:])
        assert no_mesh["work"]["idle"] >= 1  # the same probes without the mesh object: some would be idle
    finally:
        pt.close()


# ---- outputs, counting, determinism -------------------------------------------------------------------------------------------------
def test_bound_outputs_counting_off_and_repeated_calls(srt, room):
    import torch

    pt, objs = room
    grid = PS.room_grid(0.9, (4, 3, 5))
    P = grid.probes
    d = srt.light_probe_sphere(63)
    want = check(srt, pt, objs, grid, 63, PS.RELOCATE, directions=d)
    dev = "cuda:%d" % pt.device
    rec = torch.full((P + 3, 4), SENTINEL, dtype=torch.float32, device=dev)
    pos = torch.full((P + 5, 4), SENTINEL, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    try:
        pt.bind_probe_states_output("records", rec)
        pt.bind_probe_states_output("positions", pos)
        for _ in range(2):  # COUNT_WORK off: the same bits, twice
            pt.classify_probes(relocate=True, positions=True)
            pt.wait()
            r, p = rec.cpu().numpy(), pos.cpu().numpy()
            assert same(r[:P], want["records"]) and same(p[:P], want["positions"]) and np.all(r[P:] == SENTINEL) and np.all(p[P:] == SENTINEL)
            assert same(pt.probe_states_output("records"), want["records"]) and same(pt.probe_states_output("positions"), want["positions"])
        with pytest.raises(srt.SrtError):
            pt.probe_states_work()  # the last call did not count
        # RECORDS alone: the bound positions stay untouched, and reading them is refused
        pos.fill_(SENTINEL)
        torch.cuda.synchronize()
        pt.classify_probes(relocate=True, count_work=True)
        pt.wait()
        assert np.all(pos.cpu().numpy() == SENTINEL) and same(rec.cpu().numpy()[:P], want["records"])
        with pytest.raises(srt.SrtError):
            pt.probe_states_output("positions")
        assert {k: pt.probe_states_work()[k] for k in KEYS} == want["work"]
    finally:
        pt.wait()
        pt.bind_probe_states_output("records", None)
        pt.bind_probe_states_output("positions", None)
    # back on the own buffers
    pt.classify_probes(relocate=True, positions=True)
    assert same(pt.probe_states_output("records"), want["records"]) and same(pt.probe_states_output("positions"), want["positions"])


def test_the_states_follow_an_update_of_the_scene(srt, oracle):
    objs = PS.synthetic_room()
    pt = tracer(srt, oracle, (objs, None))
    try:
        grid = PS.room_grid()
        before = check(srt, pt, objs, grid, 64, PS.RELOCATE)
        moved = [dict(o) for o in objs]
        moved[6]["position"] = (0.9, 1.6, 1.7)  # the big box
        oarr, n = oracle.make_objects(moved)
        pt.update_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
        after = check(srt, pt, moved, grid, 64, PS.RELOCATE)
        assert not same(before["records"], after["records"])
        pt.set_scene(C.cast(oracle.make_objects(objs)[0], C.POINTER(srt.Object)), n)
        again = check(srt, pt, objs, grid, 64, PS.RELOCATE)
        assert same(again["records"], before["records"])
    finally:
        pt.close()


# ---- the positions, bound device to device as light-probe positions -------------------------------------------------------------------
def test_positions_bound_as_light_probe_positions_give_the_depth_maps_of_the_reference_s_positions(srt, room):
    import torch

    pt, objs = room
    grid = PS.room_grid(0.9, (4, 3, 5))
    P = grid.probes
    d = srt.light_probe_sphere(64)
    want = PS.classify(grid, objs, d, PS.RELOCATE)
    assert want["work"]["moved"] >= 3
    pt.trace_probe_depth(want["positions"], d, resolution=8, sharpness=4, max_distance=3.0)  # the reference's positions, written from the host
    depth = pt.probe_depth_output("moments")
    pos = torch.zeros((P, 4), dtype=torch.float32, device="cuda:%d" % pt.device)
    try:
        pt.bind_probe_states_output("positions", pos)
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        pt.classify_probes(directions=d, relocate=True, positions=True)
        pt.trace_probe_depth(pos, None, resolution=8, sharpness=4, max_distance=3.0)  # bound: nothing crosses the bus
        assert same(pt.probe_depth_output("moments"), depth)
        at_rest = PG.positions(grid)
        pt.trace_probe_depth(at_rest, None, resolution=8, sharpness=4, max_distance=3.0)
        assert not same(pt.probe_depth_output("moments"), depth)
    finally:
        pt.wait()
        pt.bind_probe_states_output("positions", None)


# ---- errors -----------------------------------------------------------------------------------------------------------------------------
def test_errors_come_in_order_and_touch_nothing(srt, oracle):
    c = srt.capi
    objs = PS.synthetic_room()
    oarr, n = oracle.make_objects(objs)
    pt = srt.PathTracer(W, H)
    L = pt.L
    nan, inf = float("nan"), float("inf")

    def call(**kw):
        p = c.ProbeClassifyParams()
        assert L.srt_probe_classify_params_default(C.byref(p)) == c.OK
        for k, v in kw.items():
            setattr(p, k, v)
        return L.srt_classify_probes(pt._h, C.byref(p))

    def why():
        return L.srt_last_error(pt._h)

    try:
        assert call(flags=8) == c.ERR_STATE and b"srt_set_scene" in why()
        pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
        for kw in (dict(flags=8), dict(flags=0x80000000), dict(outputs=0), dict(outputs=4), dict(clearance=0.0), dict(clearance=-0.1), dict(clearance=0.6),
                   dict(clearance=nan), dict(clearance=inf), dict(max_offset=0.0), dict(max_offset=0.51), dict(max_offset=nan), dict(steps=0), dict(steps=65),
                   dict(reserved=1)):
            assert call(**kw) == c.ERR_INVALID_ARG, kw
        assert call() == c.ERR_STATE and b"no grid" in why()
        assert call(steps=0, flags=c.PROBE_CLASSIFY_RELOCATE) == c.ERR_INVALID_ARG  # the arguments before the grid
        pt.set_probe_grid((-2.05, -1.3, 0.4), (0.5, 0.5, 0.5), (9, 9, 9))
        assert call(flags=c.PROBE_CLASSIFY_RELOCATE) == c.ERR_STATE and b"directions" in why()
        buf = np.empty((729, 4), F)
        assert L.srt_read_probe_states_output(pt._h, 1, buf.ctypes.data_as(C.c_void_p)) == c.ERR_STATE  # nothing was touched
        assert L.srt_read_probe_states_output(pt._h, 3, buf.ctypes.data_as(C.c_void_p)) == c.ERR_INVALID_ARG
        assert L.srt_bind_probe_states_output(pt._h, 3, None) == c.ERR_INVALID_ARG and L.srt_bind_probe_states_output(pt._h, 0, None) == c.ERR_INVALID_ARG
        w = c.ProbeClassifyWork()
        assert L.srt_get_probe_classify_work(pt._h, C.byref(w)) == c.ERR_STATE
        assert call() == c.OK  # without relocation no directions are needed
        want = PS.classify(PS.room_grid(), objs)
        assert L.srt_read_probe_states_output(pt._h, 1, buf.ctypes.data_as(C.c_void_p)) == c.OK and same(buf, want["records"])
        assert L.srt_read_probe_states_output(pt._h, 2, buf.ctypes.data_as(C.c_void_p)) == c.ERR_STATE
        assert call(clearance=nan) == c.ERR_INVALID_ARG
        assert L.srt_read_probe_states_output(pt._h, 1, buf.ctypes.data_as(C.c_void_p)) == c.OK and same(buf, want["records"])
        assert L.srt_classify_probes(pt._h, None) == c.ERR_INVALID_ARG
        pt.wait()
    finally:
        pt.close()
