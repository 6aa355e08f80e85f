"""The probe tail (srt_probe_tail, ABI 7) on the MI355X: radiance and light-probe paths that end at the bounce limit on a surface
add the probe grid's hemisphere-mean radiance there.  Every comparison is bit for bit in all four lanes with no ray left out.

The reference is tests/probe_tail_reference.py: its path loop is pinned against the CPU oracle by tests/test_probe_tail_reference.py,
and its lookup is the shading references' (pinned against the three shading calls).  The paths of a (scene, bounces) pair are
traced once on the CPU and shared by the five flag sets.  24 x 20 camera rays make seven full blocks of 64 and one of 32 lanes.

Shared inputs: a 5 x 4 x 5 grid that covers part of the scenes only (terminal points outside it are clamped), seeded random
finite coefficients of both signs, R = 4 moments, and records with buried probes (two whole planes: every cell between them is
dark), other buried probes and offsets."""
import ctypes as C

import numpy as np
import pytest

import light_probe_reference as LP
import probe_grid_reference as PG
import probe_tail_reference as PT
from test_gpu_radiance import Scene, camera_rays, differing, reflection_scene, same, srt_camera
from test_gpu_visibility import closed_room, memory_scene, mesh_scene, scene1

pytestmark = pytest.mark.gpu

F = np.float32
W, H, N, SAMPLES = 24, 20, 480, 3
GRID = PG.Grid((-2.0, -1.0, 1.0), (1.0, 0.8, 1.2), (5, 4, 5))
FLAT = PG.Grid((-2.0, 0.1, 1.0), (1.0, 0.8, 1.2), (5, 1, 5))  # n_y == 1
R = 4
BURIED = 2
FLAG_SETS = {"none": 0, "normal_weight": PT.NORMAL_WEIGHT, "depth": PT.DEPTH, "states": PT.STATES,
             "all": PT.DEPTH | PT.STATES | PT.NORMAL_WEIGHT}
COUNTS = ("tails", "corners", "open", "dark", "mirror_ends")


def grid_inputs(grid, seed=1234):
    """(coefficients (P, 9, 4), moments (P, R*R, 4), records (P, 4)) of a grid: finite, both signs, some probes buried or moved."""
    rng = np.random.RandomState(seed)
    P = grid.probes
    co = rng.uniform(-0.6, 1.4, (P, 9, 4)).astype(F)
    co[:, 0, :3] += F(1.0)  # (a mostly positive mean, with negative lobes)
    m1 = rng.uniform(0.4, 3.0, (P, R * R)).astype(F)
    mo = np.zeros((P, R * R, 4), F)
    mo[..., 0], mo[..., 1] = m1, (m1 * m1 + rng.uniform(0.0, 0.3, (P, R * R)).astype(F)).astype(F)
    rec = np.zeros((P, 4), F)
    moved = rng.rand(P) < 0.3
    rec[moved, :3] = rng.uniform(-0.2, 0.2, (int(moved.sum()), 3)).astype(F)
    bits = np.zeros(P, np.uint32)
    bits[moved] |= 1
    ix = np.arange(P) % grid.counts[0]
    bits[(ix <= 1) | (rng.rand(P) < 0.1)] |= BURIED  # the planes ix = 0 and 1: the eight corners of every cell between them
    rec[:, 3] = bits.view(F)
    return co, mo, rec


CO, MO, REC = grid_inputs(GRID)


def fp(a):
    return np.ascontiguousarray(a, F).ctypes.data_as(C.POINTER(C.c_float))


def set_grid(pt, grid, co, mo=None, rec=None):
    pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
    pt._ck(pt.L.srt_write_probe_grid_coefficients(pt._h, fp(co), grid.probes))
    if mo is not None:
        pt._ck(pt.L.srt_write_probe_grid_depth(pt._h, fp(mo), grid.probes, R))
    if rec is not None:
        pt._ck(pt.L.srt_write_probe_grid_states(pt._h, fp(rec), grid.probes))


def tail(pt, flags, on=True, count=True):
    pt.probe_tail(enabled=on, normal_weight=bool(flags & PT.NORMAL_WEIGHT), depth=bool(flags & PT.DEPTH), states=bool(flags & PT.STATES),
                  count_work=count)


def expected(colours, terminals, grid, co, flags, first_sample=1):
    """(the radiance the mode gives, the work record's five counts) from the shared paths."""
    add, adds, work = PT.tails(terminals, grid, co, flags=flags, depth=MO, R=R, records=REC)
    return PT.radiance(colours, first_sample=first_sample, add=(add, adds)), work


SCENES = {"scene1": scene1, "room": closed_room, "reflection": reflection_scene, "mesh": mesh_scene, "memory": memory_scene}
# the seed of each (scene, bounces) case: the reflection scene's are the first at which a path ends with 0 < g < 1 and one with
# !(g > 0) (found with the reference loop on a CPU)
# the mesh scene's at B = 8 is the first at which one of its few tails meets a buried cell (dark >= 1 under STATES)
SEEDS = {("reflection", 1): 1, ("reflection", 2): 2, ("reflection", 8): 141, ("mesh", 8): 2}
_paths = {}


def room_camera(oracle):
    """Inside the closed room, turned about two axes (sines 0.6 and 0.28): no ray direction has a component of exactly zero, which
    the reference's box test (a slab test) answers with a miss, so every primary ray of the frame meets a wall."""
    cam = oracle.default_camera()
    cam.position[:] = (0.1, 0.05, 0.3)
    cam.right[:] = (0.8, 0.0, -0.6)
    cam.up[:] = (0.168, 0.96, 0.224)
    cam.forward[:] = (0.576, -0.28, 0.768)
    return cam


@pytest.fixture(scope="module")
def scenes(srt, oracle):
    made = {}

    def get(name):
        if name not in made:
            s = Scene(srt, oracle, SCENES[name](oracle))
            s.ref = PT.Scene(oracle, s.oarr, s.n, om=s.om[:2] if s.om else None, env=s.env)
            s.rays = camera_rays(oracle, room_camera(oracle) if name == "room" else oracle.default_camera())
            made[name] = s
        return made[name]

    yield get
    for s in made.values():
        s.close()


def paths(s, name, bounces, seed, samples=SAMPLES):
    key = (name, bounces, seed, samples)
    if key not in _paths:
        _paths[key] = PT.trace(s.ref, s.rays[0], s.rays[1], samples, bounces, seed=seed)
    return _paths[key]


# ---- 1. bit for bit against the reference loop ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounces", [1, 2, 8])
@pytest.mark.parametrize("name", list(SCENES))
def test_every_flag_set_gives_the_reference_loops_bits_and_counts(scenes, name, bounces):
    s = scenes(name)
    seed = SEEDS.get((name, bounces), 3 + bounces)
    colours, terminals = paths(s, name, bounces, seed)
    ended = [t for t in terminals if t is not None]
    # the preconditions, from the reference
    assert ended
    if name == "room":  # every sample ends in a lookup or a mirror end
        assert len(ended) == len(terminals)
    if name == "scene1":  # both tails and sky ends
        assert 0 < len(ended) < len(terminals)
    if name == "reflection":
        assert any(0 < float(t["g"]) < 1 for t in ended) and any(not t["g"] > 0 for t in ended)
    x = np.array([t["x"] for t in ended], F)
    lo, hi = GRID.origin, GRID.origin + GRID.spacing * (np.array(GRID.counts, F) - 1)
    outside = ((x < lo) | (x > hi)).any(axis=1)
    if name in ("scene1", "room", "memory"):
        assert outside.any() and (~outside).any()  # clamped lookups and interior ones
    set_grid(s.pt, GRID, CO, MO, REC)
    o, d = s.rays
    try:
        for label, flags in FLAG_SETS.items():
            want, work = expected(colours, terminals, GRID, CO, flags)
            if flags & PT.STATES:
                assert work["dark"] >= 1
            tail(s.pt, flags)
            s.pt.trace_radiance(o, d, samples=SAMPLES, bounces=bounces, seed=seed, count_work=True)
            got, tw, rw = s.pt.radiance(), s.pt.probe_tail_work(), s.pt.radiance_work()
            print("%s B=%d %s: %d rays differ; reference %s; device %s" % (name, bounces, label, differing(got, want), work, tw))
            assert same(got, want), "%s: %d of %d rays differ from the reference" % (label, differing(got, want), N)
            assert tw["valid"] == 1 and {k: tw[k] for k in COUNTS} == work
            assert 1 <= tw["wave_lookups"] <= tw["tails"] + tw["mirror_ends"]
            if not flags & PT.DEPTH:
                assert tw["open"] == tw["corners"]
            # a lookup traces no ray: the radiance record is the mode-off record
            tail(s.pt, flags, on=False)
            s.pt.trace_radiance(samples=SAMPLES, bounces=bounces, seed=seed, count_work=True)
            assert s.pt.radiance_work() == rw
    finally:
        tail(s.pt, 0, on=False)


def test_a_grid_with_one_probe_along_an_axis(scenes):
    s = scenes("scene1")
    colours, terminals = paths(s, "scene1", 2, 5)
    co = grid_inputs(FLAT, 77)[0]
    add, adds, work = PT.tails(terminals, FLAT, co, flags=PT.NORMAL_WEIGHT)
    want = PT.radiance(colours, add=(add, adds))
    set_grid(s.pt, FLAT, co)
    try:
        tail(s.pt, PT.NORMAL_WEIGHT)
        s.pt.trace_radiance(*s.rays, samples=SAMPLES, bounces=2, seed=5)
        got, tw = s.pt.radiance(), s.pt.probe_tail_work()
        assert same(got, want), "%d of %d rays differ" % (differing(got, want), N)
        assert {k: tw[k] for k in COUNTS} == work and work["tails"] > 0
    finally:
        tail(s.pt, 0, on=False)


# ---- 2. chunk crossing ------------------------------------------------------------------------------------------------------------
def test_seventy_samples_cross_the_chunk_and_one_ray_fills_the_wave(scenes, srt, oracle):
    s = scenes("scene1")
    o, d = s.rays
    pick = np.arange(200, 208)  # eight rays of the middle rows
    sub = PT.trace(s.ref, o[pick], d[pick], 70, 2, seed=9, id_base=0)
    assert any(sub[1][r * 70 + k] is not None for r in range(8) for k in range(64, 70))  # (tails in the slots past RAD_CHUNK)
    add, adds, work = PT.tails(sub[1], GRID, CO, flags=PT.DEPTH, depth=MO, R=R)
    want = PT.radiance(sub[0], add=(add, adds))
    set_grid(s.pt, GRID, CO, MO, REC)
    try:
        tail(s.pt, PT.DEPTH)
        s.pt.trace_radiance(o[pick], d[pick], samples=70, bounces=2, seed=9)
        assert same(s.pt.radiance(), want)
        assert {k: s.pt.probe_tail_work()[k] for k in COUNTS} == work
    finally:
        tail(s.pt, 0, on=False)
    # one ray of 64 samples in the closed room: every path ends at the limit, all 64 in the same step at B = 1
    r = Scene(srt, oracle, closed_room(oracle), 8, 8)
    try:
        ro, rd = camera_rays(oracle, oracle.default_camera(), 8, 8)
        i = 4 + 4 * 8
        ref = PT.Scene(oracle, r.oarr, r.n, env=r.env)
        colours, terminals = PT.trace(ref, ro[i:i + 1], rd[i:i + 1], 64, 1, seed=0, id_base=36)
        assert all(t is not None for t in terminals)
        add, adds, work = PT.tails(terminals, GRID, CO)
        set_grid(r.pt, GRID, CO)
        tail(r.pt, 0)
        r.pt.trace_radiance(ro[i:i + 1], rd[i:i + 1], samples=64, bounces=1, seed=0, id_base=36, count_work=True)
        assert same(r.pt.radiance(), PT.radiance(colours, add=(add, adds)))
        tw = r.pt.probe_tail_work()
        assert {k: tw[k] for k in COUNTS} == work and tw["tails"] + tw["mirror_ends"] == 64 and tw["wave_lookups"] == 1
        assert r.pt.radiance_work()["wave_calls"] <= 3
    finally:
        r.close()


# ---- 3. zero coefficients ---------------------------------------------------------------------------------------------------------
def test_zero_coefficients_give_the_bits_and_the_radiance_work_of_the_mode_off(scenes):
    s = scenes("scene1")
    o, d = s.rays
    s.pt.trace_radiance(o, d, samples=70, bounces=8, seed=2, count_work=True)
    off, off_work = s.pt.radiance(), s.pt.radiance_work()
    set_grid(s.pt, GRID, np.zeros_like(CO), MO, REC)
    try:
        tail(s.pt, PT.DEPTH | PT.STATES | PT.NORMAL_WEIGHT)
        s.pt.trace_radiance(samples=70, bounces=8, seed=2, count_work=True)
        assert same(s.pt.radiance(), off) and s.pt.radiance_work() == off_work
        assert s.pt.probe_tail_work()["tails"] > 0
    finally:
        tail(s.pt, 0, on=False)


# ---- 4. continuation and splitting ------------------------------------------------------------------------------------------------
def test_continuation_and_splitting_with_the_mode_on(scenes):
    s = scenes("room")
    o, d = s.rays
    set_grid(s.pt, GRID, CO, MO, REC)
    try:
        tail(s.pt, PT.STATES)
        s.pt.trace_radiance(o, d, samples=9, bounces=2, seed=5)
        whole = s.pt.radiance()
        s.pt.trace_radiance(samples=3, bounces=2, seed=5, first_sample=1, reset=True)
        first = s.pt.radiance()
        s.pt.trace_radiance(samples=6, bounces=2, seed=5, first_sample=4, reset=False)
        assert same(s.pt.radiance(), whole) and not same(first, whole)
        parts = []
        for a, b in ((0, 200), (200, N)):
            s.pt.trace_radiance(o[a:b], d[a:b], samples=9, bounces=2, seed=5, id_base=a)
            parts.append(s.pt.radiance())
        assert same(np.concatenate(parts), whole)
        tail(s.pt, 0, on=False)
        s.pt.trace_radiance(o, d, samples=9, bounces=2, seed=5)
        assert not same(s.pt.radiance(), whole)  # (the tail adds light in the room)
    finally:
        tail(s.pt, 0, on=False)


# ---- 5. light probes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 96])
def test_light_probes_under_the_mode(scenes, srt, K):
    import torch

    s = scenes("room")
    pt = s.pt
    pos = np.zeros((6, 4), F)
    pos[:, :3] = [(-1.5, 0.2, 2.0), (0.0, 0.5, 3.0), (1.2, -0.4, 4.0), (0.4, 1.0, 2.5), (-0.6, -0.5, 4.5), (1.8, 0.3, 1.5)]
    dirs = LP.sphere(K).reshape(K, 4).astype(F)
    set_grid(pt, GRID, CO, MO, REC)
    dev = "cuda:%d" % pt.device
    try:
        tail(pt, PT.DEPTH | PT.STATES)
        pt.trace_light_probes(pos, dirs, samples=SAMPLES, bounces=1, seed=4, radiance=True, count_work=True)
        rad, co, tw = pt.light_probe_radiance(), pt.light_probe_coefficients(), pt.probe_tail_work()
        # RADIANCE: srt_trace_radiance on the explicit rays under the same mode
        o = np.repeat(pos, K, axis=0)
        d = np.tile(dirs, (6, 1))
        pt.trace_radiance(o, d, samples=SAMPLES, bounces=1, seed=4)
        explicit = pt.radiance()
        assert same(rad.reshape(-1, 4), explicit), "%d of %d rays differ from srt_trace_radiance" % (differing(rad.reshape(-1, 4), explicit), 6 * K)
        assert {k: pt.probe_tail_work()[k] for k in COUNTS} == {k: tw[k] for k in COUNTS} and tw["tails"] > 0
        assert same(co, LP.project(rad, dirs))
        tail(pt, 0, on=False)
        pt.trace_radiance(samples=SAMPLES, bounces=1, seed=4)
        assert not same(pt.radiance(), explicit)
        # the listed call: probes 1, 3 and 4 as the unlisted call writes them, the others' sentinel
        tail(pt, PT.DEPTH | PT.STATES)
        t_co = torch.full((6 * 9, 4), -7.0, dtype=torch.float32, device=dev)
        t_rad = torch.full((6 * K, 4), -7.0, dtype=torch.float32, device=dev)
        pt.bind_light_probe_output("coefficients", t_co)
        pt.bind_light_probe_output("radiance", t_rad)
        pt.bind_probe_list(np.array([3, 6, 0, 0, 1, 3, 4, 0, 0, 0], np.uint32))
        pt.trace_light_probes(samples=SAMPLES, bounces=1, seed=4, radiance=True, listed=True)
        pt.wait()
        lco, lrad = t_co.cpu().numpy().reshape(6, 9, 4), t_rad.cpu().numpy().reshape(6, K, 4)
        for p in range(6):
            if p in (1, 3, 4):
                assert same(lco[p], co[p]) and same(lrad[p], rad[p]), p
            else:
                assert (lco[p] == -7.0).all() and (lrad[p] == -7.0).all(), p
        # the feedback loop on one buffer: the tail's coefficient source as the call's COEFFICIENTS output
        before = t_co.clone()
        tail(pt, 0)
        pt._ck(pt.L.srt_bind_probe_grid_coefficients(pt._h, C.c_void_p(t_co.data_ptr()), 6))
        pt.set_probe_grid((0.0, 0.0, 1.0), (1.0, 1.0, 1.0), (3, 2, 1))
        capi = srt.capi
        p = capi.LightProbeParams()
        pt.L.srt_light_probe_params_default(C.byref(p))
        p.sample_count, p.max_bounces, p.outputs = SAMPLES, 1, capi.LIGHT_PROBE_COEFFICIENTS
        assert pt.L.srt_trace_light_probes(pt._h, C.byref(p)) == capi.ERR_STATE
        assert pt.L.srt_trace_light_probes_listed(pt._h, C.byref(p)) == capi.ERR_STATE
        p.max_bounces = 0  # T1: unchanged, and unchecked
        assert pt.L.srt_trace_light_probes_listed(pt._h, C.byref(p)) == capi.OK
        pt.wait()
        p.max_bounces = 1
        snap = t_co.clone()
        assert pt.L.srt_trace_light_probes(pt._h, C.byref(p)) == capi.ERR_STATE
        pt.wait()
        assert torch.equal(t_co, snap) and not torch.equal(snap, before)  # the refused call writes nothing (the B = 0 call did write)
    finally:
        tail(pt, 0, on=False)
        pt._ck(pt.L.srt_bind_probe_grid_coefficients(pt._h, None, 0))
        pt.bind_light_probe_output("coefficients", None)
        pt.bind_light_probe_output("radiance", None)
        pt.bind_probe_list(None)


# ---- 6. errors and mode -----------------------------------------------------------------------------------------------------------
def test_state_errors_mode_off_repeatability_and_the_passes_that_ignore_the_mode(srt, oracle):
    import torch

    c = srt.capi
    s = Scene(srt, oracle, scene1(oracle))
    pt = s.pt
    try:
        o, d = camera_rays(oracle, oracle.default_camera())
        pt.write_rays(o, d)

        def rc(bounces=2):
            p = c.RadianceParams()
            pt.L.srt_radiance_params_default(C.byref(p))
            p.sample_count, p.max_bounces = SAMPLES, bounces
            return pt.L.srt_trace_radiance(pt._h, C.byref(p))

        # the two light-probe calls meet every refusal that srt_trace_radiance meets: four probes, 64 directions, two of them listed
        pos = np.zeros((4, 4), F)
        pos[:, :3] = [(-1.0, 0.5, 3.0), (0.0, 0.5, 3.0), (1.0, 0.5, 3.0), (0.0, 1.0, 2.0)]
        pt.trace_light_probes(pos, 64, samples=1, bounces=1)
        pt.bind_probe_list(np.array([2, 4, 0, 0, 0, 2, 0, 0], np.uint32))

        def lp(listed, bounces=1):
            p = c.LightProbeParams()
            pt.L.srt_light_probe_params_default(C.byref(p))
            p.sample_count, p.max_bounces = 1, bounces
            return (pt.L.srt_trace_light_probes_listed if listed else pt.L.srt_trace_light_probes)(pt._h, C.byref(p))

        def refused():
            return (rc(), lp(False), lp(True)) == (c.ERR_STATE,) * 3

        w = c.ProbeTailWork()
        assert lp(False) == c.OK and lp(True) == c.OK
        assert rc() == c.OK and pt.L.srt_get_probe_tail_work(pt._h, C.byref(w)) == c.ERR_STATE  # the mode is off
        off = pt.radiance(N)
        tail(pt, PT.DEPTH | PT.STATES)
        assert refused()  # no grid
        assert lp(False, 0) == c.OK and lp(True, 0) == c.OK
        assert rc(0) == c.OK        # T1: max_bounces == 0 is unchanged and asks for nothing
        assert pt.L.srt_get_probe_tail_work(pt._h, C.byref(w)) == c.OK and (w.valid, w.tails, w.wave_lookups) == (1, 0, 0)
        pt.set_probe_grid(GRID.origin, GRID.spacing, GRID.counts)
        assert refused()  # no coefficients
        pt._ck(pt.L.srt_write_probe_grid_coefficients(pt._h, fp(CO), GRID.probes - 1))
        assert refused()  # a count that is not nx*ny*nz
        pt._ck(pt.L.srt_write_probe_grid_coefficients(pt._h, fp(CO), GRID.probes))
        assert refused()  # DEPTH without maps
        pt._ck(pt.L.srt_write_probe_grid_depth(pt._h, fp(MO), GRID.probes - 1, R))
        assert refused()
        pt._ck(pt.L.srt_write_probe_grid_depth(pt._h, fp(MO), GRID.probes, R))
        assert refused()  # STATES without records
        pt._ck(pt.L.srt_write_probe_grid_states(pt._h, fp(REC), GRID.probes - 1))
        assert refused()
        pt._ck(pt.L.srt_write_probe_grid_states(pt._h, fp(REC), GRID.probes))
        assert (rc(), lp(False), lp(True)) == (c.OK,) * 3  # everything the flags ask for is there
        # the coefficient array as the RADIANCE output: refused, and nothing is written
        t = torch.full((GRID.probes * 9, 4), 0.25, dtype=torch.float32, device="cuda:%d" % pt.device)
        pt._ck(pt.L.srt_bind_probe_grid_coefficients(pt._h, C.c_void_p(t.data_ptr()), GRID.probes))
        pt.bind_radiance(t)
        assert rc() == c.ERR_STATE
        pt.wait()
        assert bool((t == 0.25).all())
        pt.bind_radiance(None)
        pt._ck(pt.L.srt_bind_probe_grid_coefficients(pt._h, None, 0))
        bad = c.ProbeTailParams()
        pt.L.srt_probe_tail_params_default(C.byref(bad))
        bad.flags = 16
        assert pt.L.srt_probe_tail(pt._h, C.byref(bad)) == c.ERR_INVALID_ARG  # ... and the previous setting stands:
        # two identical runs: identical bits and wave_lookups
        runs = []
        for _ in range(2):
            assert rc() == c.OK
            runs.append((pt.radiance(N), pt.probe_tail_work()))
        assert same(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and runs[0][1]["tails"] > 0
        assert not same(runs[0][0], off)
        # srt_render and srt_render_adaptive ignore the mode
        pt.set_camera(srt_camera(srt, oracle.default_camera()))

        def frames():
            pt.render(spp=2, bounces=2, seed=1)
            a = pt.accumulator()
            pt.set_sample_counts(2)
            pt.write_sample_budget(np.full((H, W), 3, np.uint32))
            pt.render_adaptive(bounces=2, seed=1)
            return a, pt.accumulator()

        on = frames()
        tail(pt, 0, on=False)
        plain = frames()
        assert same(on[0], plain[0]) and same(on[1], plain[1])
        # the mode off after on restores the bits
        assert rc() == c.OK and same(pt.radiance(N), off)
        assert pt.L.srt_get_probe_tail_work(pt._h, C.byref(w)) == c.ERR_STATE
    finally:
        s.close()


# ---- 7. quality -------------------------------------------------------------------------------------------------------------------
MEASURED_RATIO = {"B1_tail": 1.51, "B1_tail_depth_states": 1.65}  # rmse(without) / rmse(with), one measured run (see the docstring)


def test_the_tail_lowers_the_error_of_one_bounce_in_scene_indirect(srt):
    """tools/probe_tail_quality.py's protocol at 96 x 54 in Scene_indirect, grid spacing 0.5, coefficients from probes traced at
    B = 8: the relative luminance RMSE over the diffuse pixels of camera-ray radiance at B = 1, n = 64, against a 4096-sample
    B = 8 srt_render, without the tail and with it.  The measured ratios rmse(without) / rmse(with) are in MEASURED_RATIO and in
    profiles/probe_tail/probe_tail_quality.jsonl; the test asserts half of each (noise and the SH approximation get a factor of
    two), and nothing for a ratio that was measured below 1.5.  One run: 42 diffuse pixels, rmse 0.0795 without, 0.0528 with the
    tail (ratio 1.51), 0.0483 with DEPTH | STATES (ratio 1.65)."""
    import os
    import sys

    from conftest import ROOT

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import probe_tail_quality as Q

    pt, rmse, info = Q.frame_setup(srt, "Scene_indirect", 96, 54, 4096, 0.5)
    try:
        without = rmse(64, 1, None)
        for key, tail_flags in (("B1_tail", {}), ("B1_tail_depth_states", {"depth": True, "states": True})):
            with_tail = rmse(64, 1, tail_flags)
            ratio = without / with_tail
            print("Scene_indirect 96x54 B=1 n=64 %s: rmse without %.4f, with %.4f, ratio %.2f (%s)" % (key, without, with_tail, ratio, info))
            measured = MEASURED_RATIO[key]
            if measured is not None and measured >= 1.5:
                assert ratio >= measured / 2
    finally:
        pt.bind_rays(None, None)
        pt.close()


# ---- 8. the command line ----------------------------------------------------------------------------------------------------------
def test_the_cli_gives_the_bytes_of_the_python_route(scenes, srt, tmp_path):
    """srt_render --rays --radiance N --probe-tail, and the feedback rounds of --probe-grid --probe-feedback F: the tail reading the
    coefficient history, then srt_blend_probes, and the frame shaded from the history."""
    import os
    import subprocess

    from conftest import ROOT, scene_path

    cli = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
    # the ray file: Scene1's camera rays under the tail with the normal weight
    s = scenes("scene1")
    o, d = s.rays
    (tmp_path / "in.f32").write_bytes(np.concatenate([o, d], axis=1).astype(F).tobytes())
    (tmp_path / "co.f32").write_bytes(CO.tobytes())
    set_grid(s.pt, GRID, CO)
    try:
        tail(s.pt, PT.NORMAL_WEIGHT, count=False)
        s.pt.trace_radiance(o, d, samples=3, bounces=2, seed=7)
        want = s.pt.radiance()
        tail(s.pt, 0, on=False)
        s.pt.trace_radiance(samples=3, bounces=2, seed=7)
        assert not same(s.pt.radiance(), want)
    finally:
        tail(s.pt, 0, on=False)
    out = tmp_path / "out.bin"
    base = [cli, "--scene", scene_path("Scene1"), "--rays", str(tmp_path / "in.f32"), "--rays-out", str(out), "--radiance", "3", "--bounces", "2", "--seed", "7"]
    run = subprocess.run(base + ["--probe-tail", "--probe-tail-normal-weight", "--probe-tail-grid", "-2,-1,1,1,0.8,1.2,5,4,5", "--probe-tail-coefficients",
                                 str(tmp_path / "co.f32")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    assert out.read_bytes() == want.tobytes()
    for bad in (["--probe-tail"], ["--probe-tail", "--probe-tail-grid", "-2,-1,1,1,0.8,1.2,5,4,5", "--probe-tail-coefficients", str(tmp_path / "co.f32"), "--probe-tail-depth"],
                ["--probe-tail", "--probe-tail-grid", "-2,-1,1,1,0.8,1.2,5,4,4", "--probe-tail-coefficients", str(tmp_path / "co.f32")]):
        assert subprocess.run(base + bad, capture_output=True, text=True, timeout=120).returncode == 2, bad
    # the feedback rounds in Scene_indirect: three rounds at one bounce
    w, h, K, rounds = 32, 24, 64, 3
    grid = PG.Grid((-2.5, -1.0, 0.5), (1.25, 0.8, 1.5), (5, 4, 5))
    pt = srt.PathTracer(w, h)
    try:
        objs, cnt = srt.host.Scene(scene_path("Scene_indirect")).objects_copy()
        pt.set_scene(objs, cnt)
        pt.set_camera(srt.default_camera())
        pos = srt.probe_grid_positions(grid.origin, grid.spacing, grid.counts)
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        pt.reset_probe_history(grid.probes, which="coefficients")
        lookups = 0
        for f in range(1, rounds + 1):
            if f > 1:
                pt._ck(pt.L.srt_write_probe_grid_coefficients(pt._h, fp(pt.probe_history("coefficients")), grid.probes))
            pt.probe_tail(enabled=f > 1, count_work=True)
            pt.trace_light_probes(pos, K, samples=16, bounces=1, seed=f)
            pt.blend_probes()
            if f > 1:
                lookups += pt.probe_tail_work()["tails"]
        pt.probe_tail(enabled=False)
        assert lookups > 0
        history = pt.probe_history("coefficients")
        pt.render_gbuffer()
        pt.shade_probe_grid(coefficients=history)
        image = pt.probe_grid_output()
        pt.trace_light_probes(pos, K, samples=16, bounces=1, seed=1)  # (one round, no feedback: other light)
        pt.shade_probe_grid(coefficients=pt.light_probe_coefficients())
        assert not same(pt.probe_grid_output(), image)
    finally:
        pt.close()
    img = tmp_path / "irradiance.f32"
    run = subprocess.run([cli, "--scene", scene_path("Scene_indirect"), "--width", str(w), "--height", str(h), "--probe-grid", "-2.5,-1,0.5,1.25,0.8,1.5,5,4,5",
                          "--probe-directions", str(K), "--probe-feedback", str(rounds), "--probe-bounces", "1", "--irradiance-out", str(img)],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "probe feedback round 3" in run.stderr
    assert img.read_bytes() == image.tobytes()
