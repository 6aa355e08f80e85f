"""The listed probe traces (srt_trace_light_probes_listed, srt_trace_probe_depth_listed, ABI 7) on the MI355X, bit for bit against
the unlisted calls (rule L): every probe listed, the synthetic room's real list over sentinel-filled outputs, an empty list, a
shuffled list, a list with indices out of range, a continuation over two listed calls, more listed probes than resident waves, and
the per-frame route classify -> list -> listed trace -> blend -> shade with every buffer bound device to device."""
import numpy as np
import pytest

import probe_grid_reference as PG
import probe_states_reference as PS
import probe_update_reference as PU
from test_gpu_probe_states import tracer
from test_gpu_visibility import Frame, mesh_scene, scene1

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
SENTINEL = -7.0
R = 8
N_SAMPLES, BOUNCES = 3, 3
LP_KEYS = ("probes", "rays", "samples", "closest_calls", "wave_calls", "waves")
PD_KEYS = ("probes", "rays", "far_rays", "wave_calls", "waves")


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(U), b.view(U))


class Outputs:
    """The four outputs bound to sentinel-filled tensors with a border."""

    def __init__(self, pt, P, K):
        import torch

        self.pt, self.P, self.K = pt, P, K
        dev = "cuda:%d" % pt.device
        self.t = dict(coefficients=torch.empty((P * 9 + 5, 4), dtype=torch.float32, device=dev), radiance=torch.empty((P * K + 5, 4), dtype=torch.float32, device=dev),
                      moments=torch.empty((P * R * R + 5, 4), dtype=torch.float32, device=dev), distances=torch.empty((P * K + 5,), dtype=torch.float32, device=dev))
        self.shape = dict(coefficients=(P, 9, 4), radiance=(P, K, 4), moments=(P, R * R, 4), distances=(P, K))
        for k in ("coefficients", "radiance"):
            pt.bind_light_probe_output(k, self.t[k])
        for k in ("moments", "distances"):
            pt.bind_probe_depth_output(k, self.t[k])

    def fill(self):
        import torch

        for t in self.t.values():
            t.fill_(SENTINEL)
        torch.cuda.synchronize()

    def read(self):
        """The four arrays; the borders must hold the sentinel."""
        self.pt.wait()
        out = {}
        for k, t in self.t.items():
            a = t.cpu().numpy()
            n = int(np.prod(self.shape[k][:2]))
            assert np.all(a[n:] == SENTINEL), k
            out[k] = a[:n].reshape(self.shape[k])
        return out

    def close(self):
        self.pt.wait()
        for k in ("coefficients", "radiance"):
            self.pt.bind_light_probe_output(k, None)
        for k in ("moments", "distances"):
            self.pt.bind_probe_depth_output(k, None)
        self.pt.bind_probe_list(None)


def trace(pt, listed, seed=5, samples=N_SAMPLES, first_sample=1, reset=True):
    pt.trace_light_probes(samples=samples, bounces=BOUNCES, seed=seed, first_sample=first_sample, reset=reset, id_base=1000, radiance=True, count_work=True, listed=listed)
    pt.trace_probe_depth(resolution=R, sharpness=3, max_distance=4.0, distances=True, count_work=True, listed=listed)


def expect_slots(got, full, idx, P):
    """Listed slots hold the unlisted call's bits, every other slot the sentinel."""
    skipped = np.setdiff1d(np.arange(P), idx)
    for k in got:
        assert same(got[k][idx], full[k][idx]), k
        assert np.all(got[k][skipped] == SENTINEL), k


def run_cases(srt, pt, positions, K, words, thorough):
    P = positions.shape[0]
    d = srt.light_probe_sphere(K)
    pt.trace_light_probes(positions, d, samples=1, bounces=0)  # (makes the positions and directions current)
    o = Outputs(pt, P, K)
    try:
        o.fill()
        trace(pt, False)
        full, lw, dw = o.read(), pt.light_probe_work(), pt.probe_depth_work()
        assert not any(np.any(v == SENTINEL) for v in full.values())
        # (a) every probe listed: all outputs and the work counts of the unlisted call
        pt.bind_probe_list(PU.probe_list(PU.records_of(np.zeros(P, U))))
        o.fill()
        trace(pt, True)
        got = o.read()
        for k in got:
            assert same(got[k], full[k]), k
        assert {k: pt.light_probe_work()[k] for k in LP_KEYS} == {k: lw[k] for k in LP_KEYS}
        assert {k: pt.probe_depth_work()[k] for k in PD_KEYS} == {k: dw[k] for k in PD_KEYS}
        # (b) the real list: listed slots equal, skipped slots keep the sentinel; `probes` counts n
        idx = PU.listed(words)
        assert 5 <= idx.shape[0] <= P - 5
        pt.bind_probe_list(words)
        o.fill()
        trace(pt, True)
        expect_slots(o.read(), full, idx, P)
        assert pt.light_probe_work()["probes"] == idx.shape[0] == pt.probe_depth_work()["probes"]
        assert pt.light_probe_work()["rays"] == idx.shape[0] * K == pt.probe_depth_work()["rays"]
        if not thorough:
            return
        # (c) an empty list: nothing is written
        empty = words.copy()
        empty[0] = 0
        pt.bind_probe_list(empty)
        o.fill()
        trace(pt, True)
        expect_slots(o.read(), full, idx[:0], P)
        assert pt.light_probe_work()["probes"] == 0 == pt.probe_depth_work()["rays"]
        # (d) a list shuffled on the host: the same bits per slot
        shuffled = words.copy()
        shuffled[4:4 + idx.shape[0]] = np.random.default_rng(K).permutation(idx).astype(U)
        assert not np.array_equal(shuffled, words)
        pt.bind_probe_list(shuffled)
        o.fill()
        trace(pt, True)
        expect_slots(o.read(), full, idx, P)
        # (e) indices >= P are skipped, a count beyond P is clamped: nothing out of range, the other slots right
        bad = words.copy()
        bad[4 + 1], bad[4 + 3] = P, 0xFFFFFFF0
        bad[0] = P + 1000
        good = PU.listed(bad, P)
        assert good.shape[0] == idx.shape[0] - 2
        pt.bind_probe_list(bad)
        o.fill()
        trace(pt, True)
        expect_slots(o.read(), full, good, P)
        # (f) a continuation over two listed calls equals one call of the summed sample count
        pt.bind_probe_list(words)
        o.fill()
        trace(pt, True, samples=2)
        trace(pt, True, samples=N_SAMPLES - 2, first_sample=3, reset=False)
        expect_slots(o.read(), full, idx, P)
    finally:
        o.close()


@pytest.fixture(scope="module")
def room(srt, oracle):
    objs = PS.synthetic_room()
    pt = tracer(srt, oracle, (objs, None))
    yield pt, objs
    pt.close()


@pytest.mark.parametrize("K", [1, 64, 65, 130])
def test_the_room_listed_against_unlisted(srt, room, K):
    pt, objs = room
    grid = PS.room_grid(0.9, (4, 3, 5))
    c = PS.classify(grid, objs, srt.light_probe_sphere(64), PS.RELOCATE)
    run_cases(srt, pt, c["positions"], K, PU.probe_list(c["records"]), thorough=True)


@pytest.mark.parametrize("K", [1, 64, 65, 130])
def test_scene1_and_the_mesh_scene_listed_against_unlisted(srt, oracle, K):
    """Every case of the room's test again under the sky and in the mesh scene (the MESH instantiations of the listed kernels)."""
    for scene, grid in ((scene1(oracle), PG.Grid((-4.0, -1.5, 1.0), (1.0, 1.0, 1.0), (5, 4, 5))), (mesh_scene(oracle), PG.Grid((-2.0, -2.2, 3.0), (1.0, 1.0, 1.0), (5, 4, 5)))):
        pt = tracer(srt, oracle, scene)
        try:
            c = PS.classify(grid, scene[0])
            words = PU.probe_list(c["records"], PU.BURIED)
            run_cases(srt, pt, c["positions"], K, words, thorough=True)
        finally:
            pt.close()


def test_more_listed_probes_than_resident_waves(srt, room):
    """The 17 x 18 x 17 grid: 5202 probes, all listed: more than the 4096 waves of 1024 resident workgroups; then its real list."""
    pt, objs = room
    grid = PS.room_grid(0.24, (17, 18, 17))
    P = grid.probes
    c = PS.classify(grid, objs)
    d = srt.light_probe_sphere(64)
    kw = dict(samples=1, bounces=2, seed=3, count_work=True)
    pt.trace_light_probes(c["positions"], d, **kw)
    pt.trace_probe_depth(resolution=4, max_distance=4.0, count_work=True)
    full, dfull, lw, dw = pt.light_probe_coefficients(), pt.probe_depth_output("moments"), pt.light_probe_work(), pt.probe_depth_work()
    try:
        pt.bind_probe_list(PU.probe_list(c["records"], 0))
        pt.trace_light_probes(listed=True, **kw)
        pt.trace_probe_depth(resolution=4, max_distance=4.0, count_work=True, listed=True)
        assert same(pt.light_probe_coefficients(), full) and same(pt.probe_depth_output("moments"), dfull)
        assert pt.light_probe_work() == lw and pt.probe_depth_work() == dw and lw["probes"] == P > lw["waves"]
        words = PU.probe_list(c["records"])
        idx = PU.listed(words)
        pt.bind_probe_list(words)
        pt.trace_light_probes(listed=True, **dict(kw, seed=4))  # another seed: the slots not listed keep seed 3's bits
        pt.trace_probe_depth(resolution=4, max_distance=5.0, count_work=True, listed=True)
        got, gotd = pt.light_probe_coefficients(), pt.probe_depth_output("moments")
        skipped = np.setdiff1d(np.arange(P), idx)
        assert same(got[skipped], full[skipped]) and same(gotd[skipped], dfull[skipped]) and pt.light_probe_work()["probes"] == idx.shape[0]
        pt.trace_light_probes(**dict(kw, seed=4))
        pt.trace_probe_depth(resolution=4, max_distance=5.0)
        assert same(got[idx], pt.light_probe_coefficients()[idx]) and same(gotd[idx], pt.probe_depth_output("moments")[idx])
    finally:
        pt.wait()
        pt.bind_probe_list(None)


# ---- (h) the per-frame route, device to device --------------------------------------------------------------------------------------
def test_the_per_frame_route_device_to_device_equals_the_route_through_host_copies(srt, oracle):
    import torch

    fr = Frame(srt, oracle, scene1(oracle))  # (under the sky: the room is closed and dark)
    pt = fr.pt
    try:
        grid = PG.Grid((-4.0, -1.5, 1.0), (1.0, 1.0, 1.0), (5, 4, 5))
        P, K = grid.probes, 65
        d = srt.light_probe_sphere(K)
        dev = "cuda:%d" % pt.device
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)

        def frames():
            """Two frames of listed trace + blend: the histories hold the result."""
            for f in (1, 2):
                pt.trace_light_probes(samples=2, bounces=3, seed=f, listed=True)
                pt.trace_probe_depth(resolution=R, sharpness=3, max_distance=4.0, listed=True)
                pt.blend_probes(hysteresis=0.7, moments=True, listed=True)

        # the route through host copies
        pt.classify_probes(directions=d, relocate=True, positions=True)
        rec, pos = pt.probe_states_output("records"), pt.probe_states_output("positions")
        pt.bind_probe_grid_states(rec)
        pt.list_probes()
        words = pt.probe_list_output(P)
        assert same(words, PU.probe_list(rec)) and 5 <= words[0] <= P - 5
        pt.trace_light_probes(pos, d, samples=1, bounces=0)  # (the positions written from the host)
        pt.bind_probe_list(words)
        pt.reset_probe_history(P, R)
        frames()
        hist, dhist = pt.probe_history("coefficients"), pt.probe_history("moments")
        pt.shade_probe_grid_states(coefficients=hist, states=rec, moments=dhist, resolution=R, normal_weight=True)
        want = pt.probe_grid_output()
        idx = PU.listed(words)
        assert hist[idx, 0, 3].all() and not hist[np.setdiff1d(np.arange(P), idx)].any()
        # the same route with every buffer bound: no read-back in between
        t_rec = torch.zeros((P, 4), dtype=torch.float32, device=dev)
        t_pos = torch.zeros((P, 4), dtype=torch.float32, device=dev)
        t_list = torch.zeros((4 + P,), dtype=torch.int32, device=dev)
        t_hist = torch.full((P * 9, 4), SENTINEL, dtype=torch.float32, device=dev)
        t_dhist = torch.full((P * R * R, 4), SENTINEL, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        try:
            pt.bind_probe_states_output("records", t_rec)
            pt.bind_probe_states_output("positions", t_pos)
            pt.classify_probes(relocate=True, positions=True)
            pt.bind_probe_grid_states(t_rec)
            pt.list_probes(output=t_list)
            pt.bind_probe_list(t_list)
            pt.trace_light_probes(t_pos, None, samples=1, bounces=0)  # (binds the positions)
            pt.bind_probe_history("coefficients", t_hist)
            pt.bind_probe_history("moments", t_dhist)
            pt.reset_probe_history(P, R)
            frames()
            pt.shade_probe_grid_states(coefficients=t_hist, states=t_rec, moments=t_dhist, resolution=R, normal_weight=True)
            got = pt.probe_grid_output()
            assert same(got, want) and got[fr.obj != -1][:, :3].any()
            assert same(t_hist.cpu().numpy().reshape(P, 9, 4), hist) and same(t_dhist.cpu().numpy().reshape(P, R * R, 4), dhist)
        finally:
            pt.wait()
            for k in ("records", "positions"):
                pt.bind_probe_states_output(k, None)
            pt.bind_probe_list_output(None)
            pt.bind_probe_list(None)
            pt.bind_probe_history("coefficients", None)
            pt.bind_probe_history("moments", None)
            pt.bind_probe_grid_states(None)
    finally:
        fr.close()


# ---- the layers above -----------------------------------------------------------------------------------------------------------------
def test_host_library_and_cli_give_the_bytes_of_the_c_calls(srt, oracle, tmp_path):
    import os
    import subprocess

    from conftest import ROOT, scene_path

    W, H, FRAMES, K = 24, 20, 3, 64
    fr = Frame(srt, oracle, scene1(oracle))
    pt = fr.pt
    try:
        grid = PG.Grid((-4.0, -1.5, 1.0), (1.0, 1.0, 1.0), (5, 4, 5))
        P = grid.probes
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        pt.classify_probes(directions=K, relocate=True, positions=True)
        rec, pos = pt.probe_states_output("records"), pt.probe_states_output("positions")
        pt.bind_probe_grid_states(rec)
        pt.list_probes(count_work=True)
        words, lwork = pt.probe_list_output(P), pt.probe_list_work()
        pt.bind_probe_list(words)
        pt.trace_light_probes(pos, None, samples=1, bounces=0)  # (the positions)
        pt.reset_probe_history(P, 8)
        for f in range(1, FRAMES + 1):
            pt.trace_light_probes(samples=2, bounces=2, seed=f, listed=True)
            pt.trace_probe_depth(resolution=8, listed=True)
            pt.blend_probes(hysteresis=0.75, depth_hysteresis=0.75, moments=True, listed=True, count_work=True)
        hist, dhist, bwork = pt.probe_history("coefficients"), pt.probe_history("moments"), pt.probe_blend_work()
        pt.shade_probe_grid_states(coefficients=hist, states=rec, moments=dhist)
        want = pt.probe_grid_output()
        assert want[fr.obj != -1][:, :3].any()
    finally:
        fr.close()
    r = srt.host.Renderer(W, H)
    try:
        r.set_scene(srt.host.Scene(scene_path("Scene1")))
        r.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        hrec, hpos = r.classify_probes(P, K, relocate=True, positions=True)
        assert same(hrec, rec) and same(hpos, pos)
        assert same(r.list_probes(hrec, count_work=True), words) and r.probe_list_work() == lwork
        r.reset_probe_history(P, 8)
        for f in range(1, FRAMES + 1):
            r.trace_light_probes_listed(hpos if f == 1 else None, K if f == 1 else None, samples=2, bounces=2, seed=f)
            r.trace_probe_depth_listed(resolution=8)
            r.blend_probes(hysteresis=0.75, depth_hysteresis=0.75, moments=True, listed=True, count_work=True)
        assert same(r.probe_history("coefficients"), hist) and same(r.probe_history("moments"), dhist) and r.probe_blend_work() == bwork
        assert same(r.shade_probe_grid_states(hist, hrec, dhist), want)
    finally:
        r.close()
    cli = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
    out = tmp_path / "irradiance.f32"
    base = [cli, "--scene", scene_path("Scene1"), "--width", str(W), "--height", str(H), "--probe-grid", "-4,-1.5,1,1,1,1,5,4,5", "--probe-directions", str(K),
            "--bounces", "2", "--irradiance-out", str(out)]
    run = subprocess.run(base + ["--probe-classify", "--probe-relocate", "--probe-depth", "8", "--probe-update", str(FRAMES), "--probe-hysteresis", "0.75",
                                 "--probe-samples", "2"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert out.read_bytes() == want.tobytes()
    out.unlink()
    for extra in (["--probe-update", "3"], ["--probe-classify", "--probe-samples", "2"], ["--probe-classify", "--probe-update", "0"],
                  ["--probe-classify", "--probe-update", "2", "--probe-hysteresis", "1"]):
        run = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert run.returncode == 2 and "--probe-update" in run.stderr and not out.exists(), (extra, run.returncode, run.stderr)


def test_cli_probe_update_with_a_moving_object_gives_the_bytes_of_the_python_route(srt, oracle, tmp_path):
    """srt_render --probe-update --move-object: before every frame but the first the object moves (srt_update_scene), the grid is
    classified and listed again, and the blend gets the records of the frame before (SRT_PROBE_BLEND_PREVIOUS_STATES)."""
    import ctypes as C
    import os
    import re
    import subprocess

    from conftest import ROOT, scene_path

    W, H, FRAMES, K, OBJ = 24, 20, 4, 64, 64  # object 64: the unit sphere at (0, 0, 5)
    step = (F(0.5), F(0.0), F(-0.25))
    objs = scene1(oracle)[0]
    fr = Frame(srt, oracle, (objs, None))
    pt = fr.pt
    try:
        grid = PG.Grid((-4.0, -1.5, 1.0), (1.0, 1.0, 1.0), (5, 4, 5))
        P = grid.probes
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        pt.reset_probe_history(P, 8)
        rec, works = None, []
        for f in range(1, FRAMES + 1):
            moved = f > 1
            if moved:
                objs[OBJ]["position"] = tuple(float(F(p) + s) for p, s in zip(objs[OBJ]["position"], step))
                oarr, n = oracle.make_objects(objs)
                pt.update_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
                pt.bind_probe_previous_states(rec)
            pt.classify_probes(directions=K, relocate=True, positions=True)
            rec, pos = pt.probe_states_output("records"), pt.probe_states_output("positions")
            pt.bind_probe_grid_states(rec)
            pt.list_probes()
            pt.bind_probe_list(pt.probe_list_output(P))
            pt.trace_light_probes(pos, None, samples=2, bounces=2, seed=f, listed=True)
            pt.trace_probe_depth(resolution=8, listed=True)
            pt.blend_probes(hysteresis=0.75, depth_hysteresis=0.75, moments=True, listed=True, previous_states=moved, count_work=moved)
            if moved:
                works.append(pt.probe_blend_work())
        # the condition on the inputs: the move changes records, so that probes restart that a blend without the previous records keeps
        assert sum(w["restarted"] for w in works) >= 3
        hist, dhist = pt.probe_history("coefficients"), pt.probe_history("moments")
        pt.render_gbuffer(outputs=["object", "normal_depth", "position"])
        pt.shade_probe_grid_states(coefficients=hist, states=rec, moments=dhist)
        want = pt.probe_grid_output()
    finally:
        fr.close()
    cli = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
    out, sout = tmp_path / "irradiance.f32", tmp_path / "states.f32"
    run = subprocess.run([cli, "--scene", scene_path("Scene1"), "--width", str(W), "--height", str(H), "--probe-grid", "-4,-1.5,1,1,1,1,5,4,5", "--probe-directions", str(K),
                          "--bounces", "2", "--irradiance-out", str(out), "--probe-classify", "--probe-relocate", "--states-out", str(sout), "--probe-depth", "8",
                          "--probe-update", str(FRAMES), "--probe-hysteresis", "0.75", "--probe-samples", "2", "--move-object", "%d:0.5,0,-0.25" % OBJ],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert out.read_bytes() == want.tobytes() and sout.read_bytes() == rec.tobytes()
    got = [tuple(int(v) for v in m) for m in re.findall(r"probe update frame \d+: (\d+) probes blended, (\d+) restarted, (\d+) changed", run.stderr)]
    assert got == [(w["probes"], w["restarted"], w["changed"]) for w in works]
