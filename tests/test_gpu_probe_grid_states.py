"""Probe-grid shading that obeys the probe records (srt_shade_probe_grid_states, ABI 7) on the MI355X.  Every comparison is bit for
bit over all four lanes of every pixel.  All-zero records must reproduce srt_shade_probe_grid and srt_shade_probe_grid_depth as the
device computes them; random records (offsets within 0.45 of the spacing, about 30 % buried, one pixel with all eight corners
buried) go against tests/probe_states_reference.py's shade(); records of srt_classify_probes are bound device to device; the
three existing shading calls return the bits they returned before; and all three calls, which share one device body, go against
their references on tiles whose hit counts lie on both sides of a trip boundary."""
import ctypes as C
import itertools

import numpy as np
import pytest

import probe_grid_reference as PG
import probe_states_reference as PS
from test_gpu_probe_grid import H, W, check as check_exact, covering_grid, random_coefficients, same, with_albedo
from test_gpu_probe_grid_depth import check as check_depth, synthetic_moments
from test_gpu_visibility import Frame, scene1

pytestmark = pytest.mark.gpu

F = np.float32
FLAGS = [sum(c) for k in range(3) for c in itertools.combinations((PG.NORMAL_WEIGHT, PG.ALBEDO), k)]
COUNTS = ("pixels", "corners", "segments", "open", "wave_trips")


def kwargs(flags):
    return dict(normal_weight=bool(flags & PG.NORMAL_WEIGHT), albedo=bool(flags & PG.ALBEDO))


def random_records(fr, grid, seed=41):
    """(P, 4): offsets uniform within +-0.45 spacing, about 30 % BURIED, the other state bits at random (they are not looked at);
    the eight corner probes of the first hit pixel are all BURIED."""
    rng = np.random.default_rng(seed)
    rec = np.zeros((grid.probes, 4), dtype=F)
    rec[:, :3] = rng.uniform(-0.45, 0.45, (grid.probes, 3)) * grid.spacing.astype(np.float64)[None, :]
    bits = (rng.integers(0, 16, grid.probes).astype(np.uint32) & ~np.uint32(PS.BURIED)) | np.where(rng.random(grid.probes) < 0.3, PS.BURIED, 0).astype(np.uint32)
    pix = buried_pixel(fr, grid)
    c = PG.corners(grid, fr.pos.reshape(-1, 4)[[pix], :3], fr.nd.reshape(-1, 4)[[pix], :3])
    bits[c["probe"].reshape(-1)] |= PS.BURIED
    rec[:, 3] = bits.view(F)
    return rec


def buried_pixel(fr, grid):
    """The hit pixel whose corners random_records() buries: the first one of the cell that holds the fewest hit pixels."""
    pix = np.flatnonzero(fr.obj.reshape(-1) != -1)
    i, _ = PG.cells(grid, fr.pos.reshape(-1, 4)[pix, :3])
    _, inverse, count = np.unique(i, axis=0, return_inverse=True, return_counts=True)
    return int(pix[np.flatnonzero(count[inverse.reshape(-1)] == count.min())[0]])


def check(fr, grid, coeff, rec, flags, depth=None, R=None, band_weight=PG.IRRADIANCE, bias=0.0, min_variance=1e-4, write=True):
    """One counting call against the reference; returns (image, work, reference counts)."""
    pt = fr.pt
    want, counts = PS.shade(grid, coeff, rec, fr.obj, fr.nd, fr.pos, albedo=getattr(fr, "alb", None), flags=flags, band_weight=band_weight, depth=depth, R=R, bias=bias,
                            min_variance=min_variance)
    pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
    pt.shade_probe_grid_states(coefficients=coeff if write else None, states=rec if write else None, moments=depth if write else None, depth=depth is not None,
                               resolution=R, bias=bias, min_variance=min_variance, band_weight=band_weight, count_work=True, **kwargs(flags))
    got, work = pt.probe_grid_output(), pt.probe_grid_work()
    print("flags %d depth %s: work %s, skipped by 3s %d, pixels with eight buried corners %d" % (flags, R, work, counts["skipped"], counts["all8"]))
    assert same(got, want), "differs from the reference at %d pixels" % int((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum())
    assert work["valid"] == 1 and work["waves"] > 0 and {k: work[k] for k in COUNTS} == {k: counts[k] for k in COUNTS}
    assert work["analytic_tests"] == work["node_visits"] == work["triangle_tests"] == 0
    return got, work, counts


@pytest.fixture(scope="module")
def frame1(srt, oracle):
    fr = with_albedo(Frame(srt, oracle, scene1(oracle)))
    assert fr.hits == 295
    yield fr
    fr.close()


# ---- all-zero records: the parent calls, bit for bit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
def test_zero_records_reproduce_the_parent_calls(frame1, flags):
    fr, pt = frame1, frame1.pt
    grid = covering_grid(fr, (4, 3, 5))
    coeff = random_coefficients(grid.probes)
    zero = np.zeros((grid.probes, 4), dtype=F)
    parent, pwork = check_exact(fr, grid, coeff, flags)  # srt_shade_probe_grid against its own reference
    got, work, _ = check(fr, grid, coeff, zero, flags)
    assert same(got, parent) and {k: work[k] for k in COUNTS} == {k: pwork[k] for k in COUNTS} and work["segments"] == work["open"] == 0
    for R in (4, 8, 16):
        depth = synthetic_moments(grid.probes, R)
        parent, pwork, _ = check_depth(fr, grid, coeff, depth, R, flags)  # srt_shade_probe_grid_depth against its own reference
        got, work, _ = check(fr, grid, coeff, zero, flags, depth=depth, R=R)
        assert same(got, parent) and {k: work[k] for k in COUNTS} == {k: pwork[k] for k in COUNTS}
    # the other state bits are not looked at
    other = zero.copy()
    other[:, 3] = np.full(grid.probes, PS.MOVED | PS.INSIDE | PS.IDLE, np.uint32).view(F)
    pt.shade_probe_grid_states(states=other, depth=True, **kwargs(flags))
    assert same(pt.probe_grid_output(), parent)


# ---- hit counts on both sides of a trip boundary: all three calls ---------------------------------------------------------------------
@pytest.mark.parametrize("hits", [(0, 1, 8), (9, 63, 64)])
def test_tiles_whose_hit_count_crosses_a_trip_boundary(srt, oracle, hits):
    """24 x 8: three tiles with `hits` hit pixels, scattered over the lanes, so that a tile takes 0, 1, 2 or 8 trips, the last one
    full, with one item or with seven; the lane that takes item 8 r + c past the last rank reads record 0, and the owner of rank r
    collects in trip r >> 3.  Synthetic guides with points inside a 3 x 3 x 3 grid around one small sphere (the any-hit query
    decides something, and the reference takes its bits from srt_trace_occlusion)."""
    import types

    import torch

    from test_gpu_visibility import one_pixel_scene

    w, h = 24, 8
    rng = np.random.default_rng(50 + sum(hits))
    obj = np.full((h, w), -1, np.int32)
    for tile, n in enumerate(hits):
        lanes = 1 + rng.choice(63, n, replace=False) if n < 64 else np.arange(64)  # (lane 0 misses: the ranks are not the lanes)
        obj[lanes >> 3, 8 * tile + (lanes & 7)] = 1
    hit = obj != -1
    assert [int(hit[:, 8 * t:8 * t + 8].sum()) for t in range(3)] == list(hits)
    grid = PG.Grid((-1.0, -1.0, 4.0), (1.0, 1.0, 1.0), (3, 3, 3))
    pos = np.zeros((h, w, 4), F)
    pos[..., :3] = rng.uniform(-0.95, 0.95, (h, w, 3)) + np.array([0.0, 0.0, 5.0])
    pos[..., 3] = 1.0
    nrm = rng.normal(size=(h, w, 3))
    nd = np.concatenate([nrm / np.linalg.norm(nrm, axis=2, keepdims=True), np.full((h, w, 1), 3.0)], -1).astype(F)
    alb = np.concatenate([rng.uniform(0.05, 0.9, (h, w, 3)), np.zeros((h, w, 1))], -1).astype(F)
    nd[~hit], pos[~hit], alb[~hit] = np.array([0, 0, 0, np.inf], F), 0, 0
    oarr, n = oracle.make_objects(one_pixel_scene(oracle)[0])  # a sphere of radius 0.3 at (0, 0, 5): the grid's centre
    pt = srt.PathTracer(w, h)
    keep = {k: torch.from_numpy(v).to("cuda:%d" % pt.device) for k, v in (("object", obj), ("normal_depth", nd), ("position", pos), ("albedo", alb))}
    torch.cuda.synchronize()
    try:
        pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
        for k, t in keep.items():
            pt.bind_gbuffer(k, t)
        fr = types.SimpleNamespace(pt=pt, obj=obj, nd=nd, pos=pos, alb=alb)
        coeff = random_coefficients(grid.probes, 51)
        depth = synthetic_moments(grid.probes, 4, 52, lo=0.3, hi=1.6)  # (the corner distances here run from 0 to 1.7)
        rec = random_records(fr, grid, 53)
        assert (rec[:, 3].view(np.uint32) & PS.BURIED).any()
        flags = PG.NORMAL_WEIGHT | PG.ALBEDO
        _, work = check_exact(fr, grid, coeff, flags)
        assert work["pixels"] == sum(hits) and work["wave_trips"] == sum((n + 7) // 8 for n in hits)
        _, vwork = check_exact(fr, grid, coeff, flags | PG.VISIBILITY, write=False)
        assert vwork["segments"] == work["corners"]
        check_depth(fr, grid, coeff, depth, 4, flags)
        check(fr, grid, coeff, rec, flags)
        check(fr, grid, coeff, rec, flags, depth=depth, R=4)
    finally:
        pt.wait()
        for k in keep:
            pt.bind_gbuffer(k, None)
        pt.close()


# ---- random records against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
def test_random_records_every_flag_combination_with_and_without_depth(frame1, flags):
    fr, pt = frame1, frame1.pt
    grid = covering_grid(fr, (4, 3, 5))
    coeff = random_coefficients(grid.probes, 19)
    rec = random_records(fr, grid)
    zero_img, _, _ = check(fr, grid, coeff, np.zeros_like(rec), flags)
    for depth, R in ((None, None), (synthetic_moments(grid.probes, 8, 27), 8), (synthetic_moments(grid.probes, 16, 28), 16)):
        got, work, counts = check(fr, grid, coeff, rec, flags, depth=depth, R=R)
        # the condition on the inputs: a pixel with all eight corners buried gets (0, 0, 0, 0), and rule 3s decides a tenth of the corners
        assert counts["all8"] >= 1 and counts["skipped"] >= 0.1 * (counts["skipped"] + counts["corners"])
        assert not got.reshape(-1, 4)[buried_pixel(fr, grid)].view(np.uint32).any()
        assert counts["corners"] >= 0.3 * (counts["skipped"] + counts["corners"])  # ... and leaves enough of them for rule 4s
        assert not same(got, zero_img)
        hem, _, _ = check(fr, grid, coeff, rec, flags, depth=depth, R=R, band_weight=PG.HEMISPHERE, write=False)
        assert not same(got, hem) and same(got[..., 3], hem[..., 3])
        # turning COUNT_WORK off changes no output bit, and the same call twice gives the same bits
        for _ in range(2):
            pt.shade_probe_grid_states(depth=depth is not None, **kwargs(flags))
            assert same(pt.probe_grid_output(), got)
    assert not got[fr.obj == -1].view(np.uint32).any()
    # offsets alone (nothing buried) already change the image: rule 4s
    moved = rec.copy()
    moved[:, 3] = 0.0
    got2, _, c2 = check(fr, grid, coeff, moved, flags | PG.NORMAL_WEIGHT)
    assert c2["skipped"] == 0 and not same(got2, check(fr, grid, coeff, np.zeros_like(rec), flags | PG.NORMAL_WEIGHT)[0])


def test_a_band_a_bound_output_and_records_that_are_not_finite(frame1):
    import torch

    from test_gpu_probe_grid import SENTINEL

    fr, pt = frame1, frame1.pt
    grid = covering_grid(fr, (4, 3, 5))
    coeff = random_coefficients(grid.probes, 20)
    rec = random_records(fr, grid, 42)
    depth = synthetic_moments(grid.probes, 4, 29)
    full, _, _ = check(fr, grid, coeff, rec, PG.ALBEDO, depth=depth, R=4)
    big = torch.full((W * H + 70, 4), SENTINEL, dtype=torch.float32, device="cuda:%d" % pt.device)
    torch.cuda.synchronize()
    try:
        pt.shade_probe_grid_states(output=big[:W * H].view(H, W, 4), rows=(0, 7), depth=True, albedo=True, count_work=True)
        pt.wait()
        g = big.cpu().numpy()
        img = g[:W * H].reshape(H, W, 4)
        assert same(img[H - 7:], full[H - 7:]) and np.all(img[:H - 7] == SENTINEL) and np.all(g[W * H:] == SENTINEL)
        _, cnt = PS.shade(grid, coeff, rec, fr.obj, fr.nd, fr.pos, albedo=fr.alb, flags=PG.ALBEDO, depth=depth, R=4, rows=(0, 7))
        work = pt.probe_grid_work()
        assert {k: work[k] for k in COUNTS} == {k: cnt[k] for k in COUNTS}
        pt.shade_probe_grid_states(rows=(7, 20), depth=True, albedo=True)
        pt.wait()
        g = big.cpu().numpy()
        assert same(g[:W * H].reshape(H, W, 4), full) and np.all(g[W * H:] == SENTINEL)
    finally:
        pt.wait()
        pt.bind_probe_grid_output(None)
    bad = rec.copy()
    pick = np.random.default_rng(43).integers(0, 5, bad.shape[0])
    bad[:, 0] = np.where(pick == 0, np.nan, np.where(pick == 1, np.inf, bad[:, 0]))
    bad[:, 2] = np.where(pick == 2, -np.inf, np.where(pick == 3, 1e30, bad[:, 2]))
    pt.shade_probe_grid_states(states=bad, depth=True, count_work=True)
    pt.wait()
    got, work = pt.probe_grid_output(), pt.probe_grid_work()
    assert got.shape == (H, W, 4) and work["pixels"] == fr.hits and not got[fr.obj == -1].view(np.uint32).any()
    check(fr, grid, coeff, rec, 0)  # and the pass still works afterwards


# ---- records of srt_classify_probes, bound device to device ---------------------------------------------------------------------------
def test_records_of_the_classification_bound_without_a_copy(srt, frame1):
    import torch

    fr, pt = frame1, frame1.pt
    grid = covering_grid(fr, (9, 5, 9))  # its lowest plane lies in the ground sphere wherever the ground is higher than its lowest hit point
    objs = scene1(fr.oracle)[0]
    d = srt.light_probe_sphere(64)
    want = PS.classify(grid, objs, d, PS.RELOCATE)
    assert want["work"]["buried"] >= 1
    t = torch.zeros((grid.probes, 4), dtype=torch.float32, device="cuda:%d" % pt.device)
    try:
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        pt.bind_probe_states_output("records", t)
        pt.classify_probes(directions=d, relocate=True)
        coeff = random_coefficients(grid.probes, 23)
        flags = PG.NORMAL_WEIGHT | PG.ALBEDO
        img, cnt = PS.shade(grid, coeff, want["records"], fr.obj, fr.nd, fr.pos, albedo=fr.alb, flags=flags)
        pt.shade_probe_grid_states(coefficients=coeff, states=t, count_work=True, **kwargs(flags))  # the device tensor
        got, work = pt.probe_grid_output(), pt.probe_grid_work()
        print("classified records: work %s, skipped %d, idle %d" % (work, cnt["skipped"], want["work"]["idle"]))
        assert same(got, img) and {k: work[k] for k in COUNTS} == {k: cnt[k] for k in COUNTS} and cnt["skipped"] > 0
        assert same(pt.probe_states_output("records"), want["records"])
        # in the reference no corner that enters a sum belongs to an IDLE probe
        idle = (want["state"] & PS.IDLE) != 0
        assert not idle[cnt["used"]].any()
        # written records give the same bits as bound ones
        pt.shade_probe_grid_states(states=want["records"], **kwargs(flags))
        assert same(pt.probe_grid_output(), got)
    finally:
        pt.wait()
        pt.bind_probe_states_output("records", None)
        pt.bind_probe_grid_states(None)


# ---- the existing calls, and errors ---------------------------------------------------------------------------------------------------
def test_the_three_existing_shading_calls_keep_their_bits_and_errors_come_in_order(srt, oracle, frame1):
    fr, pt = frame1, frame1.pt
    c = srt.capi
    grid = covering_grid(fr, (4, 3, 5))
    coeff = random_coefficients(grid.probes, 24)
    depth = synthetic_moments(grid.probes, 8, 30)
    before = [check_exact(fr, grid, coeff, 0)[0], check_exact(fr, grid, coeff, PG.VISIBILITY | PG.NORMAL_WEIGHT)[0], check_depth(fr, grid, coeff, depth, 8, PG.ALBEDO)[0]]
    check(fr, grid, coeff, random_records(fr, grid, 44), PG.NORMAL_WEIGHT, depth=depth, R=8)
    after = [check_exact(fr, grid, coeff, 0, write=False)[0], check_exact(fr, grid, coeff, PG.VISIBILITY | PG.NORMAL_WEIGHT, write=False)[0],
             check_depth(fr, grid, coeff, depth, 8, PG.ALBEDO, write=False)[0]]
    assert all(same(a, b) for a, b in zip(before, after))
    # errors on a fresh handle
    oarr, n = oracle.make_objects(scene1(oracle)[0])
    p2 = srt.PathTracer(W, H)
    L = p2.L
    fptr = C.POINTER(C.c_float)

    def call(with_depth=False, dkw=None, **kw):
        p = c.ProbeGridParams()
        assert L.srt_probe_grid_params_default(C.byref(p)) == c.OK
        p.row_begin, p.row_end = 0, H
        for k, v in kw.items():
            if k in ("band_weight", "reserved"):
                getattr(p, k)[:] = v
            else:
                setattr(p, k, v)
        if not with_depth:
            return L.srt_shade_probe_grid_states(p2._h, C.byref(p), None)
        d = c.ProbeGridDepthParams()
        assert L.srt_probe_grid_depth_params_default(C.byref(d)) == c.OK
        for k, v in (dkw or {}).items():
            setattr(d, k, v)
        return L.srt_shade_probe_grid_states(p2._h, C.byref(p), C.byref(d))

    def why():
        return L.srt_last_error(p2._h)

    try:
        rec = np.zeros((75, 4), F)
        assert call(flags=16) == c.ERR_STATE and b"srt_set_scene" in why()
        p2.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
        for kw in (dict(row_begin=-1), dict(flags=16), dict(flags=c.PROBE_GRID_VISIBILITY), dict(flags=c.PROBE_GRID_VISIBILITY | c.PROBE_GRID_ALBEDO), dict(reserved=(1, 0))):
            assert call(**kw) == c.ERR_INVALID_ARG and call(True, **kw) == c.ERR_INVALID_ARG, kw
        assert call(flags=c.PROBE_GRID_VISIBILITY) == c.ERR_INVALID_ARG and b"SRT_PROBE_GRID_VISIBILITY" in why()
        assert call() == c.ERR_STATE and b"no grid" in why()
        p2.set_probe_grid((-4.0, -1.2, 2.0), (2.0, 1.5, 2.0), (5, 3, 5))
        assert call() == c.ERR_STATE and b"no coefficients" in why()
        co = random_coefficients(75, 18)
        assert L.srt_write_probe_grid_coefficients(p2._h, co.ctypes.data_as(fptr), 75) == c.OK
        assert call() == c.ERR_STATE and b"OBJECT" in why()
        p2.set_camera(srt.default_camera())
        p2.render_gbuffer(outputs=["object", "normal_depth", "position"])
        assert call() == c.ERR_STATE and b"no states" in why()
        assert call(True) == c.ERR_STATE and b"no depth maps" in why()  # the parent call's errors come first
        for probes in (0, (1 << 30) + 1):
            assert L.srt_write_probe_grid_states(p2._h, rec.ctypes.data_as(fptr), probes) == c.ERR_INVALID_ARG
            assert L.srt_bind_probe_grid_states(p2._h, 4096, probes) == c.ERR_INVALID_ARG
        assert L.srt_write_probe_grid_states(p2._h, None, 75) == c.ERR_INVALID_ARG and L.srt_bind_probe_grid_states(p2._h, None, 75) == c.ERR_INVALID_ARG
        assert L.srt_write_probe_grid_states(p2._h, rec.ctypes.data_as(fptr), 74) == c.OK  # one probe short
        assert call() == c.ERR_STATE and b"state count" in why()
        assert L.srt_write_probe_grid_states(p2._h, rec.ctypes.data_as(fptr), 75) == c.OK
        mo = synthetic_moments(75, 4, 26)
        assert L.srt_write_probe_grid_depth(p2._h, mo.ctypes.data_as(fptr), 75, 4) == c.OK
        assert call(True, dict(bias=-1.0)) == c.ERR_INVALID_ARG
        buf = np.empty((H, W, 4), F)
        assert L.srt_read_probe_grid_output(p2._h, buf.ctypes.data_as(fptr)) == c.ERR_STATE  # nothing was touched
        assert call(flags=c.PROBE_GRID_COUNT_WORK) == c.OK
        good, work = p2.probe_grid_output(), p2.probe_grid_work()
        assert good[..., 3].any() and work["corners"] > 0 and work["segments"] == 0
        assert call(True, flags=c.PROBE_GRID_COUNT_WORK) == c.OK and p2.probe_grid_work()["segments"] == work["corners"]
        assert L.srt_shade_probe_grid_states(p2._h, None, None) == c.ERR_INVALID_ARG
        p2.wait()
    finally:
        p2.close()


# ---- the layers above -----------------------------------------------------------------------------------------------------------------
def test_host_library_and_cli_give_the_bytes_of_the_c_calls(srt, oracle, frame1, tmp_path):
    import os
    import subprocess

    from conftest import ROOT, scene_path

    fr, pt = frame1, frame1.pt
    grid = PG.Grid((-4.0, -1.5, 1.0), (1.0, 0.75, 1.0), (9, 5, 9))
    P = grid.probes
    pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
    pt.classify_probes(directions=64, relocate=True, clearance=0.2, max_offset=0.4, steps=5, count_work=True, positions=True)
    rec, pos, cwork = pt.probe_states_output("records"), pt.probe_states_output("positions"), pt.probe_states_work()
    assert cwork["moved"] >= 1 and cwork["buried"] >= 1
    pt.trace_light_probes(pos, 64, samples=3, bounces=2, seed=13)
    coeff = pt.light_probe_coefficients()
    pt.trace_probe_depth(resolution=8, sharpness=4, max_distance=5.0)
    depth = pt.probe_depth_output("moments")
    pt.shade_probe_grid_states(coefficients=coeff, states=rec, moments=depth, bias=0.25, normal_weight=True, albedo=True, band_weight=PG.HEMISPHERE, count_work=True)
    want, work = pt.probe_grid_output(), pt.probe_grid_work()
    pt.shade_probe_grid_states(albedo=True, band_weight=PG.HEMISPHERE)
    plain = pt.probe_grid_output()
    assert 0 < work["open"] <= work["segments"] and not same(plain, want)
    # host.py over PathTraceRenderer::classifyProbes / shadeProbeGridStates: it renders the guides itself
    r = srt.host.Renderer(W, H)
    try:
        r.set_scene(srt.host.Scene(scene_path("Scene1")))
        r.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        hrec, hpos = r.classify_probes(P, 64, relocate=True, clearance=0.2, max_offset=0.4, steps=5, count_work=True, positions=True)
        assert same(hrec, rec) and same(hpos, pos) and r.probe_states_work() == cwork
        assert same(r.shade_probe_grid_states(coeff, rec, depth, bias=0.25, normal_weight=True, albedo=True, band_weight=PG.HEMISPHERE, count_work=True), want)
        assert r.probe_grid_work() == work
        assert same(r.shade_probe_grid_states(albedo=True, band_weight=PG.HEMISPHERE), plain)
    finally:
        r.close()
    # the command-line tool: classification, probes and depth maps at the positions it gives, shading with the records
    cli = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
    out, sout = tmp_path / "irradiance.f32", tmp_path / "states.f32"
    base = [cli, "--scene", scene_path("Scene1"), "--width", str(W), "--height", str(H), "--probe-grid", "-4,-1.5,1,1,0.75,1,9,5,9", "--probe-directions", "64",
            "--radiance", "3", "--bounces", "2", "--seed", "13", "--irradiance-out", str(out), "--probe-albedo", "--probe-hemisphere"]
    classify = ["--probe-classify", "--probe-relocate", "--probe-clearance", "0.2", "--probe-max-offset", "0.4", "--probe-steps", "5", "--states-out", str(sout)]
    run = subprocess.run(base + classify + ["--probe-depth", "8", "--probe-depth-sharpness", "4", "--probe-depth-max", "5", "--probe-depth-bias", "0.25", "--probe-normal-weight"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert out.read_bytes() == want.tobytes() and sout.read_bytes() == rec.tobytes()
    run = subprocess.run(base + classify, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert out.read_bytes() == plain.tobytes()
    out.unlink()
    for extra in (["--probe-classify", "--probe-visibility"], ["--probe-relocate"], ["--probe-classify", "--probe-steps", "0"]):
        run = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert run.returncode == 2 and "--probe-classify" in run.stderr and not out.exists(), (extra, run.returncode, run.stderr)
