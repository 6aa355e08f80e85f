"""Probe-grid shading with the filtered visibility test (srt_shade_probe_grid_depth, ABI 7) on the MI355X.  Every comparison is bit
for bit over all four lanes of every pixel.  The expected image and the work counts are tests/probe_depth_reference.py's shade()
(rule 7b on top of tests/probe_grid_reference.py) on the frame's guides; the moments are synthetic (uniform, so that both sides of
the L > m1 + bias branch are taken) or come from srt_trace_probe_depth at the grid's own probe positions."""
import ctypes as C
import itertools

import numpy as np
import pytest

import probe_depth_reference as PD
import probe_grid_reference as PG
from test_gpu_probe_grid import H, SENTINEL, W, check as check_exact, covering_grid, random_coefficients, same, with_albedo
from test_gpu_visibility import Frame, mesh_scene, scene1

pytestmark = pytest.mark.gpu

F = np.float32
DEPTH_FLAGS = [sum(c) for k in range(3) for c in itertools.combinations((PG.NORMAL_WEIGHT, PG.ALBEDO), k)]


def synthetic_moments(probes, R, seed=21, lo=4.0, hi=15.0):
    """(probes, R*R, 4): m1 uniform in [lo, hi], m2 = m1^2 + uniform[0, 0.5], the other two lanes arbitrary.  The range of m1 is
    chosen for the branch coverage condition: Scene1's ground is a sphere of radius 1000, so a grid that covers the frame's hit points
    has cells metres wide, and the corner distances L of covering_grid((4, 3, 5)) run from 0.09 to 17.5 with the 10th, 50th and 90th
    percentile at 6.3, 9.4 and 12.2 (the CPU oracle's guides).  With m1 in [0.2, 3] 99 % of the corners would take the L > m1 + bias
    branch; with [4, 15] about half do."""
    rng = np.random.default_rng(seed)
    m = np.empty((probes, R * R, 4), dtype=F)
    m1 = rng.uniform(lo, hi, (probes, R * R))
    m[..., 0] = m1
    m[..., 1] = m1 * m1 + rng.uniform(0.0, 0.5, (probes, R * R))
    m[..., 2:] = rng.uniform(0.0, 4.0, (probes, R * R, 2))
    return m


def kwargs(flags):
    return dict(normal_weight=bool(flags & PG.NORMAL_WEIGHT), albedo=bool(flags & PG.ALBEDO))


def check(fr, grid, coeff, depth, R, flags, band_weight=PG.IRRADIANCE, bias=0.0, min_variance=1e-4, write=True):
    """One counting call against the reference; returns (image, work, reference counts)."""
    pt = fr.pt
    want, counts = PD.shade(grid, coeff, depth, R, fr.obj, fr.nd, fr.pos, albedo=getattr(fr, "alb", None), flags=flags, band_weight=band_weight, bias=bias,
                            min_variance=min_variance)
    pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
    pt.shade_probe_grid_depth(coefficients=coeff if write else None, moments=depth if write else None, resolution=R, bias=bias, min_variance=min_variance,
                              band_weight=band_weight, count_work=True, **kwargs(flags))
    got, work = pt.probe_grid_output(), pt.probe_grid_work()
    print("flags %d counts %s R %d: work %s, branch taken at %d corners" % (flags, grid.counts, R, work, counts["taken"]))
    assert same(got, want), "differs from the reference at %d pixels" % int((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum())
    assert work["valid"] == 1 and work["waves"] > 0
    assert {k: work[k] for k in ("pixels", "corners", "segments", "open", "wave_trips")} == {k: counts[k] for k in ("pixels", "corners", "segments", "open", "wave_trips")}
    assert work["analytic_tests"] == work["node_visits"] == work["triangle_tests"] == 0
    return got, work, counts


@pytest.fixture(scope="module")
def frame1(srt, oracle):
    fr = with_albedo(Frame(srt, oracle, scene1(oracle)))
    assert fr.hits == 295
    yield fr
    fr.close()


# ---- synthetic moments: every accepted flag combination, both band weights, every resolution ----------------------------------------------
@pytest.mark.parametrize("flags", DEPTH_FLAGS)
def test_every_flag_combination_with_synthetic_moments(frame1, flags):
    fr = frame1
    grid = covering_grid(fr, (4, 3, 5))
    coeff = random_coefficients(grid.probes)
    for R in (16, 8, 4):
        depth = synthetic_moments(grid.probes, R)
        got, work, counts = check(fr, grid, coeff, depth, R, flags)
        # the branch coverage condition: both sides of L > m1 + bias are taken, and the weight decides something
        assert 0.1 * counts["corners"] <= counts["taken"] <= 0.9 * counts["corners"]
        assert 0 < work["open"] <= work["segments"] == work["corners"]
        hem, _, _ = check(fr, grid, coeff, depth, R, flags, band_weight=PG.HEMISPHERE, write=False)
        assert not same(got, hem) and same(got[..., 3], hem[..., 3])
        hit = fr.obj != -1
        assert not got[~hit].view(np.uint32).any() and work["pixels"] == fr.hits
        # turning COUNT_WORK off changes no output bit, and the same call twice gives the same bits
        for _ in range(2):
            fr.pt.shade_probe_grid_depth(**kwargs(flags))
            assert same(fr.pt.probe_grid_output(), got)
    # a bias and a variance floor that matter
    depth = synthetic_moments(grid.probes, 16)
    plain, _, _ = check(fr, grid, coeff, depth, 16, flags)
    biased, _, c2 = check(fr, grid, coeff, depth, 16, flags, bias=0.75, min_variance=0.3)
    assert not same(plain, biased) and 0 < c2["taken"] < c2["corners"]


def test_the_filtered_weight_differs_from_no_test_and_leaves_the_exact_call_s_bits(frame1):
    fr, pt = frame1, frame1.pt
    grid = covering_grid(fr, (4, 3, 5))
    coeff = random_coefficients(grid.probes)
    flags = PG.VISIBILITY | PG.NORMAL_WEIGHT
    before, _ = check_exact(fr, grid, coeff, flags)  # srt_shade_probe_grid against its own reference
    none, _ = check_exact(fr, grid, coeff, PG.NORMAL_WEIGHT)
    depth = synthetic_moments(grid.probes, 8)
    got, _, _ = check(fr, grid, coeff, depth, 8, PG.NORMAL_WEIGHT)
    assert not same(got, none) and not same(got, before)
    after, _ = check_exact(fr, grid, coeff, flags, write=False)
    assert same(after, before)
    # moments that say "nothing nearer than far away" switch the test off: the bits of the call without any test
    far = np.zeros((grid.probes, 64, 4), dtype=F)
    far[..., 0], far[..., 1] = 1e4, 1e8
    open_, work, counts = check(fr, grid, coeff, far, 8, PG.NORMAL_WEIGHT)
    assert same(open_, none) and counts["taken"] == 0 and work["open"] == work["segments"]


# ---- real moments, bound device to device -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,counts", [(scene1, (4, 3, 5)), (mesh_scene, (5, 4, 5))])
def test_moments_traced_on_the_grid_s_positions_and_bound_without_a_copy(srt, oracle, scene, counts):
    import torch

    fr = with_albedo(Frame(srt, oracle, scene(oracle)))
    pt = fr.pt
    grid = covering_grid(fr, counts)
    positions = srt.probe_grid_positions(grid.origin, grid.spacing, grid.counts)
    R = 8
    t = torch.zeros((grid.probes * R * R, 4), dtype=torch.float32, device="cuda:%d" % pt.device)
    try:
        diag = float(np.sqrt((grid.spacing.astype(np.float64) ** 2).sum()))
        pt.bind_probe_depth_output("moments", t)
        pt.trace_probe_depth(positions, 128, resolution=R, sharpness=4, max_distance=1.5 * diag)
        depth = pt.probe_depth_output("moments")
        assert np.isfinite(depth).all() and depth.any()
        coeff = random_coefficients(grid.probes, 31)
        flags = PG.NORMAL_WEIGHT | PG.ALBEDO
        want, cnt = PD.shade(grid, coeff, depth, R, fr.obj, fr.nd, fr.pos, albedo=fr.alb, flags=flags, bias=0.05 * diag)
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        pt.shade_probe_grid_depth(coefficients=coeff, moments=t, resolution=R, bias=0.05 * diag, count_work=True, **kwargs(flags))  # the device tensor
        got, work = pt.probe_grid_output(), pt.probe_grid_work()
        print("real moments: work %s, branch taken at %d corners" % (work, cnt["taken"]))
        assert same(got, want)
        assert (work["segments"], work["open"]) == (cnt["segments"], cnt["open"]) and 0 < cnt["taken"] < cnt["corners"]
        # written moments give the same bits as bound ones, and the depth output is still the trace's to read
        pt.shade_probe_grid_depth(moments=depth, bias=0.05 * diag, **kwargs(flags))
        assert same(pt.probe_grid_output(), got) and same(pt.probe_depth_output("moments"), depth)
    finally:
        pt.wait()
        pt.bind_probe_depth_output("moments", None)
        pt.bind_probe_grid_depth(None)
        fr.close()


# ---- bands, grids, bad moments ------------------------------------------------------------------------------------------------------------------
def test_a_partial_band_a_bound_output_and_a_grid_with_a_one_probe_axis(frame1):
    import torch

    fr, pt = frame1, frame1.pt
    grid = covering_grid(fr, (4, 3, 5))
    coeff = random_coefficients(grid.probes, 16)
    depth = synthetic_moments(grid.probes, 16, 22)
    flags = PG.ALBEDO
    full, _, _ = check(fr, grid, coeff, depth, 16, flags)
    big = torch.full((W * H + 70, 4), SENTINEL, dtype=torch.float32, device="cuda:%d" % pt.device)
    view = big[:W * H].view(H, W, 4)
    torch.cuda.synchronize()
    try:
        pt.shade_probe_grid_depth(output=view, rows=(0, 7), count_work=True, **kwargs(flags))
        pt.wait()
        g = big.cpu().numpy()
        img = g[:W * H].reshape(H, W, 4)
        assert same(img[H - 7:], full[H - 7:]) and np.all(img[:H - 7] == SENTINEL) and np.all(g[W * H:] == SENTINEL)
        _, cnt = PD.shade(grid, coeff, depth, 16, fr.obj, fr.nd, fr.pos, albedo=fr.alb, flags=flags, rows=(0, 7))
        work = pt.probe_grid_work()
        assert {k: work[k] for k in ("pixels", "corners", "segments", "open", "wave_trips")} == {k: cnt[k] for k in ("pixels", "corners", "segments", "open", "wave_trips")}
        pt.shade_probe_grid_depth(rows=(7, 20), **kwargs(flags))  # the second band completes the frame
        pt.wait()
        g = big.cpu().numpy()
        assert same(g[:W * H].reshape(H, W, 4), full) and np.all(g[W * H:] == SENTINEL)
    finally:
        pt.wait()
        pt.bind_probe_grid_output(None)
    for counts in ((1, 4, 1), (4, 1, 5)):
        grid = covering_grid(fr, counts)
        lo, hi = (15.0, 40.0) if counts == (1, 4, 1) else (4.0, 15.0)  # (one column of probes: L runs from 17.6 to 57)
        _, work, cnt = check(fr, grid, random_coefficients(grid.probes, 8), synthetic_moments(grid.probes, 4, 23, lo, hi), 4, PG.NORMAL_WEIGHT)
        assert work["corners"] <= 4 * fr.hits and 0 < cnt["taken"] < cnt["corners"]


def test_moments_that_are_not_finite_give_some_value_and_no_fault(frame1):
    fr, pt = frame1, frame1.pt
    grid = covering_grid(fr, (4, 3, 5))
    coeff = random_coefficients(grid.probes, 17)
    depth = synthetic_moments(grid.probes, 8, 24)
    bad = depth.copy()
    rng = np.random.default_rng(25)
    pick = rng.integers(0, 6, bad.shape[:2])
    bad[..., 0] = np.where(pick == 0, np.nan, np.where(pick == 1, np.inf, np.where(pick == 2, -np.inf, bad[..., 0])))
    bad[..., 1] = np.where(pick == 3, np.nan, np.where(pick == 4, np.inf, bad[..., 1]))
    pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
    pt.shade_probe_grid_depth(coefficients=coeff, moments=bad, resolution=8, count_work=True)
    pt.wait()
    got, work = pt.probe_grid_output(), pt.probe_grid_work()
    assert got.shape == (H, W, 4) and work["pixels"] == fr.hits and work["open"] <= work["segments"]
    assert not got[fr.obj == -1].view(np.uint32).any()
    # and the pass still works afterwards
    check(fr, grid, coeff, depth, 8, 0)


# ---- errors ---------------------------------------------------------------------------------------------------------------------------------------
def test_visibility_is_refused_and_the_extra_errors_come_in_order(srt, oracle):
    c = srt.capi
    oarr, n = oracle.make_objects(scene1(oracle)[0])
    pt = srt.PathTracer(W, H)
    L = pt.L
    fptr = C.POINTER(C.c_float)
    nan, inf = float("nan"), float("inf")

    def call(depth=None, **kw):
        p = c.ProbeGridParams()
        assert L.srt_probe_grid_params_default(C.byref(p)) == c.OK
        p.row_begin, p.row_end = 0, H
        for k, v in kw.items():
            if k in ("band_weight", "reserved"):
                getattr(p, k)[:] = v
            else:
                setattr(p, k, v)
        d = c.ProbeGridDepthParams()
        assert L.srt_probe_grid_depth_params_default(C.byref(d)) == c.OK
        for k, v in (depth or {}).items():
            if k == "reserved":
                d.reserved[:] = v
            else:
                setattr(d, k, v)
        return L.srt_shade_probe_grid_depth(pt._h, C.byref(p), C.byref(d))

    def why():
        return L.srt_last_error(pt._h)

    try:
        coeff = random_coefficients(75, 18)
        depth = synthetic_moments(75, 4, 26)
        assert call(flags=16) == c.ERR_STATE and b"srt_set_scene" in why()
        pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
        for kw in (dict(row_begin=-1), dict(row_end=H + 1), dict(flags=16), dict(flags=c.PROBE_GRID_VISIBILITY), dict(flags=c.PROBE_GRID_VISIBILITY | c.PROBE_GRID_ALBEDO),
                   dict(reserved=(1, 0)), dict(band_weight=(nan, 1, 1))):
            assert call(**kw) == c.ERR_INVALID_ARG, kw
        assert call(flags=c.PROBE_GRID_VISIBILITY) == c.ERR_INVALID_ARG and b"exclude each other" in why()
        assert call(depth=dict(bias=-1.0)) == c.ERR_STATE and b"no grid" in why()  # rule 16 comes first
        pt.set_probe_grid((-4.0, -1.2, 2.0), (2.0, 1.5, 2.0), (5, 3, 5))
        assert call() == c.ERR_STATE and b"no coefficients" in why()
        assert L.srt_write_probe_grid_coefficients(pt._h, coeff.ctypes.data_as(fptr), 75) == c.OK
        assert call() == c.ERR_STATE and b"OBJECT" in why()
        pt.set_camera(srt.default_camera())
        pt.render_gbuffer(outputs=["object", "normal_depth", "position"])
        assert call(depth=dict(bias=nan)) == c.ERR_STATE and b"no depth maps" in why()  # the maps come before the depth parameters
        # maps that are none are refused and leave none
        for probes, R in ((0, 4), (75, 5), (75, 0), (75, 32), ((1 << 26) + 1, 4)):
            assert L.srt_write_probe_grid_depth(pt._h, depth.ctypes.data_as(fptr), probes, R) == c.ERR_INVALID_ARG, (probes, R)
            assert L.srt_bind_probe_grid_depth(pt._h, 4096, probes, R) == c.ERR_INVALID_ARG, (probes, R)
        assert L.srt_write_probe_grid_depth(pt._h, None, 75, 4) == c.ERR_INVALID_ARG and L.srt_bind_probe_grid_depth(pt._h, None, 75, 4) == c.ERR_INVALID_ARG
        assert call() == c.ERR_STATE and b"no depth maps" in why()
        assert L.srt_write_probe_grid_depth(pt._h, depth.ctypes.data_as(fptr), 74, 4) == c.OK  # one probe short
        assert call(depth=dict(min_variance=0.0)) == c.ERR_STATE and b"depth probe count" in why()
        assert L.srt_write_probe_grid_depth(pt._h, depth.ctypes.data_as(fptr), 75, 4) == c.OK
        for dk in (dict(bias=-1e-6), dict(bias=nan), dict(bias=inf), dict(min_variance=0.0), dict(min_variance=-1.0), dict(min_variance=nan), dict(min_variance=inf),
                   dict(reserved=(1, 0)), dict(reserved=(0, 1))):
            assert call(depth=dk) == c.ERR_INVALID_ARG, dk
        buf = np.empty((H, W, 4), F)
        assert L.srt_read_probe_grid_output(pt._h, buf.ctypes.data_as(fptr)) == c.ERR_STATE  # nothing was touched
        assert call(flags=c.PROBE_GRID_COUNT_WORK) == c.OK
        good, work = pt.probe_grid_output(), pt.probe_grid_work()
        assert good[..., 3].any() and work["segments"] == work["corners"] > 0
        for kw, dk in ((dict(flags=c.PROBE_GRID_VISIBILITY), None), (dict(), dict(bias=-1.0)), (dict(row_begin=-1), None)):
            assert call(depth=dk, **kw) == c.ERR_INVALID_ARG
            assert same(pt.probe_grid_output(), good) and pt.probe_grid_work() == work
        assert call(depth=dict(bias=0.0)) == c.OK and call(depth=dict(bias=2.5, min_variance=1e-30)) == c.OK
        assert L.srt_shade_probe_grid_depth(pt._h, None, None) == c.ERR_INVALID_ARG
        assert L.srt_probe_grid_depth_params_default(None) == c.ERR_INVALID_ARG
        pt.wait()
    finally:
        pt.close()


# ---- the layers above ---------------------------------------------------------------------------------------------------------------------------
def test_host_library_and_cli_give_the_bytes_of_the_c_calls(srt, oracle, frame1, tmp_path):
    import os
    import subprocess

    from conftest import ROOT, scene_path

    fr, pt = frame1, frame1.pt
    grid = PG.Grid((-4.0, -1.0, 1.0), (2.0, 1.5, 2.0), (5, 3, 5))
    positions = srt.probe_grid_positions(grid.origin, grid.spacing, grid.counts)
    pt.trace_light_probes(positions, 64, samples=3, bounces=2, seed=13)
    coeff = pt.light_probe_coefficients()
    pt.trace_probe_depth(resolution=8, sharpness=4, max_distance=5.0, distances=True, count_work=True)
    depth, dist, dwork = pt.probe_depth_output("moments"), pt.probe_depth_output("distances"), pt.probe_depth_work()
    pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
    pt.shade_probe_grid_depth(coefficients=coeff, moments=depth, bias=0.25, normal_weight=True, albedo=True, band_weight=PG.HEMISPHERE, count_work=True)
    want, work = pt.probe_grid_output(), pt.probe_grid_work()
    assert 0 < work["open"] <= work["segments"]
    # host.py over PathTraceRenderer::traceProbeDepth / shadeProbeGridDepth: it renders the guides itself
    r = srt.host.Renderer(W, H)
    try:
        r.set_scene(srt.host.Scene(scene_path("Scene1")))
        assert same(r.trace_probe_depth(positions, 64, resolution=8, sharpness=4, max_distance=5.0, distances=True, count_work=True), depth)
        assert same(r.probe_depth_distances(), dist) and r.probe_depth_work() == dwork
        r.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        assert same(r.shade_probe_grid_depth(coeff, depth, bias=0.25, normal_weight=True, albedo=True, band_weight=PG.HEMISPHERE, count_work=True), want)
        assert r.probe_grid_work() == work
    finally:
        r.close()
    # the command-line tool: G-buffer, probes, depth maps, shading; W * H float4, scene rows, and the moments
    cli = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
    out, mout = tmp_path / "irradiance.f32", tmp_path / "moments.f32"
    base = [cli, "--scene", scene_path("Scene1"), "--width", str(W), "--height", str(H), "--probe-grid", "-4,-1,1,2,1.5,2,5,3,5", "--probe-directions", "64",
            "--radiance", "3", "--bounces", "2", "--seed", "13", "--irradiance-out", str(out)]
    run = subprocess.run(base + ["--probe-depth", "8", "--probe-depth-sharpness", "4", "--probe-depth-max", "5", "--probe-depth-bias", "0.25", "--probe-normal-weight",
                                 "--probe-albedo", "--probe-hemisphere", "--probe-depth-out", str(mout)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert out.read_bytes() == want.tobytes() and mout.read_bytes() == depth.tobytes()
    out.unlink()
    for extra in (["--probe-depth", "8", "--probe-visibility"], ["--probe-depth", "5"], ["--probe-depth-bias", "0.1"], ["--probe-depth", "8", "--probe-depth-sharpness", "7"],
                  ["--probe-depth", "8", "--probe-depth-max", "0"], ["--probe-depth", "8", "--probe-depth-bias", "-1"]):
        run = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert run.returncode == 2 and "--probe-depth" in run.stderr and not out.exists(), (extra, run.returncode, run.stderr)
