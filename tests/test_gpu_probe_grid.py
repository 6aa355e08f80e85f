"""Probe-grid shading (srt_shade_probe_grid, ABI 7) on the MI355X.  Every comparison is bit for bit over all four lanes of every
pixel, NaN compared by its bits.  The expected image is tests/probe_grid_reference.py (the header's rules 1-9 in numpy binary32)
with the visibility bits taken from srt_write_rays + srt_trace_occlusion on the reference's own segments: that pins the fused
pass against the existing any-hit query, as tests/test_gpu_visibility.py does for the visibility pass.  The work counts are
compared with the counts the reference derives (rule 17: wave_trips = sum over tiles of ceil(h / 8))."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import probe_grid_reference as PG
import visibility_reference as VR
from conftest import ROOT, scene_path
from test_gpu_visibility import Frame, closed_room, indirect_scene, mesh_scene, one_pixel_scene, scene1, sky_camera

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
F = np.float32
W, H = 24, 20
SENTINEL = -7.0
ALL_FLAGS = [sum(c) for k in range(4) for c in itertools.combinations((PG.VISIBILITY, PG.NORMAL_WEIGHT, PG.ALBEDO), k)]


def same(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def random_coefficients(probes, seed=7):
    return np.random.default_rng(seed).uniform(-1.0, 2.0, (probes, 9, 4)).astype(F)


def covering_grid(fr, counts, margin=0.05):
    """A grid of `counts` probes whose outer planes enclose every hit point of the frame."""
    p = fr.pos[fr.obj != -1][:, :3].astype(np.float64)
    lo, hi = p.min(axis=0) - margin, p.max(axis=0) + margin
    spacing = [(hi[a] - lo[a]) / (counts[a] - 1) if counts[a] > 1 else 1.0 for a in range(3)]
    return PG.Grid(lo, spacing, counts)


def with_albedo(fr):
    fr.pt.render_gbuffer()
    fr.alb = fr.pt.gbuffer("albedo")
    return fr


def kwargs(flags):
    return dict(visibility=bool(flags & PG.VISIBILITY), normal_weight=bool(flags & PG.NORMAL_WEIGHT), albedo=bool(flags & PG.ALBEDO))


def expected(fr, grid, coeff, flags, band_weight=PG.IRRADIANCE, rows=None):
    """(reference image, reference work counts): the visibility bits by srt_trace_occlusion on the reference's segments."""
    occ = None
    if flags & PG.VISIBILITY:
        _, _, O4, D4 = PG.segments(grid, fr.obj, fr.nd, fr.pos, flags)
        occ = VR.occluded_by_tracer(fr.pt, O4, D4)
    img = PG.shade(grid, coeff, fr.obj, fr.nd, fr.pos, albedo=getattr(fr, "alb", None), flags=flags, band_weight=band_weight, occluded=occ)
    return img, PG.work_formula(grid, fr.obj, fr.nd, fr.pos, flags, occ, rows=rows), occ


def check(fr, grid, coeff, flags, band_weight=PG.IRRADIANCE, write=True):
    """One counting call against the reference and the work formula; returns (image, work)."""
    pt = fr.pt
    want, (pixels, corners, segments, open_, trips), _ = expected(fr, grid, coeff, flags, band_weight)
    pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
    pt.shade_probe_grid(coefficients=coeff if write else None, band_weight=band_weight, count_work=True, **kwargs(flags))
    got, work = pt.probe_grid_output(), pt.probe_grid_work()
    print("flags %d counts %s: work %s" % (flags, grid.counts, work))
    assert same(got, want), "differs from the reference at %d pixels" % int((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum())
    assert work["valid"] == 1 and work["waves"] > 0
    assert (work["pixels"], work["corners"], work["segments"], work["open"], work["wave_trips"]) == (pixels, corners, segments, open_, trips)
    if not flags & PG.VISIBILITY:
        assert work["analytic_tests"] == work["node_visits"] == work["triangle_tests"] == 0
    return got, work


@pytest.fixture(scope="module")
def frame1(srt, oracle):
    """Scene1 (the LDS instantiation) at 24 x 20 with the default camera: partial tiles in both directions."""
    fr = with_albedo(Frame(srt, oracle, scene1(oracle)))
    assert fr.hits == 295
    yield fr
    fr.close()


# ---- every flag combination, both band weights --------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_every_flag_combination_on_scene1(frame1, flags):
    fr = frame1
    grid = covering_grid(fr, (4, 3, 5))
    coeff = random_coefficients(grid.probes)
    got, work = check(fr, grid, coeff, flags)
    hem, _ = check(fr, grid, coeff, flags, band_weight=PG.HEMISPHERE, write=False)
    assert not same(got, hem) and same(got[..., 3], hem[..., 3])
    hit = fr.obj != -1
    assert not got[~hit].view(np.uint32).any() and work["pixels"] == fr.hits
    if flags & PG.VISIBILITY:
        assert 0 < work["open"] < work["segments"]  # the query decides something here
    else:
        assert (got[hit][:, 3] > 0).all()
    # turning COUNT_WORK off changes no output bit, and the same call twice gives the same bits
    for _ in range(2):
        fr.pt.shade_probe_grid(**kwargs(flags))
        assert same(fr.pt.probe_grid_output(), got)


def test_coefficients_traced_on_the_grid_s_positions_and_bound_without_a_copy(srt, frame1):
    import torch

    fr, pt = frame1, frame1.pt
    grid = covering_grid(fr, (4, 3, 5))
    positions = srt.probe_grid_positions(grid.origin, grid.spacing, grid.counts)
    assert same(positions, PG.positions(grid))
    t = torch.zeros((grid.probes * 9, 4), dtype=torch.float32, device="cuda:0")
    try:
        pt.bind_light_probe_output("coefficients", t)
        pt.trace_light_probes(positions, 64, samples=2, bounces=3, seed=5)
        coeff = pt.light_probe_coefficients()
        assert np.isfinite(coeff).all() and coeff.any()
        flags = PG.VISIBILITY | PG.NORMAL_WEIGHT | PG.ALBEDO
        want, counts, _ = expected(fr, grid, coeff, flags, PG.HEMISPHERE)
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        pt.shade_probe_grid(coefficients=t, band_weight=PG.HEMISPHERE, count_work=True, **kwargs(flags))  # the device tensor: nothing crosses the bus
        got = pt.probe_grid_output()
        assert same(got, want)
        # written coefficients give the same bits as bound ones
        pt.shade_probe_grid(coefficients=coeff, band_weight=PG.HEMISPHERE, **kwargs(flags))
        assert same(pt.probe_grid_output(), got)
        # the light-probe output is still the trace's to read
        assert same(pt.light_probe_coefficients(), coeff)
    finally:
        pt.wait()
        pt.bind_light_probe_output("coefficients", None)
        pt.L.srt_bind_probe_grid_coefficients(pt._h, None, 0)


# ---- grids ------------------------------------------------------------------------------------------------------------------------------
def test_a_grid_with_one_probe_on_two_axes(frame1):
    fr = frame1
    grid = covering_grid(fr, (1, 4, 1))
    coeff = random_coefficients(grid.probes, 8)
    for flags in (0, PG.VISIBILITY | PG.NORMAL_WEIGHT):
        _, work = check(fr, grid, coeff, flags)
        assert work["corners"] <= 2 * fr.hits  # only corners 0 and 2 exist


def test_a_small_grid_that_covers_part_of_the_frame_clamps(frame1):
    fr = frame1
    grid = PG.Grid((-1.0, -1.2, 3.5), (1.5, 1.0, 2.0), (2, 2, 2))
    i, f = PG.cells(grid, fr.pos[fr.obj != -1][:, :3])
    assert ((f == 0) | (f == 1)).any(axis=1).sum() > 0 and ((f > 0) & (f < 1)).all(axis=1).sum() > 0  # clamped and interior pixels
    coeff = random_coefficients(grid.probes, 9)
    for flags in (0, PG.VISIBILITY, PG.NORMAL_WEIGHT | PG.ALBEDO):
        _, work = check(fr, grid, coeff, flags)
        assert work["corners"] < 8 * fr.hits


def test_a_probe_plane_through_the_floor_gives_corners_with_f_0(srt, oracle):
    fr = with_albedo(Frame(srt, oracle, mesh_scene(oracle)))
    # the box floor's top is y = -1: the probe plane iy = 0 lies in it, and hit points at or below it have f_y = 0
    grid = PG.Grid((-4.0, -1.0, 1.0), (2.0, 1.25, 2.0), (5, 3, 5))
    _, f = PG.cells(grid, fr.pos[fr.obj != -1][:, :3])
    assert 0 < int((f[:, 1] == 0).sum()) < fr.hits
    coeff = random_coefficients(grid.probes, 10)
    for flags in (0, PG.VISIBILITY, PG.VISIBILITY | PG.NORMAL_WEIGHT | PG.ALBEDO):
        _, work = check(fr, grid, coeff, flags)
        assert work["corners"] < 8 * fr.hits
    fr.close()


def test_a_grid_inside_the_ground_sphere_is_occluded_everywhere(frame1):
    fr = frame1
    grid = PG.Grid((-2.0, -6.0, 3.0), (1.0, 1.0, 1.0), (5, 3, 5))  # Scene1's ground: centre (0, -1001.2, 5), radius 1000
    coeff = random_coefficients(grid.probes, 11)
    got, work = check(fr, grid, coeff, PG.VISIBILITY)
    assert not got.view(np.uint32).any() and work["open"] == 0 and work["segments"] == work["corners"] > 0
    # the fall-back the header names: a second call without the query
    got, _ = check(fr, grid, coeff, 0)
    assert (got[fr.obj != -1][:, 3] > 0).all()


# ---- frames -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,hits", [(8, 8, 41), (9, 1, 9)])
def test_one_tile_and_a_partial_tile(srt, oracle, w, h, hits):
    fr = with_albedo(Frame(srt, oracle, scene1(oracle), w=w, h=h))
    assert fr.hits == hits
    grid = covering_grid(fr, (4, 3, 5))
    coeff = random_coefficients(grid.probes, 12)
    for flags in (0, PG.VISIBILITY | PG.NORMAL_WEIGHT | PG.ALBEDO):
        _, work = check(fr, grid, coeff, flags)
        assert work["wave_trips"] == ((hits + 7) // 8 if (w, h) == (8, 8) else 2)  # 9 x 1: tiles of 8 and 1 hit pixels
    fr.close()


def test_a_camera_that_sees_only_sky(srt, oracle):
    fr = Frame(srt, oracle, scene1(oracle), cam=sky_camera(srt))
    assert fr.hits == 0
    grid = PG.Grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2))
    fr.pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
    fr.pt.shade_probe_grid(coefficients=random_coefficients(8), visibility=True, count_work=True)
    work = fr.pt.probe_grid_work()
    assert not fr.pt.probe_grid_output().view(np.uint32).any()
    assert work["pixels"] == work["corners"] == work["segments"] == work["wave_trips"] == work["analytic_tests"] == 0 and work["valid"] == 1
    fr.close()


def test_a_frame_where_exactly_one_pixel_hits(srt, oracle):
    fr = with_albedo(Frame(srt, oracle, one_pixel_scene(oracle), w=8, h=8))
    assert fr.hits == 1 and fr.obj[4, 4] == 0
    grid = PG.Grid((-1.0, -1.0, 3.5), (2.0, 2.0, 2.0), (2, 2, 2))  # the hit point (0, 0, 4.7) is interior
    coeff = random_coefficients(8, 13)
    for flags in ALL_FLAGS:
        got, work = check(fr, grid, coeff, flags)
        assert work["pixels"] == 1 and work["corners"] == 8 and work["wave_trips"] == 1
        assert int((got[..., 3] != 0).sum()) == 1
    fr.close()


# ---- every instantiation ----------------------------------------------------------------------------------------------------------------
def test_scene_indirect_and_the_closed_room(srt, oracle):
    for scene in (indirect_scene, closed_room):
        fr = with_albedo(Frame(srt, oracle, scene(oracle)))
        grid = covering_grid(fr, (4, 3, 5))
        coeff = random_coefficients(grid.probes, 14)
        for flags in (0, PG.VISIBILITY, PG.VISIBILITY | PG.NORMAL_WEIGHT | PG.ALBEDO):
            _, work = check(fr, grid, coeff, flags)
        assert 0 < work["open"] < work["segments"]
        fr.close()


def test_a_mesh_over_a_box_floor_before_and_after_a_refit(srt, oracle):
    fr = with_albedo(Frame(srt, oracle, mesh_scene(oracle), refit=True))
    grid = PG.Grid((-3.0, -1.5, 2.0), (1.5, 1.0, 1.5), (5, 4, 5))
    coeff = random_coefficients(grid.probes, 15)
    flags = PG.VISIBILITY | PG.NORMAL_WEIGHT
    before, work = check(fr, grid, coeff, flags)
    assert work["node_visits"] > 0 and work["triangle_tests"] > 0 and 0 < work["open"] < work["segments"]
    moved = mesh_scene(oracle, at=(0.5, 0.25, 5.5))
    oarr2, n2 = oracle.make_objects(moved[0])
    fr.pt.update_scene(C.cast(oarr2, C.POINTER(srt.Object)), n2)
    assert fr.pt.update_info()["path"] == 2
    fr.oarr, fr.n = oarr2, n2
    fr.guides()
    with_albedo(fr)
    after, work2 = check(fr, grid, coeff, flags)
    fresh = with_albedo(Frame(srt, oracle, moved))
    assert np.array_equal(fresh.obj, fr.obj)
    got, work3 = check(fresh, grid, coeff, flags)
    assert same(got, after) and not same(before, after)
    assert {k: work3[k] for k in ("pixels", "corners", "segments", "open", "wave_trips")} == {k: work2[k] for k in ("pixels", "corners", "segments", "open", "wave_trips")}
    fresh.close()
    fr.close()


# ---- bands, bound outputs ---------------------------------------------------------------------------------------------------------------
def test_bands_a_bound_output_and_nothing_written_past_the_frame(frame1):
    import torch

    fr, pt = frame1, frame1.pt
    grid = covering_grid(fr, (4, 3, 5))
    coeff = random_coefficients(grid.probes, 16)
    flags = PG.VISIBILITY | PG.ALBEDO
    full, _ = check(fr, grid, coeff, flags)
    big = torch.full((W * H + 70, 4), SENTINEL, dtype=torch.float32, device="cuda:0")
    view = big[:W * H].view(H, W, 4)
    torch.cuda.synchronize()
    try:
        pt.shade_probe_grid(output=view, rows=(0, 7), count_work=True, **kwargs(flags))
        pt.wait()
        g = big.cpu().numpy()
        img = g[:W * H].reshape(H, W, 4)
        assert same(img[H - 7:], full[H - 7:]) and np.all(img[:H - 7] == SENTINEL) and np.all(g[W * H:] == SENTINEL)
        _, counts, _ = expected(fr, grid, coeff, flags, rows=(0, 7))
        work = pt.probe_grid_work()
        assert (work["pixels"], work["corners"], work["segments"], work["open"], work["wave_trips"]) == counts
        assert same(pt.probe_grid_output()[H - 7:], full[H - 7:])  # the read follows the binding
        pt.shade_probe_grid(rows=(7, 20), **kwargs(flags))  # the second band completes the frame
        pt.wait()
        g = big.cpu().numpy()
        assert same(g[:W * H].reshape(H, W, 4), full) and np.all(g[W * H:] == SENTINEL)
    finally:
        pt.wait()
        pt.bind_probe_grid_output(None)
    assert same(pt.probe_grid_output(), full)  # the own buffer still holds the last whole frame written into it
    pt.shade_probe_grid(**kwargs(flags))
    assert same(pt.probe_grid_output(), full)


# ---- isolation and errors -----------------------------------------------------------------------------------------------------------------
def test_the_pass_leaves_every_other_output_stats_and_the_launch_shape_alone(srt, oracle):
    w, h = 160, 96
    names = ("object", "normal_depth", "position", "albedo")
    fields = ("rays", "sample_chunks", "tile_rows", "chunk_samples", "shape_source", "path_samples")
    rng = np.random.default_rng(95)
    O4, D4 = VR.rays(rng.uniform((-5, -1, 0), (5, 4, 10), (500, 3)), VR.unit(rng.normal(size=(500, 3))), 4.0)
    probes = np.array([[0.0, 1.5, 3.0, 0.0], [-2.0, 0.2, 4.5, 0.0]], F)
    oarr, n = oracle.make_objects(scene1(oracle)[0])
    grid = PG.Grid((-4.0, -1.2, 2.0), (2.0, 1.5, 2.0), (5, 3, 5))
    runs = []
    for with_pass in (False, True):
        pt = srt.PathTracer(w, h)
        pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
        pt.set_camera(srt.default_camera())
        pt.render(spp=8, bounces=3, seed=5, count_rays=True, count_work=True)
        pt.render_gbuffer()
        pt.render_visibility(5, 3.0, count_work=True)
        pt.write_rays(O4, D4)
        pt.trace_rays()
        pt.trace_radiance(samples=2, bounces=2, seed=3)
        pt.trace_light_probes(probes, 64, samples=2, bounces=2, seed=4, radiance=True, count_work=True)

        def state():
            return (pt.accumulator(), pt.framebuffer(), {k: pt.gbuffer(k) for k in names}, {k: pt.ray_output(k) for k in srt.capi.RAY_OUTPUTS}, pt.stats(),
                    pt.work_counts().as_dict(), (pt.visibility("ao"), pt.visibility("sun"), pt.radiance(), pt.light_probe_coefficients(), pt.light_probe_radiance()),
                    (pt.visibility_work(), pt.light_probe_work()))

        before = state()
        if with_pass:
            pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
            pt.shade_probe_grid(coefficients=random_coefficients(grid.probes, 17), visibility=True, normal_weight=True, albedo=True, count_work=True)
            pt.wait()
            after = state()
            assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)) and np.array_equal(before[1], after[1])
            assert all(np.array_equal(before[2][k].view(np.uint32), after[2][k].view(np.uint32)) for k in names)
            assert all(np.array_equal(before[3][k].view(np.uint32), after[3][k].view(np.uint32)) for k in before[3])
            assert all(getattr(before[4], f) == getattr(after[4], f) for f in fields) and before[4].kernel_ms == after[4].kernel_ms
            assert before[5] == after[5] and before[7] == after[7]
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(before[6], after[6]))
            work = pt.probe_grid_work()
            assert 0 < work["open"] < work["segments"]
        pt.render(spp=8, first_sample=9, reset=False, bounces=3, seed=5, count_rays=True, count_work=True)
        st = pt.stats()
        runs.append(([getattr(st, f) for f in fields], pt.work_counts().as_dict(), pt.framebuffer(), pt.accumulator()))
        pt.close()
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1]
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32))


def test_errors_are_found_in_the_header_s_order_and_leave_the_previous_output_readable(srt, oracle):
    c = srt.capi
    oarr, n = oracle.make_objects(scene1(oracle)[0])
    pt = srt.PathTracer(W, H)
    L = pt.L
    fptr = C.POINTER(C.c_float)
    nan, inf = float("nan"), float("inf")

    def call(**kw):
        p = c.ProbeGridParams()
        assert L.srt_probe_grid_params_default(C.byref(p)) == c.OK
        p.row_begin, p.row_end = 0, H
        for k, v in kw.items():
            if k == "band_weight":
                p.band_weight[:] = v
            elif k == "reserved":
                p.reserved[:] = v
            else:
                setattr(p, k, v)
        return L.srt_shade_probe_grid(pt._h, C.byref(p))

    def why():
        return L.srt_last_error(pt._h)

    def set_grid(origin=(-4.0, -1.2, 2.0), spacing=(2.0, 1.5, 2.0), counts=(5, 3, 5)):
        g = c.ProbeGrid((C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), (C.c_int32 * 3)(*counts))
        return L.srt_set_probe_grid(pt._h, C.byref(g))

    try:
        w = c.ProbeGridWork()
        buf = np.empty((H, W, 4), F)
        coeff = random_coefficients(75, 18)
        assert call(flags=16) == c.ERR_STATE and b"srt_set_scene" in why()  # before srt_set_scene, whatever the arguments
        pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
        # the arguments come before the inputs
        for kw in (dict(row_begin=-1), dict(row_end=H + 1), dict(row_begin=7, row_end=7), dict(row_begin=9, row_end=3), dict(flags=16), dict(flags=0x80000001),
                   dict(reserved=(1, 0)), dict(reserved=(0, 1)), dict(band_weight=(nan, 1, 1)), dict(band_weight=(1, nan, 1)), dict(band_weight=(1, 1, nan))):
            assert call(**kw) == c.ERR_INVALID_ARG, kw
        assert call() == c.ERR_STATE and b"no grid" in why()
        # grids that are none are refused and leave no grid
        for kw in (dict(counts=(0, 3, 5)), dict(counts=(5, 3, -1)), dict(counts=(1 << 15, 1 << 15, 2)), dict(spacing=(nan, 1, 1)), dict(spacing=(1, inf, 1)),
                   dict(spacing=(1, 1, 0.0)), dict(spacing=(-1.0, 1, 1)), dict(origin=(0, nan, 0)), dict(origin=(inf, 0, 0))):
            assert set_grid(**kw) == c.ERR_INVALID_ARG, kw
        assert call() == c.ERR_STATE and b"no grid" in why()
        assert set_grid() == c.OK
        assert call() == c.ERR_STATE and b"no coefficients" in why()
        assert L.srt_write_probe_grid_coefficients(pt._h, coeff.ctypes.data_as(fptr), 0) == c.ERR_INVALID_ARG
        assert L.srt_write_probe_grid_coefficients(pt._h, None, 75) == c.ERR_INVALID_ARG
        assert L.srt_bind_probe_grid_coefficients(pt._h, None, 3) == c.ERR_INVALID_ARG and L.srt_bind_probe_grid_coefficients(pt._h, 4096, (1 << 30) + 1) == c.ERR_INVALID_ARG
        assert call() == c.ERR_STATE and b"no coefficients" in why()
        assert L.srt_write_probe_grid_coefficients(pt._h, coeff.ctypes.data_as(fptr), 74) == c.OK  # one probe short
        assert call() == c.ERR_STATE and b"OBJECT" in why()  # a missing guide comes before the count
        pt.set_camera(srt.default_camera())
        for have, missing in ((["object"], b"NORMAL_DEPTH"), (["object", "normal_depth"], b"POSITION")):
            pt.render_gbuffer(outputs=have)
            assert call() == c.ERR_STATE and missing in why()
        pt.render_gbuffer(outputs=["object", "normal_depth", "position"])
        assert call(flags=c.PROBE_GRID_ALBEDO) == c.ERR_STATE and b"ALBEDO" in why()
        assert call() == c.ERR_STATE and b"nx * ny * nz" in why()
        assert L.srt_read_probe_grid_output(pt._h, buf.ctypes.data_as(fptr)) == c.ERR_STATE and L.srt_get_probe_grid_work(pt._h, C.byref(w)) == c.ERR_STATE
        assert L.srt_write_probe_grid_coefficients(pt._h, coeff.ctypes.data_as(fptr), 75) == c.OK
        assert call(flags=c.PROBE_GRID_VISIBILITY | c.PROBE_GRID_COUNT_WORK) == c.OK
        good, work = pt.probe_grid_output(), pt.probe_grid_work()
        assert good[..., 3].any()
        # every refusal leaves the previous output and record readable
        for kw in (dict(row_begin=-1), dict(flags=16), dict(reserved=(0, 7)), dict(band_weight=(1, nan, 1)), dict(flags=c.PROBE_GRID_ALBEDO)):
            assert call(**kw) in (c.ERR_INVALID_ARG, c.ERR_STATE), kw
            assert same(pt.probe_grid_output(), good) and pt.probe_grid_work() == work, kw
        assert set_grid(counts=(5, 3, 4)) == c.OK and call() == c.ERR_STATE and same(pt.probe_grid_output(), good)
        assert set_grid(spacing=(0.0, 1, 1)) == c.ERR_INVALID_ARG and call() == c.ERR_STATE  # the refused grid left the previous one
        assert set_grid() == c.OK and call() == c.OK
        assert L.srt_get_probe_grid_work(pt._h, C.byref(w)) == c.ERR_STATE  # that call did not count
        # infinite band weights are not NaN: accepted
        assert call(band_weight=(inf, 1, 1)) == c.OK
        assert L.srt_shade_probe_grid(pt._h, None) == c.ERR_INVALID_ARG and L.srt_set_probe_grid(pt._h, None) == c.ERR_INVALID_ARG
        assert L.srt_read_probe_grid_output(pt._h, None) == c.ERR_INVALID_ARG and L.srt_get_probe_grid_work(pt._h, None) == c.ERR_INVALID_ARG
        pt.wait()
    finally:
        pt.close()


# ---- the layers above ---------------------------------------------------------------------------------------------------------------------
def test_host_library_and_cli_give_the_bytes_of_the_c_calls(srt, oracle, frame1, tmp_path):
    fr, pt = frame1, frame1.pt
    grid = PG.Grid((-4.0, -1.0, 1.0), (2.0, 1.5, 2.0), (5, 3, 5))
    positions = srt.probe_grid_positions(grid.origin, grid.spacing, grid.counts)
    pt.trace_light_probes(positions, 64, samples=3, bounces=2, seed=13)
    coeff = pt.light_probe_coefficients()
    pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
    flags = PG.VISIBILITY | PG.NORMAL_WEIGHT | PG.ALBEDO
    pt.shade_probe_grid(coefficients=coeff, band_weight=PG.HEMISPHERE, count_work=True, **kwargs(flags))
    want, work = pt.probe_grid_output(), pt.probe_grid_work()
    assert 0 < work["open"] < work["segments"]
    pt.shade_probe_grid()
    plain = pt.probe_grid_output()
    # host.py over PathTraceRenderer::shadeProbeGrid: it renders the guides itself
    r = srt.host.Renderer(W, H)
    try:
        r.set_scene(srt.host.Scene(scene_path("Scene1")))
        r.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        assert same(r.shade_probe_grid(coeff, band_weight=PG.HEMISPHERE, count_work=True, **kwargs(flags)), want)
        assert r.probe_grid_work() == work
        assert same(r.shade_probe_grid(rows=(0, H)), plain) and same(r.probe_grid_output(), plain)
    finally:
        r.close()
    # the command-line tool: G-buffer, probes, shading; W * H float4, scene rows
    base = [CLI, "--scene", scene_path("Scene1"), "--width", str(W), "--height", str(H), "--probe-grid", "-4,-1,1,2,1.5,2,5,3,5", "--probe-directions", "64",
            "--radiance", "3", "--bounces", "2", "--seed", "13"]
    for extra, image in ((["--probe-visibility", "--probe-normal-weight", "--probe-albedo", "--probe-hemisphere"], want), ([], plain)):
        out = tmp_path / "irradiance.f32"
        run = subprocess.run(base + extra + ["--irradiance-out", str(out)], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr[-2000:]
        assert out.read_bytes() == image.tobytes(), extra
