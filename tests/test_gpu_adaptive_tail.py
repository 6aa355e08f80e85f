"""srt_render_adaptive_tail (ABI 7) on the MI355X: adaptive renders whose paths end in the probe grid.  Every comparison is bit for
bit (NaN compares as its bits) with no pixel left out.  The feature is pinned by its equivalence rule R3: pixel p after n_p samples
holds element p of srt_trace_radiance under the same srt_probe_tail setting on the frame's camera rays (ray x + y * W, id_base 0,
first_sample 1, n_p samples, RESET), and the framebuffer pixel is its tone_map at memory row H - 1 - y.  One radiance run per distinct
count of a map, shared by the pixels of that count.  24 x 20 makes nine 8 x 8 tiles, the bottom row of tiles four rows high.  The
grid inputs are tests/test_gpu_probe_tail.py's (5 x 4 x 5, R = 4, buried planes); one case is checked against the numpy loops of
tests/probe_tail_reference.py, which no device code has touched."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import probe_tail_reference as PT
from conftest import ROOT, scene_path
from test_gpu_adaptive import SENT_ACC, SENT_FB, Bound, sentinels
from test_gpu_denoise import _ppm_rgb, tone_map
from test_gpu_probe_tail import CO, COUNTS, GRID, MO, R, REC, SCENES, SEEDS, expected, fp, room_camera, set_grid, tail
from test_gpu_radiance import Scene, camera_rays, same, srt_camera

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 24, 20
ALL = PT.DEPTH | PT.STATES | PT.NORMAL_WEIGHT
FLAG_SETS = {"none": 0, "depth": PT.DEPTH, "states": PT.STATES, "all": ALL}
BUDGETS = np.array([0, 1, 3, 64, 65, 70], np.uint32)  # a pixel left alone, and both sides of the chunk of 64 samples
TAIL_KEYS = COUNTS + ("wave_lookups",)


def mixed_map(w=W, h=H):
    """The six budgets dealt over the pixels by a fixed pattern: every tile holds all of them."""
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    return BUDGETS[(x * 5 + y * 7 + (x // 3)) % 6]


class Frame(Scene):
    """A tracer with a scene, its camera set, the camera rays of the frame, and accumulator and framebuffer bound to torch tensors."""

    def __init__(self, srt, oracle, name, w=W, h=H):
        super().__init__(srt, oracle, SCENES[name](oracle), w, h)
        self.name = name
        self.ocam = room_camera(oracle) if name == "room" else oracle.default_camera()
        self.pt.set_camera(srt_camera(srt, self.ocam))
        self.rays = camera_rays(oracle, self.ocam, w, h)
        self.bound = Bound(self.pt, w, h)

    def start(self, counts, budget, sentinel=True):
        full = lambda v: np.ascontiguousarray(np.broadcast_to(np.uint32(v), (self.h, self.w))) if np.isscalar(v) else v
        self.pt.write_sample_counts(full(counts))
        self.pt.write_sample_budget(full(budget))
        if sentinel:
            self.bound.sentinel()

    def radiance(self, n, bounces, seed):
        """srt_trace_radiance under the mode as it stands on the frame's camera rays: (h, w, 4)."""
        self.pt.trace_radiance(self.rays[0], self.rays[1], samples=int(n), bounces=bounces, seed=seed, count_work=True)
        return self.pt.radiance().reshape(self.h, self.w, 4)

    def want(self, counts, bounces, seed, fb0=None, acc0=None):
        """(framebuffer, accumulator) of rule R3: per pixel the radiance run of its count; where `counts` is 0, (fb0, acc0)."""
        fb, acc = sentinels(self.w, self.h)
        fb, acc = (fb0 if fb0 is not None else fb).copy(), (acc0 if acc0 is not None else acc).copy()
        for n in np.unique(counts):
            if n == 0:
                continue
            rad = self.radiance(n, bounces, seed)
            m = counts == n  # scene rows; the framebuffer's memory row is H - 1 - y
            acc[m] = rad[m]
            fb[m[::-1]] = tone_map(rad)[::-1][m[::-1]]
        return fb, acc


def check(got, want, what):
    (gfb, gacc), (wfb, wacc) = got, want
    d = (gacc.view(np.uint32) != wacc.view(np.uint32)).any(axis=-1)
    assert not d.any(), "%s: %d accumulator elements differ" % (what, int(d.sum()))
    assert np.array_equal(gfb, wfb), "%s: %d framebuffer pixels differ" % (what, int((gfb != wfb).sum()))


@pytest.fixture(scope="module")
def frames(srt, oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Frame(srt, oracle, name)
            set_grid(made[name].pt, GRID, CO, MO, REC)
        return made[name]

    yield get
    for s in made.values():
        s.close()


# ---- 1. R3 on a mixed map -----------------------------------------------------------------------------------------------------------
CASES = [(n, b, "all") for n in SCENES for b in (1, 2, 8)] + [("room", 1, f) for f in ("none", "depth", "states")]


@pytest.mark.parametrize("name,bounces,flag_set", CASES)
def test_every_pixel_holds_the_radiance_trace_of_its_own_count(frames, name, bounces, flag_set):
    s = frames(name)
    seed = SEEDS.get((name, bounces), 3 + bounces)
    b = mixed_map()
    assert set(np.unique(b)) == set(BUDGETS)
    try:
        tail(s.pt, FLAG_SETS[flag_set])
        s.start(0, b)
        s.pt.render_adaptive_tail(bounces=bounces, seed=seed)
        got = s.bound.read()
        assert np.array_equal(s.pt.sample_counts(), b)
        tw = s.pt.probe_tail_work()
        check(got, s.want(b, bounces, seed), "%s B=%d %s" % (name, bounces, flag_set))
        assert tw["valid"] == 1 and tw["tails"] > 0  # (the mode did something in every scene)
    finally:
        tail(s.pt, 0, on=False)


# ---- 2. independent of device code --------------------------------------------------------------------------------------------------
def test_a_uniform_budget_in_the_room_gives_the_bits_of_the_numpy_loops(frames, oracle):
    s = frames("room")
    ref = PT.Scene(oracle, s.oarr, s.n, env=s.env)
    colours, terminals = PT.trace(ref, s.rays[0], s.rays[1], 3, 1, seed=4)
    assert all(t is not None for t in terminals)  # the closed room: every sample ends in a lookup or a mirror end
    want, work = expected(colours, terminals, GRID, CO, ALL)
    try:
        tail(s.pt, ALL)
        s.start(0, 3)
        s.pt.render_adaptive_tail(bounces=1, seed=4)
        fb, acc = s.bound.read()
        tw = s.pt.probe_tail_work()
        assert same(acc.reshape(-1, 4), want), "%d pixels differ from the reference loops" % int(
            (acc.reshape(-1, 4).view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum())
        assert np.array_equal(fb, tone_map(want.reshape(H, W, 4))[::-1])
        assert {k: tw[k] for k in COUNTS} == work and work["tails"] > 0
    finally:
        tail(s.pt, 0, on=False)


# ---- 3. work records ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bounces", [("scene1", 2), ("room", 1), ("mesh", 8)])
def test_the_two_work_records(frames, name, bounces):
    s = frames(name)
    seed = SEEDS.get((name, bounces), 3 + bounces)
    try:
        tail(s.pt, ALL)
        runs = []
        for _ in range(2):
            s.start(0, 3)
            s.pt.render_adaptive_tail(bounces=bounces, seed=seed, count_work=True)
            runs.append((s.bound.read(), s.pt.probe_tail_work(), s.pt.adaptive_work()))
        check(runs[1][0], runs[0][0], "the call repeated")
        assert runs[0][1] == runs[1][1] and runs[0][2] == runs[1][2]  # (the six tail counts, wave_lookups included)
        tw, aw = runs[0][1], runs[0][2]
        assert 1 <= tw["wave_lookups"] <= tw["tails"] + tw["mirror_ends"]
        # the five counts of srt_trace_radiance under the mode with 3 samples on the same rays
        s.radiance(3, bounces, seed)
        rw = s.pt.probe_tail_work()
        assert {k: tw[k] for k in COUNTS} == {k: rw[k] for k in COUNTS} and tw["tails"] > 0
        # srt_adaptive_work: a lookup traces no ray
        s.start(0, 3)
        s.pt.render_adaptive(bounces=bounces, seed=seed, count_work=True)
        assert s.pt.adaptive_work() == aw and aw["samples"] == 3 * W * H and aw["pixels"] == W * H
        # without SRT_ADAPTIVE_COUNT_WORK the adaptive record is refused and the tail's is still this call's
        s.start(0, 3)
        s.pt.render_adaptive_tail(bounces=bounces, seed=seed)
        assert s.pt.probe_tail_work() == tw
        assert s.pt.L.srt_get_adaptive_work(s.pt._h, C.byref(s.srt.capi.AdaptiveWork())) == s.srt.capi.ERR_STATE
    finally:
        tail(s.pt, 0, on=False)


# ---- 4. R4: zero coefficients -------------------------------------------------------------------------------------------------------
def test_zero_coefficients_give_the_buffers_and_the_work_of_srt_render_adaptive(frames):
    s = frames("scene1")
    b = mixed_map()
    s.start(0, b)
    s.pt.render_adaptive(bounces=2, seed=5, count_work=True)
    plain, plain_counts, plain_work = s.bound.read(), s.pt.sample_counts(), s.pt.adaptive_work()
    set_grid(s.pt, GRID, np.zeros_like(CO), MO, REC)
    try:
        tail(s.pt, ALL)
        s.start(0, b)
        s.pt.render_adaptive_tail(bounces=2, seed=5, count_work=True)
        check(s.bound.read(), plain, "zero coefficients")
        assert np.array_equal(s.pt.sample_counts(), plain_counts) and s.pt.adaptive_work() == plain_work
        assert s.pt.probe_tail_work()["tails"] > 0
        # ... and the coefficients matter
        set_grid(s.pt, GRID, CO, MO, REC)
        s.start(0, b)
        s.pt.render_adaptive_tail(bounces=2, seed=5)
        assert not np.array_equal(s.bound.read()[1].view(np.uint32), plain[1].view(np.uint32))
    finally:
        tail(s.pt, 0, on=False)
        set_grid(s.pt, GRID, CO, MO, REC)


# ---- 5. continuation ----------------------------------------------------------------------------------------------------------------
def test_two_calls_equal_one_call_with_the_sum_and_keep_counts_only_reads(frames):
    s = frames("room")
    try:
        tail(s.pt, PT.STATES)
        s.start(0, 5)
        s.pt.render_adaptive_tail(bounces=2, seed=5)
        whole = s.bound.read()
        s.start(0, 2)
        s.pt.render_adaptive_tail(bounces=2, seed=5)
        first = s.bound.read()
        assert (s.pt.sample_counts() == 2).all()
        s.start(s.pt.sample_counts(), 3, sentinel=False)
        s.pt.render_adaptive_tail(bounces=2, seed=5)
        check(s.bound.read(), whole, "2 then 3")
        assert (s.pt.sample_counts() == 5).all()
        assert not np.array_equal(first[1].view(np.uint32), whole[1].view(np.uint32))
        check(whole, s.want(np.full((H, W), 5), 2, 5), "5 at once")
        # KEEP_COUNTS: the same samples, the counts buffer unchanged
        s.start(0, 5)
        s.pt.render_adaptive_tail(bounces=2, seed=5, keep_counts=True)
        check(s.bound.read(), whole, "KEEP_COUNTS")
        assert (s.pt.sample_counts() == 0).all()
    finally:
        tail(s.pt, 0, on=False)


# ---- 6. untouched pixels ------------------------------------------------------------------------------------------------------------
def test_only_the_pixels_with_a_budget_change(frames):
    s = frames("scene1")
    b = np.zeros((H, W), np.uint32)
    b[6:9, 7:10] = 4  # a 3 x 3 block across two tile rows and two tile columns
    n0 = np.where(b > 0, 0, 0xDEAD).astype(np.uint32)
    try:
        tail(s.pt, ALL)
        s.start(n0, b)
        s.pt.render_adaptive_tail(bounces=2, seed=7, count_work=True)
        got = s.bound.read()
        check(got, s.want(b, 2, 7), "the 3 x 3 block")
        changed = (got[1].view(np.uint32) != SENT_ACC).any(axis=-1)
        assert np.array_equal(changed, b > 0) and int((got[0] != SENT_FB).sum()) == 9
        assert np.array_equal(s.pt.sample_counts(), np.where(b > 0, 4, 0xDEAD))
        assert s.pt.adaptive_work()["pixels"] == 9
        # an all-zero map: nothing changes, and the tail's record is valid and all zeros
        s.start(n0, 0)
        s.pt.render_adaptive_tail(bounces=2, seed=7, count_work=True)
        check(s.bound.read(), sentinels(), "an all-zero map")
        assert np.array_equal(s.pt.sample_counts(), n0)
        tw = s.pt.probe_tail_work()
        assert tw["valid"] == 1 and all(tw[k] == 0 for k in TAIL_KEYS)
        assert s.pt.adaptive_work()["wave_calls"] == 0
    finally:
        tail(s.pt, 0, on=False)


# ---- 7. partial tiles and a band ----------------------------------------------------------------------------------------------------
def test_partial_tiles_and_a_band_of_rows(srt, oracle):
    w, h = 27, 19
    s = Frame(srt, oracle, "scene1", w, h)
    try:
        set_grid(s.pt, GRID, CO, MO, REC)
        tail(s.pt, ALL)
        rows = (5, 14)  # memory rows: scene rows [h - 14, h - 5), nine of them
        inside = np.zeros((h, w), bool)
        inside[h - rows[1]:h - rows[0]] = True
        b = mixed_map(w, h)
        s.start(0, b)
        s.pt.render_adaptive_tail(bounces=2, seed=3, rows=rows)
        counts = np.where(inside, b, 0)
        check(s.bound.read(), s.want(counts, 2, 3), "27 x 19, rows [5, 14)")
        assert np.array_equal(s.pt.sample_counts(), counts)
        # ... and the whole frame: partial tile columns and rows
        s.start(0, b)
        s.pt.render_adaptive_tail(bounces=2, seed=3)
        check(s.bound.read(), s.want(b, 2, 3), "27 x 19")
    finally:
        s.close()


# ---- 8. one pixel alone -------------------------------------------------------------------------------------------------------------
def test_one_pixel_of_200_samples_fills_the_wave_and_crosses_three_chunks(frames):
    s = frames("room")
    x, y = 12, 10
    pix = x + y * W
    b = np.zeros((H, W), np.uint32)
    b[y, x] = 200
    try:
        tail(s.pt, ALL)
        s.start(0, b)
        s.pt.render_adaptive_tail(bounces=2, seed=9, count_work=True)
        (fb, acc), tw, aw = s.bound.read(), s.pt.probe_tail_work(), s.pt.adaptive_work()
        o, d = s.rays
        s.pt.trace_radiance(o[pix:pix + 1], d[pix:pix + 1], samples=200, bounces=2, seed=9, id_base=pix, count_work=True)
        want, rw = s.pt.radiance(), s.pt.probe_tail_work()
        assert same(acc[y, x][None, :], want)
        assert fb[H - 1 - y, x] == tone_map(want)[0]
        assert tw["tails"] + tw["mirror_ends"] == rw["tails"] + rw["mirror_ends"] == 200  # the closed room: every path ends at the limit
        assert {k: tw[k] for k in COUNTS} == {k: rw[k] for k in COUNTS}
        assert aw["samples"] == 200 and aw["pixels"] == 1 and aw["wave_calls"] <= 1 + 4 * 2
        acc[y, x], fb[H - 1 - y, x] = sentinels()[1][y, x], SENT_FB
        check((fb, acc), sentinels(), "the other pixels")
    finally:
        tail(s.pt, 0, on=False)


# ---- 9. 64 tiles dealt by the ticket ------------------------------------------------------------------------------------------------
def test_64_tiles_repeat_bit_for_bit(srt, oracle):
    s = Frame(srt, oracle, "scene1", 64, 64)
    try:
        set_grid(s.pt, GRID, CO, MO, REC)
        tail(s.pt, ALL)
        runs = []
        for _ in range(2):
            s.start(0, 2)
            s.pt.render_adaptive_tail(bounces=2, seed=6, count_work=True)
            runs.append((s.bound.read(), s.pt.probe_tail_work()))
            assert (s.pt.sample_counts() == 2).all()
        check(runs[1][0], runs[0][0], "the call repeated")
        assert runs[0][1] == runs[1][1] and runs[0][1]["tails"] > 0
        check(runs[0][0], s.want(np.full((64, 64), 2), 2, 6), "64 x 64")
    finally:
        s.close()


# ---- 10. R1 and R2, in order --------------------------------------------------------------------------------------------------------
def test_the_order_of_refusals_and_zero_bounces(srt, oracle):
    import torch

    c = srt.capi
    s = Frame(srt, oracle, "scene1")
    pt = s.pt
    try:
        def call(bounces=2, flags=0, reserved=0, rows=(0, H), max_samples=4096):
            p = c.AdaptiveParams()
            pt.L.srt_adaptive_params_default(C.byref(p))
            p.row_begin, p.row_end, p.max_bounces, p.seed, p.max_samples, p.flags, p.reserved = rows[0], rows[1], bounces, 3, max_samples, flags, reserved
            return pt.L.srt_render_adaptive_tail(pt._h, C.byref(p))

        def untouched():
            check(s.bound.read(), sentinels(), "a refused call")
            return (pt.sample_counts() == 0).all()

        def plain(bounces):
            s.start(0, 3)
            pt.render_adaptive(bounces=bounces, seed=3, count_work=True)
            return s.bound.read(), pt.adaptive_work()

        off2, off0 = plain(2), plain(0)
        s.start(0, 3)
        # the call's own argument errors come before the mode check (the mode is off, and has never been on)
        assert call(flags=4) == c.ERR_INVALID_ARG and call(reserved=1) == c.ERR_INVALID_ARG and call(rows=(0, H + 1)) == c.ERR_INVALID_ARG
        assert call(max_samples=0) == c.ERR_INVALID_ARG and call(bounces=-1) == c.ERR_INVALID_ARG
        # the mode off: SRT_ERR_STATE, at any bounce count
        assert call() == c.ERR_STATE and call(0) == c.ERR_STATE
        tail(pt, 0)
        tail(pt, 0, on=False)
        assert call() == c.ERR_STATE and call(0) == c.ERR_STATE and untouched()
        # the mode on, and the sequence of the probe-tail block: nothing of the grid is there yet
        tail(pt, PT.DEPTH | PT.STATES)
        assert call(flags=4) == c.ERR_INVALID_ARG  # (still first)
        assert call() == c.ERR_STATE               # no grid
        pt.set_probe_grid(GRID.origin, GRID.spacing, GRID.counts)
        assert call() == c.ERR_STATE               # no coefficients
        pt._ck(pt.L.srt_write_probe_grid_coefficients(pt._h, fp(CO), GRID.probes - 1))
        assert call() == c.ERR_STATE               # a count that is not nx*ny*nz
        pt._ck(pt.L.srt_write_probe_grid_coefficients(pt._h, fp(CO), GRID.probes))
        assert call() == c.ERR_STATE               # DEPTH without maps
        pt._ck(pt.L.srt_write_probe_grid_depth(pt._h, fp(MO), GRID.probes - 1, R))
        assert call() == c.ERR_STATE
        pt._ck(pt.L.srt_write_probe_grid_depth(pt._h, fp(MO), GRID.probes, R))
        assert call() == c.ERR_STATE               # STATES without records
        pt._ck(pt.L.srt_write_probe_grid_states(pt._h, fp(REC), GRID.probes - 1))
        assert call() == c.ERR_STATE and untouched()
        pt._ck(pt.L.srt_write_probe_grid_states(pt._h, fp(REC), GRID.probes))
        assert call() == c.OK                      # everything the flags ask for is there
        on2 = s.bound.read()
        assert not np.array_equal(on2[1].view(np.uint32), off2[0][1].view(np.uint32)) and (pt.sample_counts() == 3).all()
        # the coefficient array as the accumulator, then as the framebuffer: refused, and the tensor keeps its fill
        t = torch.full((GRID.probes * 9, 4), 0.25, dtype=torch.float32, device="cuda:%d" % pt.device)
        assert GRID.probes * 9 >= W * H
        pt._ck(pt.L.srt_bind_probe_grid_coefficients(pt._h, C.c_void_p(t.data_ptr()), GRID.probes))
        s.start(0, 3)
        pt.bind_output(s.bound.fb.data_ptr(), t.data_ptr())
        assert call() == c.ERR_STATE
        pt.bind_output(t.data_ptr() + 4096, s.bound.acc.data_ptr())  # (the framebuffer inside the array)
        assert call() == c.ERR_STATE
        pt.wait()
        assert bool((t == 0.25).all()) and (pt.sample_counts() == 0).all()
        s.bound.bind()
        assert untouched()
        assert call() == c.OK  # (bound coefficients that overlap nothing)
        pt._ck(pt.L.srt_bind_probe_grid_coefficients(pt._h, None, 0))
    finally:
        s.close()
    # max_bounces == 0 with no grid at all: SRT_OK, the bits of srt_render_adaptive, the tail's record valid and zero
    s = Frame(srt, oracle, "scene1")
    pt = s.pt
    try:
        tail(pt, ALL)
        s.start(0, 3)
        pt.render_adaptive_tail(bounces=0, seed=3, count_work=True)
        check(s.bound.read(), off0[0], "max_bounces == 0")
        assert pt.adaptive_work() == off0[1]
        tw = pt.probe_tail_work()
        assert tw["valid"] == 1 and all(tw[k] == 0 for k in TAIL_KEYS)
        with pytest.raises(srt.capi.SrtError) as e:
            pt.render_adaptive_tail(bounces=1, seed=3)
        assert e.value.code == c.ERR_STATE
        # after all of it srt_render_adaptive still gives its own bits with the mode on
        s.start(0, 3)
        pt.render_adaptive(bounces=2, seed=3, count_work=True)
        check(s.bound.read(), off2[0], "srt_render_adaptive with the mode on")
        assert pt.adaptive_work() == off2[1]
    finally:
        s.close()


# ---- 11. host layers and the command line -------------------------------------------------------------------------------------------
def test_the_host_renderer_and_the_cli_give_the_bytes_of_the_python_route(srt, tmp_path):
    import probe_grid_reference as PG

    w, h, K, rounds, spp = 24, 20, 64, 2, 4
    grid = PG.Grid((-2.5, -1.0, 0.5), (1.25, 0.8, 1.5), (5, 4, 5))
    pt = srt.PathTracer(w, h)
    try:
        objs, cnt = srt.host.Scene(scene_path("Scene_indirect")).objects_copy()
        pt.set_scene(objs, cnt)
        pt.set_camera(srt.default_camera())
        pos = srt.probe_grid_positions(grid.origin, grid.spacing, grid.counts)
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        pt.reset_probe_history(grid.probes, which="coefficients")
        for f in range(1, rounds + 1):  # the feedback rounds of srt_render --probe-grid --probe-feedback
            if f > 1:
                pt._ck(pt.L.srt_write_probe_grid_coefficients(pt._h, fp(pt.probe_history("coefficients")), grid.probes))
            pt.probe_tail(enabled=f > 1, count_work=True)
            pt.trace_light_probes(pos, K, samples=16, bounces=1, seed=f)
            pt.blend_probes()
        history = pt.probe_history("coefficients")
        pt._ck(pt.L.srt_write_probe_grid_coefficients(pt._h, fp(history), grid.probes))
        pt.probe_tail(enabled=True, count_work=True)
        pt.set_sample_counts(0)
        pt.write_sample_budget(np.full((h, w), spp, np.uint32))
        pt.render_adaptive_tail(bounces=1, seed=0)
        want = pt.framebuffer()
        assert pt.probe_tail_work()["tails"] > 0
        pt.probe_tail(enabled=False)
        pt.set_sample_counts(0)
        pt.render_adaptive(bounces=1, seed=0)
        assert not np.array_equal(pt.framebuffer(), want)  # (the tail adds light)
    finally:
        pt.close()
    # PathTraceRenderer::renderProbeTailFrame through host.py
    sc = srt.host.Scene(scene_path("Scene_indirect"))
    r = srt.host.Renderer(w, h)
    try:
        r.set_scene(sc)
        r.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        L = srt.load_library()
        assert L.srt_write_probe_grid_coefficients(r.handle(), fp(history), grid.probes) == 0
        r.probe_tail(enabled=True)
        r.render_probe_tail_frame(spp, bounces=1, seed=0)
        assert np.array_equal(r.framebuffer(), want)
        assert (r.sample_counts() == spp).all()
    finally:
        r.close()
        sc.close()
    # srt_render ... --probe-tail --probe-tail-frame
    cli = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
    out, img = tmp_path / "f.ppm", tmp_path / "irradiance.f32"
    run = subprocess.run([cli, "--scene", scene_path("Scene_indirect"), "--width", str(w), "--height", str(h), "--probe-grid", "-2.5,-1,0.5,1.25,0.8,1.5,5,4,5",
                          "--probe-directions", str(K), "--probe-feedback", str(rounds), "--probe-tail", "--probe-tail-frame", "--spp", str(spp), "--bounces", "1",
                          "--out", str(out), "--irradiance-out", str(img)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "probe tail frame" in run.stderr and img.exists()  # (everything the flow writes it still writes)
    rgb = np.stack([(want >> 16) & 0xFF, (want >> 8) & 0xFF, want & 0xFF], axis=-1).astype(np.uint8)
    assert np.array_equal(_ppm_rgb(out, w, h), rgb)


# ---- 12. quality --------------------------------------------------------------------------------------------------------------------
MEASURED_RATIO = {"B1_tail": 1.51, "B1_tail_depth_states": 1.65}  # rmse(without) / rmse(with), one measured run (see the docstring)


def test_the_tail_lowers_the_error_of_a_one_bounce_frame_in_scene_indirect(srt):
    """tools/probe_tail_frame_quality.py's protocol at 96 x 54 in Scene_indirect, grid spacing 0.5, coefficients from probes traced
    at B = 8: the relative luminance RMSE over the diffuse pixels of a B = 1, 64-sample frame of srt_render_adaptive against a
    4096-sample B = 8 srt_render, and of srt_render_adaptive_tail's frame with and without DEPTH | STATES.  The measured ratios
    rmse(without) / rmse(with) are in MEASURED_RATIO and in profiles/probe_tail_frame/probe_tail_frame_quality.jsonl; the test
    asserts half of each (noise and the SH approximation get a factor of two), and nothing for a ratio that was measured below
    1.5.  One run: 42 diffuse pixels, rmse 0.0795 without, 0.0528 with the tail (ratio 1.51), 0.0483 with DEPTH | STATES (ratio
    1.65): by rule R3 the figures of the camera-ray route (tests/test_gpu_probe_tail.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import probe_tail_frame_quality as Q

    pt, rmse, info = Q.frame_setup(srt, "Scene_indirect", 96, 54, 4096, 0.5)
    try:
        assert info["diffuse_pixels"] >= 40, info  # (42 were measured at this size)
        without = rmse(64, 1, None)
        for key, tail_flags in (("B1_tail", {}), ("B1_tail_depth_states", {"depth": True, "states": True})):
            with_tail = rmse(64, 1, tail_flags)
            ratio = without / with_tail
            print("Scene_indirect 96x54 B=1 n=64 %s: rmse without %.4f, with %.4f, ratio %.2f (%s)" % (key, without, with_tail, ratio, info))
            measured = MEASURED_RATIO[key]
            if measured is not None and measured >= 1.5:
                assert ratio >= measured / 2
    finally:
        pt.close()
