"""SRT_ADAPTIVE_SUN_SAMPLING (= 16; rules AS1 - AS8 of srt_pathtrace.h) on the MI355X: sun sampling in srt_render_adaptive and, together
with the probe tail, in srt_render_adaptive_tail.  Comparisons are bit for bit in all four lanes (NaN compares as its bits) with no
pixel left out, except the unbiasedness test, whose bound is derived from the estimator's own variance, and the error test.

Without the tail the feature is pinned by AS2: a pixel holds what srt_trace_radiance with SRT_RADIANCE_SUN_SAMPLING gives on its
camera ray at its own count (one radiance run per distinct count).  The combination with the tail has no radiance counterpart
(the traces refuse the flag under the mode): its reference is the numpy loop of tests/adaptive_sun_reference.py, pinned on the CPU
by tests/test_adaptive_sun_reference.py.  24 x 20 makes nine 8 x 8 tiles, partial in both axes; the budget map is
tests/test_gpu_adaptive_tail.py's, scenes, seeds and grid inputs are tests/test_gpu_probe_tail.py's.  Every test here fails on
the parent commit, which refuses the flag."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import adaptive_sun_reference as AS
import probe_tail_reference as PT
import sun_sampling_reference as SS
from conftest import ROOT, scene_path
from test_gpu_adaptive import SENT_ACC, SENT_FB, sentinels
from test_gpu_adaptive_tail import ALL, BUDGETS, Frame, check, mixed_map
from test_gpu_denoise import tone_map
from test_gpu_probe_tail import CO, COUNTS, GRID, MO, R, REC, SCENES, SEEDS, fp, set_grid, tail
from test_gpu_radiance import camera_rays, same, srt_camera
from test_gpu_sun_sampling import custom, floor

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 24, 20
SAMPLES = 3  # wherever numpy runs the loop
BAD_DIRECTIONS = ((0.0, -2.0, 0.0), (0.0, 0.0, 0.0), (float("nan"), -1.0, 0.0), (float("inf"), 0.0, 0.0))
_paths = {}


@pytest.fixture(scope="module")
def frames(srt, oracle):
    made = {}

    def get(name):
        if name not in made:
            s = made[name] = Frame(srt, oracle, name)
            set_grid(s.pt, GRID, CO, MO, REC)
            s.ref = SS.SunScene(PT.Scene(oracle, s.oarr, s.n, om=s.om[:2] if s.om else None, env=s.env))
        return made[name]

    yield get
    for s in made.values():
        s.close()


def radiance(s, n, bounces, seed, sun=True, first=1, reset=True):
    """srt_trace_radiance on the frame's camera rays: (h, w, 4).  reset=False continues what the last call left."""
    if reset:
        s.pt.trace_radiance(s.rays[0], s.rays[1], samples=int(n), bounces=bounces, seed=seed, first_sample=first, sun_sampling=sun)
    else:
        s.pt.trace_radiance(samples=int(n), bounces=bounces, seed=seed, first_sample=first, reset=False, sun_sampling=sun)
    return s.pt.radiance().reshape(s.h, s.w, 4)


def want_from(rad_of_count, counts, w=W, h=H):
    """(framebuffer, accumulator): per pixel rad_of_count(n) of its count n; where `counts` is 0, the sentinels."""
    fb, acc = sentinels(w, h)
    for n in np.unique(counts):
        if n == 0:
            continue
        rad = rad_of_count(int(n))
        m = counts == n  # scene rows; the framebuffer's memory row is H - 1 - y
        acc[m] = rad[m]
        fb[m[::-1]] = tone_map(rad)[::-1][m[::-1]]
    return fb, acc


def paths(s, name, bounces, seed, samples=SAMPLES):
    key = (name, bounces, seed, samples)
    if key not in _paths:
        _paths[key] = AS.trace(s.ref, s.rays[0], s.rays[1], samples, bounces, seed=seed)
    return _paths[key]


def reference(s, name, bounces, seed, flags, co=CO):
    """The accumulator (h, w, 4) of srt_render_adaptive_tail with the flag after a uniform 3 from n = 0, and the tail's five counts."""
    colours, terminals, segments, opened = paths(s, name, bounces, seed)
    add, adds, work = PT.tails(terminals, GRID, co, flags=flags, depth=MO, R=R, records=REC)
    return PT.radiance(colours, add=(add, adds)).reshape(s.h, s.w, 4), work, segments, opened


# ---- 1. AS2: a pixel is the radiance trace of its own count -----------------------------------------------------------------------
@pytest.mark.parametrize("bounces", [1, 2, 8])
@pytest.mark.parametrize("name", list(SCENES))
def test_every_pixel_holds_the_flagged_radiance_trace_of_its_own_count(frames, name, bounces):
    s = frames(name)
    seed = SEEDS.get((name, bounces), 3 + bounces)
    b = mixed_map()
    assert set(np.unique(b)) == set(BUDGETS)
    s.start(0, b)
    s.pt.render_adaptive(bounces=bounces, seed=seed, sun_sampling=True)
    got = s.bound.read()
    assert np.array_equal(s.pt.sample_counts(), b)  # the counts are written
    check(got, want_from(lambda n: radiance(s, n, bounces, seed), b), "%s B=%d" % (name, bounces))
    zero = b == 0  # the budget-0 pixels keep their sentinel bytes
    assert (got[1].view(np.uint32)[zero] == SENT_ACC).all() and (got[0][zero[::-1]] == SENT_FB).all()
    if name == "scene1":  # (the flag does something in a sunlit scene)
        s.start(0, b)
        s.pt.render_adaptive(bounces=bounces, seed=seed)
        assert not np.array_equal(s.bound.read()[1].view(np.uint32), got[1].view(np.uint32))


# ---- 2. AS3: continuation and mixing ----------------------------------------------------------------------------------------------
def test_flagged_and_unflagged_samples_share_one_mean_in_frame_order(frames):
    s = frames("scene1")
    pt = s.pt
    s.bound.sentinel()
    pt.render(spp=5, bounces=2, seed=5)  # frames 1..5 without the flag
    pt.set_sample_counts(5)
    pt.write_sample_budget(np.full((H, W), 3, np.uint32))
    pt.render_adaptive(bounces=2, seed=5, sun_sampling=True)  # 6..8 with it
    pt.write_sample_budget(np.full((H, W), 2, np.uint32))
    pt.render_adaptive(bounces=2, seed=5)  # 9..10 without
    got = s.bound.read()
    assert (pt.sample_counts() == 10).all()
    radiance(s, 5, 2, 5, sun=False)
    radiance(s, 3, 2, 5, sun=True, first=6, reset=False)
    rad = radiance(s, 2, 2, 5, sun=False, first=9, reset=False)
    check(got, (tone_map(rad)[::-1], rad), "5 plain + 3 flagged + 2 plain")
    plain = radiance(s, 10, 2, 5, sun=False)
    assert not same(plain, rad)  # (the three flagged frames matter)


def test_two_flagged_calls_equal_one_and_keep_counts_only_reads(frames):
    s = frames("scene1")
    pt = s.pt
    s.start(0, 70)
    pt.render_adaptive(bounces=2, seed=9, sun_sampling=True)
    whole = s.bound.read()
    s.start(0, 3)
    pt.render_adaptive(bounces=2, seed=9, sun_sampling=True)
    first = s.bound.read()
    assert (pt.sample_counts() == 3).all()
    s.start(pt.sample_counts(), 67, sentinel=False)
    pt.render_adaptive(bounces=2, seed=9, sun_sampling=True)
    check(s.bound.read(), whole, "3 then 67")
    assert (pt.sample_counts() == 70).all()
    assert not np.array_equal(first[1].view(np.uint32), whole[1].view(np.uint32))
    rad = radiance(s, 70, 2, 9)
    check(whole, (tone_map(rad)[::-1], rad), "70 at once")
    # KEEP_COUNTS: the same samples, the counts buffer unchanged
    s.start(0, 70)
    pt.render_adaptive(bounces=2, seed=9, sun_sampling=True, keep_counts=True)
    check(s.bound.read(), whole, "KEEP_COUNTS")
    assert (pt.sample_counts() == 0).all()


# ---- 3. AS4 against the numpy loop ------------------------------------------------------------------------------------------------
TAIL_CASES = [(n, b, ALL) for n in ("room", "scene1", "mesh") for b in (1, 2)] + [("room", 1, f) for f in (0, PT.NORMAL_WEIGHT, PT.DEPTH, PT.STATES)]


@pytest.mark.parametrize("name,bounces,flags", TAIL_CASES)
def test_the_combination_gives_the_bits_of_the_numpy_loop(frames, name, bounces, flags):
    s = frames(name)
    seed = SEEDS.get((name, bounces), 3 + bounces)
    want, work, segments, opened = reference(s, name, bounces, seed, flags)
    try:
        tail(s.pt, flags)
        s.start(0, SAMPLES)
        s.pt.render_adaptive_tail(bounces=bounces, seed=seed, sun_sampling=True, count_work=True)
        fb, acc = s.bound.read()
        tw, on = s.pt.probe_tail_work(), s.pt.adaptive_work()
        d = (acc.view(np.uint32) != want.view(np.uint32)).any(axis=-1)
        print("%s B=%d flags %d: %d pixels differ from the reference; %d segments, %d open, tail %s" % (name, bounces, flags, int(d.sum()), segments, opened, work))
        assert not d.any(), "%d of %d pixels differ from the reference loop" % (int(d.sum()), W * H)
        assert np.array_equal(fb, tone_map(want)[::-1])
        assert (s.pt.sample_counts() == SAMPLES).all()
        assert {k: tw[k] for k in COUNTS} == work and work["tails"] + work["mirror_ends"] > 0 and segments > 0
        # the flag against the same call without it: the tail's record and the path's counts are equal, wave_calls is not
        s.start(0, SAMPLES)
        s.pt.render_adaptive_tail(bounces=bounces, seed=seed, count_work=True)
        off_acc, off_tw, off = s.bound.read()[1], s.pt.probe_tail_work(), s.pt.adaptive_work()
        assert off_tw == tw
        assert (on["pixels"], on["samples"], on["closest_calls"]) == (off["pixels"], off["samples"], off["closest_calls"])
        assert off["wave_calls"] < on["wave_calls"] <= off["wave_calls"] + segments
        if name == "scene1":
            assert opened > 0 and not np.array_equal(off_acc.view(np.uint32), acc.view(np.uint32))
    finally:
        tail(s.pt, 0, on=False)


@pytest.mark.parametrize("name,bounces", [("scene1", 2), ("room", 1)])
def test_a_pixel_of_the_mixed_map_holds_the_bits_of_the_uniform_render_of_its_budget(frames, name, bounces):
    s = frames(name)
    seed = SEEDS.get((name, bounces), 3 + bounces)
    b = mixed_map()
    try:
        tail(s.pt, ALL)
        s.start(0, b)
        s.pt.render_adaptive_tail(bounces=bounces, seed=seed, sun_sampling=True)
        got = s.bound.read()
        assert np.array_equal(s.pt.sample_counts(), b)

        def uniform(n):
            s.start(0, n)
            s.pt.render_adaptive_tail(bounces=bounces, seed=seed, sun_sampling=True)
            return s.bound.read()[1]

        check(got, want_from(uniform, b), "%s B=%d: the tile packing does not enter the result" % (name, bounces))
        # ... and the uniform 3 is the numpy loop's (test above), so every count hangs on the reference
        want3 = reference(s, name, bounces, seed, ALL)[0]
        assert np.array_equal(got[1].view(np.uint32)[b == 3], want3.view(np.uint32)[b == 3])
    finally:
        tail(s.pt, 0, on=False)


# ---- 4. AS7: invariants -----------------------------------------------------------------------------------------------------------
def render_both(s, bounces, seed, sun, budget, with_tail):
    """(buffers, counts, adaptive work, tail work or None) of one call from n = 0."""
    s.start(0, budget)
    (s.pt.render_adaptive_tail if with_tail else s.pt.render_adaptive)(bounces=bounces, seed=seed, sun_sampling=sun, count_work=True)
    return s.bound.read(), s.pt.sample_counts(), s.pt.adaptive_work(), s.pt.probe_tail_work() if with_tail else None


def test_a_black_sun_gives_the_buffers_without_the_flag(srt, frames):
    s = frames("scene1")
    b = mixed_map()
    black = srt.default_environment()
    black.sun_color[:] = (0.0, 0.0, 0.0)
    try:
        s.pt.set_environment(black)
        for with_tail in (False, True):
            tail(s.pt, ALL, on=with_tail)
            off = render_both(s, 8, 2, False, b, with_tail)
            on = render_both(s, 8, 2, True, b, with_tail)
            check(on[0], off[0], "a black sun, tail %s" % with_tail)
            assert np.array_equal(on[1], off[1]) and on[2]["wave_calls"] > off[2]["wave_calls"]  # (segments are traced all the same: they add +0)
            assert on[3] == off[3]
    finally:
        s.pt.set_environment(srt.default_environment())
        tail(s.pt, 0, on=False)


def test_a_scene_without_a_diffuse_vertex_gives_the_buffers_and_the_work_without_the_flag(srt, oracle):
    from test_gpu_adaptive import Bound

    objs = [dict(type=oracle.OBJ_BOX, position=(0.0, -1.5, 5.0), half_size=(20.0, 0.5, 20.0), base=(0.7, 0.7, 0.7), smoothness=0.3, specular_amount=1.0),
            dict(type=oracle.OBJ_SPHERE, position=(0.0, 0.0, 5.0), radius=1.0, base=(0.9, 0.4, 0.2), smoothness=1.0, specular_amount=2.0, specular=(0.9, 0.9, 0.9))]
    m = custom(srt, oracle, objs, w=W, h=H)
    try:
        m.pt.set_camera(srt_camera(srt, oracle.default_camera()))
        m.bound = Bound(m.pt, W, H)
        m.start = Frame.start.__get__(m)
        set_grid(m.pt, GRID, CO, MO, REC)
        b = mixed_map()
        for with_tail in (False, True):
            tail(m.pt, ALL, on=with_tail)
            off = render_both(m, 8, 4, False, b, with_tail)
            on = render_both(m, 8, 4, True, b, with_tail)
            check(on[0], off[0], "all mirrors, tail %s" % with_tail)
            assert np.array_equal(on[1], off[1]) and on[3] == off[3]
            assert on[2] == off[2]  # no diffuse vertex: no any-hit call, the record is the same
            assert off[2]["closest_calls"] > off[2]["samples"]  # (paths do bounce there)
    finally:
        m.close()


def test_zero_coefficients_and_zero_bounces(frames):
    s = frames("scene1")
    b = mixed_map()
    flagged = render_both(s, 2, 5, True, b, False)
    set_grid(s.pt, GRID, np.zeros_like(CO), MO, REC)
    try:
        tail(s.pt, ALL)
        zero = render_both(s, 2, 5, True, b, True)
        check(zero[0], flagged[0], "R4 with the flag on both sides")
        assert np.array_equal(zero[1], flagged[1]) and zero[2] == flagged[2] and zero[3]["tails"] > 0
        # max_bounces == 0: the unflagged buffers and work, for both calls (AS6)
        for with_tail in (False, True):
            off = render_both(s, 0, 5, False, b, with_tail)
            on = render_both(s, 0, 5, True, b, with_tail)
            check(on[0], off[0], "max_bounces == 0, tail %s" % with_tail)
            assert np.array_equal(on[1], off[1]) and on[2] == off[2] and on[3] == off[3]
    finally:
        tail(s.pt, 0, on=False)
        set_grid(s.pt, GRID, CO, MO, REC)


# ---- 5. AS8: work -----------------------------------------------------------------------------------------------------------------
def test_one_pixel_of_sixty_four_samples_makes_one_any_hit_call(srt, oracle):
    s = custom(srt, oracle, [floor(oracle)])
    try:
        ocam = oracle.default_camera()
        s.pt.set_camera(srt_camera(srt, ocam))
        _, d = camera_rays(oracle, ocam, 8, 8)
        # the pixel that looks down most steeply among those whose direction has no component of exactly zero (the reference's box
        # test, a slab test, answers such a ray with a miss: the centre column never meets the floor)
        dy = np.where((d[:, :3] != 0).all(axis=1), d[:, 1], np.inf)
        pix = int(np.argmin(dy))
        assert dy[pix] < -0.2
        b = np.zeros(64, np.uint32)
        b[pix] = 64
        work = {}
        for sun in (False, True):
            s.pt.write_sample_counts(np.zeros((8, 8), np.uint32))
            s.pt.write_sample_budget(b.reshape(8, 8))
            s.pt.render_adaptive(bounces=1, seed=0, sun_sampling=sun, count_work=True)
            work[sun] = s.pt.adaptive_work()
        off, on = work[False], work[True]
        assert on["wave_calls"] == off["wave_calls"] + 1
        assert (on["closest_calls"], on["pixels"], on["samples"]) == (off["closest_calls"], off["pixels"], off["samples"]) == (128, 1, 64)
    finally:
        s.close()


def test_the_work_record_repeats_over_64_tiles_and_the_tails_record_ignores_the_flag(srt, oracle, frames):
    s = Frame(srt, oracle, "scene1", 64, 64)
    try:
        runs = []
        for _ in range(3):
            s.start(0, 2)
            s.pt.render_adaptive(bounces=2, seed=6, sun_sampling=True, count_work=True)
            runs.append((s.bound.read(), s.pt.adaptive_work()))
        for r in runs[1:]:
            check(r[0], runs[0][0], "the call repeated")
            assert r[1] == runs[0][1]
        s.start(0, 2)
        s.pt.render_adaptive(bounces=2, seed=6, count_work=True)
        off = s.pt.adaptive_work()
        on = runs[0][1]
        assert on["wave_calls"] > off["wave_calls"] and (on["closest_calls"], on["pixels"], on["samples"]) == (off["closest_calls"], off["pixels"], off["samples"])
    finally:
        s.close()
    room = frames("room")
    try:
        tail(room.pt, ALL)
        on = render_both(room, 1, 4, True, SAMPLES, True)
        off = render_both(room, 1, 4, False, SAMPLES, True)
        assert on[3] == off[3] and on[3]["valid"] == 1 and on[3]["tails"] > 0
    finally:
        tail(room.pt, 0, on=False)


# ---- 6. unbiasedness of the combination -------------------------------------------------------------------------------------------
def down_camera(oracle):
    """Above the floor, looking down at it next to the box, turned about two axes so that no ray direction has a component of
    exactly zero: right (0.8, 0, -0.6), up (0.48, 0.6, 0.64), forward (0.36, -0.8, 0.48), an orthonormal basis; the centre of the
    frame meets the floor at (0.2, -1, 5)."""
    cam = oracle.default_camera()
    cam.position[:] = (-1.6, 3.0, 2.6)
    cam.right[:] = (0.8, 0.0, -0.6)
    cam.up[:] = (0.48, 0.6, 0.64)
    cam.forward[:] = (0.36, -0.8, 0.48)
    return cam


@pytest.mark.parametrize("sun_direction", [(0.0, -1.0, 0.0), (-1.0, -1.0, -1.0)])
def test_the_flag_does_not_change_the_mean_of_a_tail_frame(srt, oracle, sun_direction):
    """The protocol of tests/test_gpu_sun_sampling.py's unbiasedness test with the tail on: a black sky with SunColor = (10, 10, 10)
    over a white diffuse floor with one white diffuse unit box standing on it at (1.2, -0.5, 5), constant DC-only coefficients, an
    8 x 8 frame from down_camera(), 1 bounce, a budget of 4096.  A: the tail alone, B: the tail with the flag, C: the tail with
    SunColor = (0, 0, 0).  The three share every path, so per sample A - C is 10 x [the blind bounce left through the cap] and
    B - C is the segment's add; with p = (mean B - mean C) / 10 the difference of the means of A and B has a standard deviation of
    at most 10 sqrt(p (1 - p) / (64 * 4096)) (the flag's own variance is smaller), and five of them are the bound.
    Chosen on the CPU with the numpy loop at 200 samples per pixel, before any device run: 59 primary rays meet the floor and 5
    the box, 925 of 12800 paths end in a lookup, 12488 of 12488 segments are open with the sun overhead, 11301 of 12200 with the
    diagonal sun, where pixels 29 and 38 have every segment occluded."""
    sd = np.array(sun_direction, np.float64)
    sd /= np.linalg.norm(sd)
    env = oracle.default_environment()
    env.sun_direction[:] = [float(F(v)) for v in sd]
    env.sky_color[:] = env.horizon_color[:] = env.ground_color[:] = (0.0, 0.0, 0.0)
    env.sun_color[:] = (10.0, 10.0, 10.0)
    box = dict(type=oracle.OBJ_BOX, position=(1.2, -0.5, 5.0), half_size=(0.5, 0.5, 0.5), base=(1.0, 1.0, 1.0), smoothness=0.0, specular_amount=0.0)
    s = custom(srt, oracle, [floor(oracle), box], env)
    co = np.zeros_like(CO)
    co[:, 0, :3] = F(0.5)
    try:
        pt = s.pt
        pt.set_camera(srt_camera(srt, down_camera(oracle)))
        set_grid(pt, GRID, co)
        tail(pt, 0)

        def frame(sun):
            pt.write_sample_counts(np.zeros((8, 8), np.uint32))
            pt.write_sample_budget(np.full((8, 8), 4096, np.uint32))
            pt.render_adaptive_tail(bounces=1, seed=21, sun_sampling=sun)
            return pt.accumulator().reshape(64, 4), pt.probe_tail_work()

        a, tw = frame(False)
        b, _ = frame(True)
        dark = srt.default_environment()
        for k in ("sun_direction", "sky_color", "horizon_color", "ground_color"):
            getattr(dark, k)[:] = getattr(env, k)[:]
        dark.sun_color[:] = (0.0, 0.0, 0.0)
        pt.set_environment(dark)
        c, _ = frame(False)
        mu_a, mu_b, mu_c = (float(np.mean(v[:, 0], dtype=np.float64)) for v in (a, b, c))
        p = (mu_b - mu_c) / 10.0
        bound = 5.0 * 10.0 * np.sqrt(p * (1.0 - p) / (64 * 4096))
        occluded = (b[:, :3].view(np.uint32) == c[:, :3].view(np.uint32)).all(axis=-1)  # B - C is the segments' add: zero only if every segment was occluded
        print("sun_direction %s: mean A %.5f, B %.5f, C %.5f, B - A %.5f, bound %.5f (%.1f %% of B - C); lookups %d; %d pixels with every segment occluded"
              % (sun_direction, mu_a, mu_b, mu_c, mu_b - mu_a, bound, 100 * bound / (mu_b - mu_c), tw["tails"], int(occluded.sum())))
        assert mu_b - mu_c > 0 and mu_c > 0 and tw["tails"] > 0
        assert abs(mu_b - mu_a) <= bound
        assert np.array_equal(a[occluded].view(np.uint32), b[occluded].view(np.uint32))
        assert np.array_equal(b[:, 0], b[:, 1]) and np.array_equal(b[:, 0], b[:, 2])
    finally:
        s.close()


# ---- 7. AS5: refusals -------------------------------------------------------------------------------------------------------------
def test_the_order_of_refusals(srt, oracle):
    import torch

    c = srt.capi
    s = Frame(srt, oracle, "scene1")
    pt = s.pt
    tn = torch.full((H, W), 0x0BAD, dtype=torch.int32, device="cuda:%d" % pt.device)
    try:
        pt.write_sample_budget(np.full((H, W), 3, np.uint32))
        pt.bind_sample_counts(tn)
        s.bound.sentinel()

        def call(fn, flags=16, bounces=2, reserved=0, rows=(0, H), max_samples=4096):
            p = c.AdaptiveParams()
            pt.L.srt_adaptive_params_default(C.byref(p))
            p.row_begin, p.row_end, p.max_bounces, p.seed, p.max_samples, p.flags, p.reserved = rows[0], rows[1], bounces, 3, max_samples, flags, reserved
            rc = fn(pt._h, C.byref(p))
            return rc, (pt.L.srt_last_error(pt._h) or b"").decode()

        plain, with_tail = pt.L.srt_render_adaptive, pt.L.srt_render_adaptive_tail

        def untouched():
            check(s.bound.read(), sentinels(), "a refused call")
            return bool((tn == 0x0BAD).all())

        def bad_sun(direction):
            e = srt.default_environment()
            e.sun_direction[:] = direction
            pt.set_environment(e)

        # flags 4, 8 and 4 | 16: SRT_ERR_INVALID_ARG, first — before the direction and, for the tail call, before the mode
        bad_sun(BAD_DIRECTIONS[0])
        for fn in (plain, with_tail):
            for flags in (4, 8, 4 | 16, 8 | 16):
                assert call(fn, flags)[0] == c.ERR_INVALID_ARG, flags
        assert untouched()
        for bad in BAD_DIRECTIONS:
            bad_sun(bad)
            # srt_render_adaptive: the own errors first, then the direction, also at max_bounces == 0
            assert call(plain, reserved=1)[0] == c.ERR_INVALID_ARG and call(plain, rows=(0, H + 1))[0] == c.ERR_INVALID_ARG
            assert call(plain, max_samples=0)[0] == c.ERR_INVALID_ARG and call(plain, bounces=-1)[0] == c.ERR_INVALID_ARG
            for bounces in (2, 0):
                rc, why = call(plain, bounces=bounces)
                assert rc == c.ERR_STATE and "sun_direction" in why, (bad, why)
            # srt_render_adaptive_tail with the mode off: the mode's refusal comes first
            rc, why = call(with_tail)
            assert rc == c.ERR_STATE and "srt_probe_tail is off" in why, (bad, why)
            assert untouched()
        # the mode on with no grid: the grid's refusal comes before the direction; then the direction last
        bad_sun(BAD_DIRECTIONS[0])
        tail(pt, PT.DEPTH)
        rc, why = call(with_tail)
        assert rc == c.ERR_STATE and "grid" in why and "sun_direction" not in why, why
        pt.set_probe_grid(GRID.origin, GRID.spacing, GRID.counts)
        rc, why = call(with_tail)
        assert rc == c.ERR_STATE and "coefficients" in why, why
        pt._ck(pt.L.srt_write_probe_grid_coefficients(pt._h, fp(CO), GRID.probes))
        rc, why = call(with_tail)
        assert rc == c.ERR_STATE and "depth" in why and "sun_direction" not in why, why
        pt._ck(pt.L.srt_write_probe_grid_depth(pt._h, fp(MO), GRID.probes, R))
        for bad in BAD_DIRECTIONS:
            bad_sun(bad)
            for bounces in (1, 0):
                rc, why = call(with_tail, bounces=bounces)
                assert rc == c.ERR_STATE and "sun_direction" in why, (bad, why)
        assert untouched()
        # without the flag the same direction is nobody's business
        assert call(with_tail, flags=0)[0] == c.OK and call(plain, flags=0)[0] == c.OK
        pt.wait()
        assert not bool((tn == 0x0BAD).any())
        # a good direction again: srt_render_adaptive with the flag succeeds while the mode is on; srt_trace_radiance is refused there
        pt.set_environment(srt.default_environment())
        assert call(plain)[0] == c.OK and call(with_tail)[0] == c.OK
        pt.write_rays(*s.rays)
        with pytest.raises(c.SrtError) as e:
            pt.trace_radiance(samples=1, bounces=1, sun_sampling=True)
        assert e.value.code == c.ERR_STATE
        pt.trace_radiance(samples=1, bounces=1)
    finally:
        pt.bind_sample_counts(None)
        s.close()


# ---- 8. layers --------------------------------------------------------------------------------------------------------------------
def test_the_renderers_setting_gives_the_bytes_of_the_python_route(srt):
    w, h, spp = 24, 20, 4
    co = np.random.RandomState(5).uniform(0.0, 1.0, (GRID.probes, 9, 4)).astype(F)
    G = 0x9E3779B9
    pt = srt.PathTracer(w, h)
    try:
        objs, cnt = srt.host.Scene(scene_path("Scene1")).objects_copy()
        pt.set_scene(objs, cnt)
        pt.set_camera(srt.default_camera())
        set_grid(pt, GRID, co)
        # the probe-tail frame: one flagged call from n = 0
        frames_ = {}
        for sun in (False, True):
            pt.probe_tail(enabled=True)
            pt.set_sample_counts(0)
            pt.write_sample_budget(np.full((h, w), spp, np.uint32))
            pt.render_adaptive_tail(bounces=1, seed=0, sun_sampling=sun)
            frames_[sun] = pt.framebuffer()
        assert not np.array_equal(frames_[True], frames_[False])
        pt.probe_tail(enabled=False)
        # the two-half workflow of PathTraceRenderer::renderAdaptiveFrame, call by call, the flag passed to every adaptive render
        halves = {}
        for sun in (False, True):
            pt.render(spp=spp // 2, bounces=2, seed=0)
            pt.bind_output(None, pt.half_ptr())
            pt.render(spp=spp // 2, bounces=2, seed=G)
            pt.bind_output()
            pt.set_sample_counts(spp // 2)
            pt.render_gbuffer(outputs=srt.capi.GBUF_OBJECT | srt.capi.GBUF_ALBEDO)
            for _ in range(2):
                pt.variance(albedo=True, merge=False, gbuffer=False)
                pt.sample_budget(threshold=0.05, floor=0.01, max_budget=8, albedo=True)
                pt.render_adaptive(bounces=2, seed=0, max_samples=8, keep_counts=True, sun_sampling=sun)
                pt.bind_output(None, pt.half_ptr())
                pt.render_adaptive(bounces=2, seed=G, max_samples=8, sun_sampling=sun)
                pt.bind_output()
            pt.variance(albedo=True, merge=True, gbuffer=False)
            halves[sun] = (pt.accumulator(), pt.sample_counts())
        assert not np.array_equal(halves[True][0].view(np.uint32), halves[False][0].view(np.uint32))
    finally:
        pt.close()
    sc = srt.host.Scene(scene_path("Scene1"))
    r = srt.host.Renderer(w, h)
    try:
        r.set_scene(sc)
        r.settings(fov=55, max_bounces=2, seed=0)
        r.set_probe_grid(GRID.origin, GRID.spacing, GRID.counts)
        assert srt.load_library().srt_write_probe_grid_coefficients(r.handle(), fp(co), GRID.probes) == 0
        r.probe_tail(enabled=True)
        r.render_probe_tail_frame(spp, bounces=1, seed=0)
        assert np.array_equal(r.framebuffer(), frames_[False])  # off by default
        r.sun_sampling(True)
        r.render_probe_tail_frame(spp, bounces=1, seed=0)
        assert np.array_equal(r.framebuffer(), frames_[True]) and (r.sample_counts() == spp).all()
        r.probe_tail(enabled=False)
        total, counts = r.render_adaptive_frame(spp, rounds=2, threshold=0.05, max_budget=8)
        assert same(r.accumulator(), halves[True][0]) and np.array_equal(counts, 2 * halves[True][1]) and total == int(counts.astype(np.int64).sum())
        r.sun_sampling(False)
        total, counts = r.render_adaptive_frame(spp, rounds=2, threshold=0.05, max_budget=8)
        assert same(r.accumulator(), halves[False][0]) and np.array_equal(counts, 2 * halves[False][1])
        # the per-call argument of host.py switches the setting on for one frame and leaves it as it was
        r.render_adaptive_frame(spp, rounds=2, threshold=0.05, max_budget=8, sun_sampling=True)
        assert same(r.accumulator(), halves[True][0])
        r.render_adaptive_frame(spp, rounds=2, threshold=0.05, max_budget=8)
        assert same(r.accumulator(), halves[False][0])
    finally:
        r.close()
        sc.close()


# ---- 9. error ---------------------------------------------------------------------------------------------------------------------
MEASURED_RATIO = {"Scene1": 2.81, "Scene2": 2.64}  # rmse(off) / rmse(on) of the camera-ray route; by AS2 the same figures
MEASURED_TAIL_RATIO = 1.84  # rmse(off) / rmse(on) of the tail frame, one measured run (see the docstring)


def _quality():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import adaptive_sun_quality as Q

    return Q


@pytest.mark.parametrize("name", list(MEASURED_RATIO))
def test_the_flag_lowers_the_error_of_an_adaptive_frame_at_equal_samples(srt, name):
    """tools/adaptive_sun_quality.py's protocol at 96 x 54: the relative luminance RMSE of the hit pixels of a uniform 16-sample,
    8-bounce srt_render_adaptive frame against a 4096-sample srt_render, flag off over flag on.  By AS2 the frames are the
    camera-ray radiance of tests/test_gpu_sun_sampling.py, whose measured ratios are 2.81 (Scene1) and 2.64 (Scene2); the test
    asserts half of each, as that test does.  One run here: Scene1, 2927 hit pixels, rmse 1.4846 off and 0.5281 on (ratio 2.81);
    Scene2, 2943 hit pixels, rmse 1.3401 off and 0.5066 on (ratio 2.65)."""
    Q = _quality()
    pt, rmse, info = Q.frame_setup(srt, name, 96, 54, 4096)
    try:
        off, on = rmse(16, False), rmse(16, True)
        ratio = off / on
        print("%s 96x54 B=8 n=16: rmse off %.4f, on %.4f, ratio %.2f (%s)" % (name, off, on, ratio, info))
        assert ratio >= MEASURED_RATIO[name] / 2
    finally:
        pt.close()


def test_the_flag_does_not_raise_the_error_of_a_tail_frame(srt):
    """tools/adaptive_sun_quality.py's tail protocol at 96 x 54 in Scene1: srt_render_adaptive_tail at 1 bounce and 64 samples
    under DEPTH | STATES, grid and inputs as tools/probe_tail_frame_quality.py makes them (spacing 0.5), the coefficients from
    probes traced at 8 bounces with the flag; relative luminance RMSE of the hit pixels against a 4096-sample, 8-bounce srt_render.
    Asserted: the flag does not raise the error (ratio >= 1).  The measured ratio is in MEASURED_TAIL_RATIO and in
    profiles/adaptive_sun/adaptive_sun_quality.jsonl; half of it is asserted too when it was measured at 2 or above (a regression
    guard taken from the code under test: the numpy loop and the unbiasedness test carry correctness).  One run: 2927 hit pixels,
    59475 probes, rmse 0.5587 off and 0.3031 on, ratio 1.84: below 2, so only ratio >= 1 is asserted."""
    Q = _quality()
    pt, rmse, info = Q.tail_setup(srt, "Scene1", 96, 54, 4096, 0.5)
    try:
        off, on = rmse(64, False), rmse(64, True)
        ratio = off / on
        print("Scene1 96x54 tail B=1 n=64: rmse off %.4f, on %.4f, ratio %.2f (%s)" % (off, on, ratio, info))
        assert ratio >= 1.0
        if MEASURED_TAIL_RATIO is not None and MEASURED_TAIL_RATIO >= 2:
            assert ratio >= MEASURED_TAIL_RATIO / 2
    finally:
        pt.bind_rays(None, None)
        pt.close()
