"""Sun sampling at diffuse bounces (SRT_RADIANCE_SUN_SAMPLING, SRT_LIGHT_PROBE_SUN_SAMPLING = 16; rules S1 - S9 of srt_pathtrace.h) on
the MI355X.  Comparisons are bit for bit in all four lanes with no ray left out, except the unbiasedness test, whose bound is
derived from the estimator's own variance.

The reference is tests/sun_sampling_reference.py: with the flag off its path loop is probe_tail_reference.path() (pinned against the
CPU oracle), and tests/test_sun_sampling_reference.py pins its cap samples and weights against the blind bounce's density.  24 x 20
camera rays make seven full blocks of 64 and one of 32 lanes.

"Straight down" in tests 3 and 4 is (0.001, -1, 0.001) normalised: the reference's box test (a slab test) answers a ray with a
component of exactly zero with a miss, so an exactly vertical ray never meets the floor."""
import ctypes as C

import numpy as np
import pytest

import light_probe_reference as LP
import probe_grid_reference as PG
import probe_tail_reference as PT
import sun_sampling_reference as SS
from test_gpu_probe_tail import SCENES, room_camera
from test_gpu_radiance import Scene, camera_rays, differing, same

pytestmark = pytest.mark.gpu

F = np.float32
W, H, N, SAMPLES = 24, 20, 480, 3
_paths = {}


@pytest.fixture(scope="module")
def scenes(srt, oracle):
    made = {}

    def get(name):
        if name not in made:
            s = Scene(srt, oracle, SCENES[name](oracle))
            s.ref = SS.SunScene(PT.Scene(oracle, s.oarr, s.n, om=s.om[:2] if s.om else None, env=s.env))
            s.rays = camera_rays(oracle, room_camera(oracle) if name == "room" else oracle.default_camera())
            made[name] = s
        return made[name]

    yield get
    for s in made.values():
        s.close()


def paths(s, name, bounces, seed):
    key = (name, bounces, seed)
    if key not in _paths:
        _paths[key] = SS.trace(s.ref, s.rays[0], s.rays[1], SAMPLES, bounces, seed=seed)
    return _paths[key]


def custom(srt, oracle, objs, env=None, w=8, h=8):
    """A tracer with a scene of dicts and an environment of the oracle's layout, and the reference of the same."""
    s = Scene(srt, oracle, (objs, None), w, h)
    if env is not None:
        s.env = env
        e = srt.default_environment()
        for k in ("sun_direction", "sky_color", "horizon_color", "ground_color", "sun_color"):
            getattr(e, k)[:] = getattr(env, k)[:]
        s.pt.set_environment(e)
    s.ref = SS.SunScene(PT.Scene(oracle, s.oarr, s.n, env=s.env))
    return s


def down_rays(points, y=0.5):
    """Rays from height y "straight down" (see the module's docstring) that meet the plane y = -1 at `points` (x, z)."""
    d = np.array([0.001, -1.0, 0.001], np.float64)
    d /= np.linalg.norm(d)
    t = (y + 1.0) / -d[1]
    o = np.zeros((len(points), 4), F)
    dd = np.zeros((len(points), 4), F)
    for i, (x, z) in enumerate(points):
        o[i, :3] = (x - t * d[0], y, z - t * d[2])
    dd[:, :3] = d
    return o, dd


def floor(oracle, **kw):
    return dict(type=oracle.OBJ_BOX, position=(0.0, -1.5, 5.0), half_size=(20.0, 0.5, 20.0), base=(1.0, 1.0, 1.0), smoothness=0.0, specular_amount=0.0, **kw)


# ---- 1. bit for bit against the reference loop ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounces", [1, 2, 8])
@pytest.mark.parametrize("name", list(SCENES))
def test_every_ray_has_the_reference_loops_bits(scenes, name, bounces):
    s = scenes(name)
    seed = 3 + bounces
    colours, segments, opened = paths(s, name, bounces, seed)
    want = SS.radiance(colours)
    o, d = s.rays
    s.pt.trace_radiance(o, d, samples=SAMPLES, bounces=bounces, seed=seed, count_work=True, sun_sampling=True)
    got, on = s.pt.radiance(), s.pt.radiance_work()
    s.pt.trace_radiance(samples=SAMPLES, bounces=bounces, seed=seed, count_work=True)
    plain, off = s.pt.radiance(), s.pt.radiance_work()
    print("%s B=%d: %d rays differ from the reference; %d segments, %d open; wave_calls %d -> %d; %d rays change with the flag"
          % (name, bounces, differing(got, want), segments, opened, off["wave_calls"], on["wave_calls"], differing(got, plain)))
    assert same(got, want), "%d of %d rays differ from the reference" % (differing(got, want), N)
    assert segments > 0
    if name == "room":  # the closed room traces segments and finds all of them occluded
        assert opened == 0
    if name == "scene1":
        assert opened > 0 and not same(got, plain)
    # S9: closest_calls is the path's; wave_calls counts the any-hit invocations on top
    assert on["closest_calls"] == off["closest_calls"] and on["samples"] == off["samples"] and on["rays"] == off["rays"]
    assert off["wave_calls"] < on["wave_calls"] <= off["wave_calls"] + segments


# ---- 2. the invariants of S8 ------------------------------------------------------------------------------------------------------
def test_a_black_sun_and_an_all_mirror_scene_give_the_bits_without_the_flag(srt, oracle, scenes):
    s = scenes("scene1")
    o, d = s.rays
    e = srt.default_environment()
    try:
        black = srt.default_environment()
        black.sun_color[:] = (0.0, 0.0, 0.0)
        s.pt.set_environment(black)
        s.pt.trace_radiance(o, d, samples=SAMPLES, bounces=8, seed=2)
        off = s.pt.radiance()
        s.pt.trace_radiance(samples=SAMPLES, bounces=8, seed=2, sun_sampling=True, count_work=True)
        assert same(s.pt.radiance(), off)
        assert s.pt.radiance_work()["wave_calls"] > 0
    finally:
        s.pt.set_environment(e)
    # no diffuse vertex: SpecularAmount >= 1 and Smoothness > 0 everywhere
    objs = [dict(type=oracle.OBJ_BOX, position=(0.0, -1.5, 5.0), half_size=(20.0, 0.5, 20.0), base=(0.7, 0.7, 0.7), smoothness=0.3, specular_amount=1.0),
            dict(type=oracle.OBJ_SPHERE, position=(0.0, 0.0, 5.0), radius=1.0, base=(0.9, 0.4, 0.2), smoothness=1.0, specular_amount=2.0, specular=(0.9, 0.9, 0.9))]
    m = custom(srt, oracle, objs, w=W, h=H)
    try:
        o, d = camera_rays(oracle, oracle.default_camera())
        m.pt.trace_radiance(o, d, samples=SAMPLES, bounces=8, seed=4, count_work=True)
        off, off_work = m.pt.radiance(), m.pt.radiance_work()
        m.pt.trace_radiance(samples=SAMPLES, bounces=8, seed=4, count_work=True, sun_sampling=True)
        assert same(m.pt.radiance(), off) and m.pt.radiance_work() == off_work
        assert off_work["closest_calls"] > off_work["samples"]  # (paths do bounce there)
    finally:
        m.close()


def test_continuation_splitting_and_seventy_samples_under_the_flag(scenes):
    s = scenes("scene1")
    o, d = s.rays
    pt = s.pt
    pt.trace_radiance(o, d, samples=9, bounces=2, seed=5, sun_sampling=True)
    whole = pt.radiance()
    pt.trace_radiance(samples=3, bounces=2, seed=5, first_sample=1, reset=True, sun_sampling=True)
    first = pt.radiance()
    pt.trace_radiance(samples=6, bounces=2, seed=5, first_sample=4, reset=False, sun_sampling=True)
    assert same(pt.radiance(), whole) and not same(first, whole)
    parts = []
    for a, b in ((0, 200), (200, N)):
        pt.trace_radiance(o[a:b], d[a:b], samples=9, bounces=2, seed=5, id_base=a, sun_sampling=True)
        parts.append(pt.radiance())
    assert same(np.concatenate(parts), whole)
    pt.trace_radiance(o, d, samples=9, bounces=2, seed=5)
    assert not same(pt.radiance(), whole)
    # 70 samples cross the chunk of 64: eight rays of the middle rows against the reference
    pick = np.arange(200, 208)
    colours, segments, _ = SS.trace(s.ref, o[pick], d[pick], 70, 2, seed=9)
    assert segments > 0
    pt.trace_radiance(o[pick], d[pick], samples=70, bounces=2, seed=9, sun_sampling=True)
    assert same(pt.radiance(), SS.radiance(colours))


@pytest.mark.parametrize("K", [64, 96])
def test_light_probes_under_the_flag(scenes, K):
    import torch

    s = scenes("scene1")
    pt = s.pt
    pos = np.zeros((6, 4), F)
    pos[:, :3] = [(-1.5, 0.2, 2.0), (0.0, 0.5, 3.0), (1.2, 0.4, 4.0), (0.4, 1.0, 2.5), (-0.6, 0.5, 4.5), (1.8, 0.3, 1.5)]
    dirs = LP.sphere(K).reshape(K, 4).astype(F)
    dev = "cuda:%d" % pt.device
    try:
        pt.trace_light_probes(pos, dirs, samples=SAMPLES, bounces=2, seed=4, radiance=True, count_work=True, sun_sampling=True)
        rad, co, on = pt.light_probe_radiance(), pt.light_probe_coefficients(), pt.light_probe_work()
        pt.trace_light_probes(samples=SAMPLES, bounces=2, seed=4, radiance=True, count_work=True)
        off = pt.light_probe_work()
        assert not same(pt.light_probe_radiance(), rad)
        assert on["closest_calls"] == off["closest_calls"] and on["wave_calls"] > off["wave_calls"]
        # RADIANCE: srt_trace_radiance on the explicit rays under the flag
        o = np.repeat(pos, K, axis=0)
        d = np.tile(dirs, (6, 1))
        pt.trace_radiance(o, d, samples=SAMPLES, bounces=2, seed=4, sun_sampling=True)
        explicit = pt.radiance()
        assert same(rad.reshape(-1, 4), explicit), "%d of %d rays differ from srt_trace_radiance" % (differing(rad.reshape(-1, 4), explicit), 6 * K)
        assert same(co, LP.project(rad, dirs))
        # the listed call: probes 1, 3 and 4 as the unlisted call writes them, the others' sentinel
        t_co = torch.full((6 * 9, 4), -7.0, dtype=torch.float32, device=dev)
        t_rad = torch.full((6 * K, 4), -7.0, dtype=torch.float32, device=dev)
        pt.bind_light_probe_output("coefficients", t_co)
        pt.bind_light_probe_output("radiance", t_rad)
        pt.bind_probe_list(np.array([3, 6, 0, 0, 1, 3, 4, 0, 0, 0], np.uint32))
        pt.trace_light_probes(samples=SAMPLES, bounces=2, seed=4, radiance=True, listed=True, sun_sampling=True)
        pt.wait()
        lco, lrad = t_co.cpu().numpy().reshape(6, 9, 4), t_rad.cpu().numpy().reshape(6, K, 4)
        for p in range(6):
            if p in (1, 3, 4):
                assert same(lco[p], co[p]) and same(lrad[p], rad[p]), p
            else:
                assert (lco[p] == -7.0).all() and (lrad[p] == -7.0).all(), p
    finally:
        pt.bind_light_probe_output("coefficients", None)
        pt.bind_light_probe_output("radiance", None)
        pt.bind_probe_list(None)


# ---- 3. work ----------------------------------------------------------------------------------------------------------------------
def test_one_ray_of_sixty_four_samples_makes_one_any_hit_call(srt, oracle):
    s = custom(srt, oracle, [floor(oracle)])
    try:
        o, d = down_rays([(0.3, 4.1)])
        s.pt.trace_radiance(o, d, samples=64, bounces=1, seed=0, count_work=True)
        off = s.pt.radiance_work()
        s.pt.trace_radiance(samples=64, bounces=1, seed=0, count_work=True, sun_sampling=True)
        on = s.pt.radiance_work()
        colours, segments, opened = SS.trace(s.ref, o, d, 64, 1, seed=0)
        assert same(s.pt.radiance(), SS.radiance(colours)) and segments == opened == 64
        assert on["wave_calls"] == off["wave_calls"] + 1 and on["closest_calls"] == off["closest_calls"]
    finally:
        s.close()


# ---- 4. unbiasedness --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sun_direction", [(0.0, -1.0, 0.0), (-1.0, -1.0, -1.0)])
def test_the_flag_does_not_change_the_mean(srt, oracle, sun_direction):
    """A black sky with SunColor = (10, 10, 10) over one white diffuse floor, 64 rays straight down onto distinct points, 1 bounce,
    4096 samples.  Without the flag a sample is exactly 10 * [the blind bounce falls into the cap]; so with p = mu_on / 10 the
    difference of the two batch means has a standard deviation of at most 10 * sqrt(p (1 - p) / (64 * 4096)) (the flag's own
    variance is far smaller), and five of them are the bound: about 13 % of the mean for the sun overhead, 7 % for the diagonal sun.
    A weight of k instead of (pi k / 6) / m^3 is off by 89 % and 51 %.  16 further rays end in the full shadow of a sphere that
    covers the whole cap: both calls give exactly 0 there."""
    sd = np.array(sun_direction, np.float64)
    sd /= np.linalg.norm(sd)
    env = oracle.default_environment()
    env.sun_direction[:] = [float(F(v)) for v in sd]
    env.sky_color[:] = env.horizon_color[:] = env.ground_color[:] = (0.0, 0.0, 0.0)
    env.sun_color[:] = (10.0, 10.0, 10.0)
    lit = custom(srt, oracle, [floor(oracle)], env)
    try:
        pts = [(-3.0 + 0.7 * (i % 8) + 0.013 * i, 2.0 + 0.6 * (i // 8)) for i in range(64)]
        o, d = down_rays(pts)
        lit.pt.trace_radiance(o, d, samples=4096, bounces=1, seed=21)
        off = lit.pt.radiance()
        lit.pt.trace_radiance(samples=4096, bounces=1, seed=21, sun_sampling=True)
        on = lit.pt.radiance()
        mu_off, mu_on = float(np.mean(off[:, 0], dtype=np.float64)), float(np.mean(on[:, 0], dtype=np.float64))
        p = mu_on / 10.0
        bound = 5.0 * 10.0 * np.sqrt(p * (1.0 - p) / (64 * 4096))
        print("sun_direction %s: mean without the flag %.5f, with %.5f, difference %.5f, bound %.5f (%.1f %% of the mean); a k weight would give %.5f"
              % (sun_direction, mu_off, mu_on, mu_on - mu_off, bound, 100 * bound / mu_on, 10 * float(SS.K)))
        assert mu_on > 0 and mu_off > 0
        assert abs(mu_on - mu_off) <= bound
        assert np.array_equal(on[:, 0], on[:, 1]) and np.array_equal(on[:, 0], on[:, 2])
    finally:
        lit.close()
    # the shadow: a sphere of radius 1.5 whose centre lies 4 along s above the patch; the cap's cone is 0.57 wide there
    centre = np.array([0.0, -1.0, 5.0]) + 4.0 * -sd
    ball = dict(type=oracle.OBJ_SPHERE, position=tuple(float(v) for v in centre), radius=1.5, base=(1.0, 1.0, 1.0), smoothness=0.0, specular_amount=0.0)
    dark = custom(srt, oracle, [floor(oracle), ball], env)
    try:
        pts = [(-0.15 + 0.1 * (i % 4), 4.85 + 0.1 * (i // 4)) for i in range(16)]
        o, d = down_rays(pts, y=-0.5)
        for sun in (False, True):
            dark.pt.trace_radiance(o, d, samples=4096, bounces=1, seed=22, sun_sampling=sun, count_work=True)
            got = dark.pt.radiance()
            assert dark.pt.radiance_work()["closest_calls"] == 2 * 16 * 4096  # (every primary ray meets the floor)
            assert (got[:, :3] == 0.0).all(), (sun, got[:, 0])
    finally:
        dark.close()


# ---- 5. errors --------------------------------------------------------------------------------------------------------------------
def test_the_flags_two_refusals(srt, oracle, scenes):
    import torch

    c = srt.capi
    s = scenes("scene1")
    pt = s.pt
    o, d = s.rays
    pt.write_rays(o, d)

    def rc(flags, bounces=2):
        p = c.RadianceParams()
        pt.L.srt_radiance_params_default(C.byref(p))
        p.sample_count, p.max_bounces, p.flags = SAMPLES, bounces, flags
        return pt.L.srt_trace_radiance(pt._h, C.byref(p))

    def lp(flags, listed):
        p = c.LightProbeParams()
        pt.L.srt_light_probe_params_default(C.byref(p))
        p.sample_count, p.max_bounces, p.flags = 1, 1, flags
        return (pt.L.srt_trace_light_probes_listed if listed else pt.L.srt_trace_light_probes)(pt._h, C.byref(p))

    assert c.RADIANCE_SUN_SAMPLING == 16 and c.LIGHT_PROBE_SUN_SAMPLING == 16
    assert rc(8) == c.ERR_INVALID_ARG and rc(8 | 16) == c.ERR_INVALID_ARG and rc(1 | 16) == c.OK
    pos = np.zeros((2, 4), F)
    pos[:, :3] = [(-1.0, 0.5, 3.0), (0.0, 0.5, 3.0)]
    pt.trace_light_probes(pos, 64, samples=1, bounces=1)
    pt.bind_probe_list(np.array([1, 2, 0, 0, 1, 0], np.uint32))
    # the probe-tail mode: refused with the flag, and the same call without the flag is what it was
    grid = PG.Grid((-2.0, -1.0, 1.0), (1.0, 0.8, 1.2), (5, 4, 5))
    co = np.random.RandomState(3).uniform(0.0, 1.0, (grid.probes, 9, 4)).astype(F)
    pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
    pt._ck(pt.L.srt_write_probe_grid_coefficients(pt._h, np.ascontiguousarray(co).ctypes.data_as(C.POINTER(C.c_float)), grid.probes))
    try:
        pt.probe_tail(enabled=True)
        assert rc(1) == c.OK
        before = pt.radiance(N)
        assert rc(1 | 16) == c.ERR_STATE and rc(1 | 16, bounces=0) == c.ERR_STATE
        assert lp(1 | 16, False) == c.ERR_STATE and lp(1 | 16, True) == c.ERR_STATE and lp(1, False) == c.OK and lp(1, True) == c.OK
        assert same(pt.radiance(N), before)  # (the refused calls wrote nothing)
        assert rc(1) == c.OK and same(pt.radiance(N), before)
        pt.probe_tail(enabled=False)
        assert rc(1 | 16) == c.OK and not same(pt.radiance(N), before)
    finally:
        pt.probe_tail(enabled=False)
        pt.bind_probe_list(None)
    # a sun direction that is not a unit vector: refused, and the bound output keeps its bytes
    t = torch.full((N, 4), 0.25, dtype=torch.float32, device="cuda:%d" % pt.device)
    pt.bind_radiance(t)
    try:
        for bad in ((0.0, -2.0, 0.0), (0.0, 0.0, 0.0), (float("nan"), -1.0, 0.0), (float("inf"), 0.0, 0.0)):
            e = srt.default_environment()
            e.sun_direction[:] = bad
            pt.set_environment(e)
            assert rc(1 | 16) == c.ERR_STATE and lp(1 | 16, False) == c.ERR_STATE, bad
            pt.wait()
            assert bool((t == 0.25).all())
        assert rc(1) == c.OK  # (without the flag the direction is nobody's business)
        pt.wait()
        assert not bool((t == 0.25).all())
    finally:
        pt.set_environment(srt.default_environment())
        pt.bind_radiance(None)


# ---- 6. error reduction -----------------------------------------------------------------------------------------------------------
MEASURED_RATIO = {"Scene1": 2.81, "Scene2": 2.64}  # rmse(off) / rmse(on), one measured run (see the docstring)


@pytest.mark.parametrize("name", list(MEASURED_RATIO))
def test_the_flag_lowers_the_error_at_equal_samples(srt, name):
    """tools/sun_sampling_quality.py's protocol at 96 x 54: the relative luminance RMSE of the hit pixels of camera-ray radiance at
    16 samples and 8 bounces against a 4096-sample srt_render, flag off and flag on.  The measured ratios rmse(off) / rmse(on) are in
    MEASURED_RATIO; the test asserts half of a ratio measured at 2 or above, and nothing otherwise.  One run: Scene1, 2927 hit
    pixels, rmse 1.4846 off and 0.5281 on (ratio 2.81); Scene2, 2943 hit pixels, rmse 1.3401 off and 0.5067 on (ratio 2.64)."""
    import os
    import sys

    from conftest import ROOT

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sun_sampling_quality as Q

    pt, rmse, info = Q.frame_setup(srt, name, 96, 54, 4096)
    try:
        off, on = rmse(16, False), rmse(16, True)
        ratio = off / on
        print("%s 96x54 B=8 n=16: rmse off %.4f, on %.4f, ratio %.2f (%s)" % (name, off, on, ratio, info))
        measured = MEASURED_RATIO[name]
        if measured is not None and measured >= 2:
            assert ratio >= measured / 2
    finally:
        pt.bind_rays(None, None)
        pt.close()
