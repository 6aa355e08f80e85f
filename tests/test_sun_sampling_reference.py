"""tests/sun_sampling_reference.py is the reference of the sun-sampling GPU tests.  What entitles it: with the flag off its path
loop is probe_tail_reference.path() bit for bit (which is pinned against the CPU oracle's accumulator); with SunColor = (0, 0, 0)
the flag changes nothing (rule S8); the frame of rule S5 is orthonormal; and the cap samples of rule S4 lie in the cap and, weighted
by rule S6, reproduce the fraction of the blind bounce's directions that fall into the cap — the figures of DESIGN.md §4.38,
from 4e7 cube-normalised, folded directions each in double precision.  No GPU."""
import numpy as np
import pytest

import probe_tail_reference as PT
import sun_sampling_reference as SS
from conftest import scene_path
from test_probe_tail_reference import camera_rays
from visibility_reference import mix32

F = np.float32
W, H, SAMPLES = 12, 10, 2


def scene(oracle, name, env=None):
    oarr, n = oracle.make_objects(oracle.load_scene_json_py(scene_path(name)))
    sc = PT.Scene(oracle, oarr, n, env=env if env is not None else oracle.default_environment())
    sc.keep = oarr
    return sc


def bits(colour):
    return np.array(colour, F).view(np.uint32).tolist()


@pytest.mark.parametrize("name", ["Scene1", "Scene_indirect"])
def test_with_the_flag_off_the_loop_is_the_probe_tail_references(oracle, name):
    sc = scene(oracle, name)
    ss = SS.SunScene(sc)
    o, d = camera_rays(oracle, oracle.default_camera(), W, H)
    segments = changed = 0
    for bounces, seed in ((0, 1), (1, 0), (8, 3)):
        for i in range(W * H):
            for f in range(1, 1 + SAMPLES):
                want, _ = PT.path(sc, o[i][:3], d[i][:3], bounces, seed, i, f)
                got, sg, op = SS.path_sun(ss, o[i][:3], d[i][:3], bounces, seed, i, f, sun=False)
                assert bits(got) == bits(want) and sg == 0 and op == 0
                on, sg, op = SS.path_sun(ss, o[i][:3], d[i][:3], bounces, seed, i, f, sun=True)
                assert op <= sg <= bounces and bits(on)[3] == bits(want)[3]  # (the alpha lane is the path's: S1)
                segments += sg
                changed += bits(on) != bits(want)
    print("%s: %d segments, %d of %d samples change" % (name, segments, changed, 3 * W * H * SAMPLES))
    assert segments > 0 and changed > 0  # (the flag does something in a sunlit scene)


def test_with_a_black_sun_the_flag_changes_nothing(oracle):
    env = oracle.default_environment()
    env.sun_color[:] = (0.0, 0.0, 0.0)
    ss = SS.SunScene(scene(oracle, "Scene1", env))
    o, d = camera_rays(oracle, oracle.default_camera(), W, H)
    segments = 0
    for i in range(W * H):
        for f in range(1, 1 + SAMPLES):
            off, _, _ = SS.path_sun(ss, o[i][:3], d[i][:3], 8, 5, i, f, sun=False)
            on, sg, _ = SS.path_sun(ss, o[i][:3], d[i][:3], 8, 5, i, f, sun=True)
            assert bits(on) == bits(off)
            segments += sg
    assert segments > 0  # (segments are traced all the same: they add +0)


def unit_directions():
    rng = np.random.RandomState(38)
    v = rng.normal(size=(50, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    return [tuple(F(x) for x in r) for r in v] + [tuple(F(x) for x in a) for a in axes]


def test_the_frame_is_orthonormal():
    for sun_direction in unit_directions():
        assert SS.frame_ok(sun_direction)
        s, t1, t2 = (np.array(v, np.float64) for v in SS.frame(sun_direction))
        assert np.array_equal(s, -np.array(sun_direction, np.float64))
        for a, b, want in ((s, s, 1), (t1, t1, 1), (t2, t2, 1), (s, t1, 0), (s, t2, 0), (t1, t2, 0)):
            assert abs(float(a @ b) - want) <= 1e-6, (sun_direction, a, b)
        assert np.allclose(np.cross(t1, t2), s, atol=2e-6)  # right-handed: t1 x t2 = s
    for bad in ((0, 0, 0), (0, -1.0001, 0), (np.nan, 0, 1), (np.inf, 0, 0), (0.6, 0.6, 0.6)):
        assert not SS.frame_ok(bad)


# the fraction of 4e7 cube-normalised, folded directions (double precision) that fall into the cap about s, +- one standard error
CAP_FRACTIONS = {(0.0, 1.0, 0.0): (0.005298, 0.000012), (1.0, 1.0, 1.0): (0.020339, 0.000023), (0.3, 0.8, -0.52): (0.010578, 0.000016)}


@pytest.mark.parametrize("s", list(CAP_FRACTIONS))
def test_cap_samples_lie_in_the_cap_and_their_weight_is_the_blind_bounces_density(s):
    want, _ = CAP_FRACTIONS[s]
    sd64 = np.array(s, np.float64)
    sd64 /= np.linalg.norm(sd64)
    sun_direction = tuple(F(-x) for x in sd64)
    assert SS.frame_ok(sun_direction)
    fr = SS.frame(sun_direction)
    keys = mix32(np.arange(20000, dtype=np.uint32) + np.uint32(0x1234567))
    w = SS.cap_sample(keys, fr)
    # element by element the array form is the scalar form
    for j in (0, 1, 7, 19999):
        one = SS.cap_sample(keys[j], fr)
        assert [F(one[l]).view(np.uint32) for l in range(3)] == [w[l][j].view(np.uint32) for l in range(3)]
    sd = SS.dot3(w, fr[0])
    assert (sd >= SS.CAP - F(2.0 ** -20)).all()
    inside = sd >= SS.CAP
    wt = SS.weight(w)
    got = float(np.mean(wt[inside], dtype=np.float64))
    print("s = %s: %d of %d samples inside, mean weight %.6f, reference fraction %.6f, a plain k weight would give %.4f"
          % (s, int(inside.sum()), len(keys), got, want, float(SS.K)))
    assert inside.sum() >= 0.99 * len(keys)
    assert abs(got - want) <= 0.02 * want
