"""tests/adaptive_sun_reference.py is the reference of the combination of sun sampling and the probe tail (rule AS4 of
srt_pathtrace.h), for which no radiance call exists to compare with.  What entitles it: with sun=False its path loop is
probe_tail_reference.path() under the tail bit for bit — colour and terminal state — and without a tail it is
sun_sampling_reference.path_sun() bit for bit, segments included; both on the five scenes of the GPU tests at 1 / 2 / 8 bounces
over a 24 x 20 frame with three samples.  The two references it is compared with are pinned by their own tests.  No GPU."""
import numpy as np
import pytest

import adaptive_sun_reference as AS
import probe_tail_reference as PT
import sun_sampling_reference as SS
from test_probe_tail_reference import camera_rays

F = np.float32
W, H, SAMPLES = 24, 20, 3


def scene_of(oracle, name):
    """The scene `name` of tests/test_gpu_probe_tail.py's SCENES as (reference scene, sun scene, camera rays)."""
    from test_gpu_probe_tail import SCENES, room_camera

    objs, meshes = SCENES[name](oracle)
    oarr, n = oracle.make_objects(objs)
    om = None
    if meshes:
        marr, mn, keep = oracle.make_meshes(meshes)
        om = (marr, mn, keep)
    sc = PT.Scene(oracle, oarr, n, om=om[:2] if om else None, env=oracle.default_environment())
    sc.keep = (oarr, om)
    cam = room_camera(oracle) if name == "room" else oracle.default_camera()
    return sc, SS.SunScene(sc), camera_rays(oracle, cam, W, H)


def bits(colour):
    return np.array(colour, F).view(np.uint32).tolist()


def terminal_bits(t):
    if t is None:
        return None
    return bits(t["x"]) + bits(t["n"]) + bits(t["T"]) + bits([t["g"]])


@pytest.mark.parametrize("name", ["scene1", "room", "reflection", "mesh", "memory"])
def test_both_identities_on_the_scenes_of_the_gpu_tests(oracle, name):
    sc, ss, (o, d) = scene_of(oracle, name)
    segments = terminals = both = 0
    for bounces in (1, 2, 8):
        seed = 3 + bounces
        for i in range(W * H):
            for f in range(1, 1 + SAMPLES):
                # sun=False: probe_tail_reference.path() under the tail
                want, wt = PT.path(sc, o[i][:3], d[i][:3], bounces, seed, i, f)
                got, gt, sg, op = AS.path_sun_tail(ss, o[i][:3], d[i][:3], bounces, seed, i, f, sun=False, tail=True)
                assert bits(got) == bits(want) and terminal_bits(gt) == terminal_bits(wt) and sg == 0 and op == 0
                # tail=False: sun_sampling_reference.path_sun()
                want, wsg, wop = SS.path_sun(ss, o[i][:3], d[i][:3], bounces, seed, i, f, sun=True)
                got, gt, sg, op = AS.path_sun_tail(ss, o[i][:3], d[i][:3], bounces, seed, i, f, sun=True, tail=False)
                assert bits(got) == bits(want) and gt is None and (sg, op) == (wsg, wop)
                # both: the colour before the lookup is path_sun's, the terminal state is path()'s (AS4: the lookup is unchanged)
                got, gt, sg, op = AS.path_sun_tail(ss, o[i][:3], d[i][:3], bounces, seed, i, f, sun=True, tail=True)
                assert bits(got) == bits(want) and terminal_bits(gt) == terminal_bits(wt) and (sg, op) == (wsg, wop)
                segments += sg
                terminals += gt is not None
                both += gt is not None and sg > 0
    print("%s: %d segments, %d terminal states, %d samples with both" % (name, segments, terminals, both))
    assert terminals > 0
    if name != "reflection":  # (the mirror scene's camera paths may end without a diffuse vertex)
        assert segments > 0 and both > 0
