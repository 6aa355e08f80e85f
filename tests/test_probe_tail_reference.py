"""tests/probe_tail_reference.py is the reference of the probe-tail GPU tests.  What entitles it: with the tail off its path loop
gives, for every camera ray of a frame, the accumulator of the CPU oracle (POW_SHARED) bit for bit in all four lanes — here for
24 x 20 rays, three samples and 1, 2 and 8 bounces in Scene1, Scene_indirect and Scene1_reflection.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import probe_tail_reference as PT
from conftest import scene_path

W, H, SAMPLES = 24, 20, 3


def camera_rays(oracle, cam, w=W, h=H):
    o = np.zeros((w * h, 4), np.float32)
    d = np.zeros((w * h, 4), np.float32)
    o[:, :3] = np.array(cam.position[:], np.float32)
    out = (C.c_float * 3)()
    for y in range(h):
        for x in range(w):
            oracle.lib().srt_oracle_ray_direction(C.byref(cam), w, h, x, y, out)
            d[x + y * w, :3] = out[:]
    return o, d


@pytest.mark.parametrize("scene", ["Scene1", "Scene_indirect", "Scene1_reflection"])
def test_the_path_loop_without_a_tail_is_the_oracle(oracle, scene):
    oarr, n = oracle.make_objects(oracle.load_scene_json_py(scene_path(scene)))
    cam, env = oracle.default_camera(), oracle.default_environment()
    sc = PT.Scene(oracle, oarr, n, env=env)
    o, d = camera_rays(oracle, cam)
    for bounces, seed in ((1, 0), (2, 7), (8, 3)):
        _, want, _ = oracle.render(oarr, n, env, cam, W, H, spp=SAMPLES, bounces=bounces, seed=seed, pow_mode=oracle.POW_SHARED)
        colours, terminals = PT.trace(sc, o, d, SAMPLES, bounces, seed=seed)
        got = PT.radiance(colours)
        want = want.reshape(W * H, 4)
        differ = int((got.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum())
        ended = sum(t is not None for t in terminals)
        print("%s B=%d: %d of %d rays differ, %d of %d paths end at the limit on a surface" % (scene, bounces, differ, W * H, ended, len(terminals)))
        assert differ == 0
        # a terminal state is what rule T2 says: a surface point, a unit-length normal's worth of floats, g in [0, 1]
        for t in terminals:
            assert t is None or (len(t["x"]) == 3 and len(t["n"]) == 3 and len(t["T"]) == 3 and 0.0 <= float(t["g"]) <= 1.0)
