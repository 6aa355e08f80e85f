"""The six-wave rows kernel (k_lds_rows6 in srt_capi.hip, chosen by srt::rows_six_waves in csrc/srt_launch_shape.h where six
workgroups' LDS fit into a CU's 160 KiB) on both sides of its threshold, against the oracle: framebuffer and all four accumulator
lanes bit for bit, NaNs compared as NaNs.

The frame is the 40 x 24 of test_gpu_sample_rows.py (partial blocks, tiles that mix sky and traced pixels, several workgroups); the
sample counts 2, 8 and 15 lie inside the window in which such a frame takes the rows path.  The scene is Scene1 plus a grid of
small spheres in front of it.  How many is taken from the rule itself: tests/native/six_wave_rule_check.cpp --grow builds the
scene image of Scene1 plus the first k spheres with the library's own build_scene_image and prints the rule's answer for every k;
`over` is the first k at which six workgroups no longer fit (the image still lives in LDS, so the launch keeps the rows path and
takes the five-wave kernel), `fits` = over - 1 is the last at which they do.  The library does not report which kernel a launch
took (no ABI change); on the fitting side the shipped library is also compared with the development library's variant 5, which
forces the five-wave rows kernel.  The counting launch stays at five waves and keeps the hand-out's step counts.
The rule itself is checked on the CPU (test_six_wave_rule).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path

W, H = 40, 24
THREADS = 16
SPPS = [2, 8, 15]
CSRC = os.path.join(ROOT, "software-raytracer_amd", "csrc")
HOST = os.path.join(ROOT, "software-raytracer_amd", "host")
GROW_MAX = 120
_ORACLE = {}


def _extra_sphere(k):
    """the k-th extra sphere: a grid of radius-1/16 spheres, 13 across, in front of the scene (dyadic numbers: exact as text)"""
    return (-1.5 + 0.25 * (k % 13), -0.5 + 0.25 * (k // 13), 2.5, 0.0625)


@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    """tests/native/six_wave_rule_check.cpp under ASan + UBSan, built once"""
    exe = str(tmp_path_factory.mktemp("six_wave") / "six_wave_rule_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC, "-I" + HOST, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "six_wave_rule_check.cpp"), os.path.join(HOST, "scene.cpp"), "-o", exe],
                   check=True, capture_output=True)
    return exe


def threshold_counts(exe, first=()):
    """{"fits": k, "over": k + 1, "bytes": {k: LDS bytes}}: the counts of extra spheres either side of the threshold, from the rule,
    for Scene1 plus the spheres `first` (x, y, z, radius) plus the first k of the grid"""
    text = "".join("%r %r %r %r\n" % tuple(s) for s in list(first) + [_extra_sphere(k) for k in range(GROW_MAX)])
    r = subprocess.run([exe, "--grow", scene_path("Scene1")], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-2000:]
    rows = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert [k for k, _, _ in rows] == list(range(len(first) + GROW_MAX + 1))
    assert rows[0][2] == 1, "plain Scene1 must pass the rule"
    rows = [(k - len(first), b, six) for k, b, six in rows[len(first):]]  # (k counts the grid's spheres)
    over = next(k for k, _, six in rows if not six)
    assert over >= 1, "the spheres ahead of the grid must leave the scene under the threshold"
    ring = 4 * 64 * 2 * 16  # (what the ring kernels' workgroups hold on top: whether an image lives in LDS is judged with it)
    print("six-wave threshold: %d spheres -> %d bytes (fits), %d -> %d bytes (over)" % (over - 1, rows[over - 1][1], over, rows[over][1]))
    assert rows[over - 1][2] == 1 and rows[over][1] > 26880 >= rows[over - 1][1]
    assert rows[over][1] + ring <= 64 * 1024, "the image must still live in LDS"
    # (Scene1's image is 5.2 KB; a small sphere costs four rows of 16 bytes and a quarter of a cluster bound: about 60 cross 8448 bytes)
    assert 40 - 2 * len(first) <= over <= 80, over
    return {"fits": over - 1, "over": over, "bytes": {k: b for k, b, _ in rows}}


@pytest.fixture(scope="module")
def counts(rule_exe):
    """{"fits": k, "over": k + 1}: the sphere counts either side of the threshold, from the rule"""
    return threshold_counts(rule_exe)


def _objects(oracle, n_extra, first=()):
    """Scene1, the objects `first`, and n_extra spheres of the grid"""
    objs = oracle.load_scene_json_py(scene_path("Scene1"))
    objs.extend(first)
    for k in range(n_extra):
        x, y, z, r = _extra_sphere(k)
        objs.append(dict(type=oracle.OBJ_SPHERE, position=(x, y, z), radius=r, base=(.2 + .05 * (k % 13), .8, .3), specular_amount=0.25 * (k % 3),
                         smoothness=0.7))
    return oracle.make_objects(objs)


def _tracer(srt, sc, lib=None):
    pt = srt.PathTracer(W, H, lib=lib) if lib is not None else srt.PathTracer(W, H)
    pt.set_scene(C.cast(sc[0], C.POINTER(srt.Object)), sc[1])
    pt.set_camera(srt.default_camera())
    return pt


def _reference(oracle, n_extra, sc, **call):
    key = (n_extra,) + tuple(sorted(call.items()))
    if key not in _ORACLE:
        fb, acc, rays = oracle.render(sc[0], sc[1], oracle.default_environment(), oracle.default_camera(), W, H, threads=THREADS,
                                      accumulator=np.zeros((H, W, 4), np.float32), **call)
        fb.setflags(write=False), acc.setflags(write=False)
        _ORACLE[key] = (fb, acc, rays)
    return _ORACLE[key]


def _assert_same(fb, acc, ofb, oacc):
    assert np.array_equal(np.isnan(acc), np.isnan(oacc))
    bad = np.where(np.isnan(oacc), False, acc.view(np.uint32) != oacc.view(np.uint32))
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:8].tolist())
    assert np.array_equal(fb, ofb)


@pytest.fixture(scope="module")
def dev(srt):
    """libsrt_pathtrace_dev.so, built once (make dev) and opened next to the shipped library."""
    subprocess.run(["make", "-C", CSRC, "-s", "dev"], check=True, timeout=900)
    L = srt.capi.open_library(os.path.join(ROOT, "software-raytracer_amd", "libsrt_pathtrace_dev.so"))
    L.srt_debug_set_variant.argtypes = [C.c_void_p, C.c_int]
    return L


@pytest.mark.gpu
@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("side", ["fits", "over"])
def test_both_sides_of_the_threshold(srt, oracle, counts, side, spp):
    n = counts[side]
    sc = _objects(oracle, n)
    ref = _reference(oracle, n, sc, spp=spp, bounces=8, seed=5)
    pt = _tracer(srt, sc)
    pt.render(spp=spp, bounces=8, seed=5, count_rays=True)
    assert pt.stats().rays == ref[2]
    _assert_same(pt.framebuffer(), pt.accumulator(), ref[0], ref[1])
    # ... and without the ray count: the launch that is timed
    pt.render(spp=spp, bounces=8, seed=5)
    _assert_same(pt.framebuffer(), pt.accumulator(), ref[0], ref[1])
    pt.close()


@pytest.mark.gpu
@pytest.mark.parametrize("spp", SPPS)
def test_forced_five_waves_gives_the_same_bits(srt, oracle, counts, dev, spp):
    """on the fitting side: the development library as it chooses (six waves) and with variant 5 (five), both the oracle's bits"""
    n = counts["fits"]
    sc = _objects(oracle, n)
    ref = _reference(oracle, n, sc, spp=spp, bounces=8, seed=5)
    for variant in (0, 5):
        pt = _tracer(srt, sc, lib=dev)
        assert dev.srt_debug_set_variant(pt._h, variant) == 0
        pt.render(spp=spp, bounces=8, seed=5)
        _assert_same(pt.framebuffer(), pt.accumulator(), ref[0], ref[1])
        pt.close()


@pytest.mark.gpu
def test_counting_launch_keeps_its_steps(srt, oracle):
    """plain Scene1: the counting launch (five waves, the timed launch's grid and shape) takes the rows hand-out's pool steps —
    241 at 8 samples and 394 at 15, the figures tests/test_gpu_sample_rows.py pins — and gives the oracle's bits"""
    sc = _objects(oracle, 0)
    pt = _tracer(srt, sc)
    for spp, steps in ((8, 241), (15, 394)):
        pt.render(spp=spp, bounces=8, seed=5, count_rays=True, count_work=True)
        ref = _reference(oracle, 0, sc, spp=spp, bounces=8, seed=5)
        c = pt.work_counts().as_dict()
        assert c["valid"] == 1 and c["closest_hit_calls"] == c["pool_steps"] + c["waves"]
        assert c["pool_steps"] == steps
        assert pt.stats().rays == ref[2]
        _assert_same(pt.framebuffer(), pt.accumulator(), ref[0], ref[1])
    pt.close()


def test_six_wave_rule(rule_exe):
    """srt::rows_six_waves at its edge (the largest fitting size, one byte and one granule above), for requests that fill LDS, and
    for the LDS bytes of Scene1, Scene3 and Scene_indirect (tests/native/six_wave_rule_check.cpp, a stand-alone program under
    ASan + UBSan)"""
    r = subprocess.run([rule_exe] + [scene_path(n) for n in ("Scene1", "Scene3", "Scene_indirect")], capture_output=True, text=True)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1].startswith("ok "), r.stdout[-800:] + r.stderr[-2000:]
    assert lines[-1].split()[-1] == "26880"
    assert len(lines) == 4, lines


def test_threshold_scene(counts):
    """the sphere counts the GPU tests use come out of the rule (the `counts` fixture asserts what they must satisfy)"""
    assert counts["over"] == counts["fits"] + 1
