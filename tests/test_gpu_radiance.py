"""Radiance queries (srt_trace_radiance, ABI 7) on the MI355X.  Every comparison is bit for bit in all four lanes with no ray left
out (NaN compares as its bits).  The feature is pinned by its equivalence guarantee: a batch of camera rays — camera.position and
the oracle's GetRayDirection for every pixel, in the order i = x + y * W — must give the accumulator of the CPU oracle
(POW_SHARED) and of srt_render.  24 x 20 rays make 7 full blocks of 64 and one of 32 lanes; 70 samples make a slot cross the
kernel's chunk of 64 samples."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path
from test_gpu_visibility import closed_room, memory_scene, mesh_scene, scene1

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
W, H = 24, 20
N = W * H


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def reflection_scene(oracle):
    return oracle.load_scene_json_py(scene_path("Scene1_reflection")), None


def empty_scene(oracle):
    return [], None


def moved_camera(oracle):
    """Moved, and turned about the world's up axis (sine 0.6, cosine 0.8)."""
    cam = oracle.default_camera()
    c, s = np.float32(0.8), np.float32(0.6)
    cam.position[:] = (0.7, 0.4, -1.5)
    cam.right[:] = (float(c), 0.0, float(-s))
    cam.up[:] = (0.0, 1.0, 0.0)
    cam.forward[:] = (float(s), 0.0, float(c))
    return cam


def srt_camera(srt, ocam):
    cam = srt.default_camera()
    cam.position[:], cam.right[:], cam.up[:], cam.forward[:] = ocam.position[:], ocam.right[:], ocam.up[:], ocam.forward[:]
    cam.fov_degrees = ocam.fov_degrees
    return cam


def camera_rays(oracle, ocam, w=W, h=H):
    """(origins, directions), (w * h, 4) float32 each, ray i = x + y * w: camera.position and GetRayDirection(camera, x, y)."""
    o = np.zeros((w * h, 4), np.float32)
    d = np.zeros((w * h, 4), np.float32)
    o[:, :3] = np.array(ocam.position[:], np.float32)
    out = (C.c_float * 3)()
    for y in range(h):
        for x in range(w):
            oracle.lib().srt_oracle_ray_direction(C.byref(ocam), w, h, x, y, out)
            d[x + y * w, :3] = out[:]
    d[:, 3] = 7.0  # (ignored: there is no t_max)
    return o, d


def same(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def differing(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).any(axis=-1).sum())


class Scene:
    """A tracer with a scene, and what the oracle needs to render the same scene."""

    def __init__(self, srt, oracle, scene, w=W, h=H):
        objs, meshes = scene
        self.srt, self.oracle, self.w, self.h = srt, oracle, w, h
        self.oarr, self.n = oracle.make_objects(objs)
        self.pt = srt.PathTracer(w, h)
        self.om = None
        if meshes:
            marr, mn, keep = oracle.make_meshes(meshes)
            self.pt.set_meshes(C.cast(marr, C.POINTER(srt.Mesh)), mn)
            self.om = (marr, mn, keep)
        self.pt.set_scene(C.cast(self.oarr, C.POINTER(srt.Object)), self.n)
        self.env = oracle.default_environment()

    def oracle_acc(self, ocam, spp, bounces, seed=0, w=None, h=None, **kw):
        """(accumulator as (w * h, 4), rays) of the oracle for the frame of `ocam`."""
        w, h = w or self.w, h or self.h
        _, acc, rays = self.oracle.render(self.oarr, self.n, self.env, ocam, w, h, spp=spp, bounces=bounces, seed=seed,
                                          pow_mode=self.oracle.POW_SHARED, meshes=self.om[:2] if self.om else None, **kw)
        return acc.reshape(w * h, 4), rays

    def close(self):
        self.pt.close()


SCENES = {"scene1": scene1, "reflection": reflection_scene, "memory": memory_scene, "mesh": mesh_scene, "empty": empty_scene}


@pytest.fixture(scope="module", params=list(SCENES))
def sc(request, srt, oracle):
    s = Scene(srt, oracle, SCENES[request.param](oracle))
    s.name = request.param
    yield s
    s.close()


@pytest.fixture(scope="module")
def sc1(srt, oracle):
    s = Scene(srt, oracle, scene1(oracle))
    yield s
    s.close()


# ---- 1. camera-ray equivalence ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bounces", [(5, 0), (5, 1), (70, 8)])
def test_camera_rays_give_the_accumulator_of_the_oracle_and_of_srt_render(sc, oracle, srt, n, bounces):
    for ocam, seed in ((oracle.default_camera(), 0), (moved_camera(oracle), 11)):
        want, rays = sc.oracle_acc(ocam, n, bounces, seed)
        o, d = camera_rays(oracle, ocam)
        sc.pt.trace_radiance(o, d, samples=n, bounces=bounces, seed=seed, count_work=True)
        got, work = sc.pt.radiance(), sc.pt.radiance_work()
        print("%s n=%d B=%d seed=%d: oracle rays %d, work %s, NaN alphas %d" % (sc.name, n, bounces, seed, rays, work, int(np.isnan(want[:, 3]).sum())))
        assert same(got, want), "%d of %d rays differ from the oracle" % (differing(got, want), N)
        sc.pt.set_camera(srt_camera(srt, ocam))
        sc.pt.render(spp=n, bounces=bounces, seed=seed)
        acc = sc.pt.accumulator().reshape(N, 4)
        assert same(got, acc), "%d of %d rays differ from srt_render" % (differing(got, acc), N)
        assert work["valid"] == 1 and work["rays"] == N and work["samples"] == N * n
        assert work["closest_calls"] == rays
        assert 64 * work["wave_calls"] >= work["closest_calls"] - work["samples"]
        assert work["wave_calls"] >= 8  # one primary invocation per block of 64 rays
        if sc.name == "empty" or bounces == 0:
            assert work["wave_calls"] == 8 and work["closest_calls"] == N * n  # every sample ends at the shared primary
        # without the work record: the same bits, and again
        for _ in range(2):
            sc.pt.trace_radiance(samples=n, bounces=bounces, seed=seed)
            assert same(sc.pt.radiance(), want)


def test_the_empty_scene_costs_one_invocation_per_block(srt, oracle):
    s = Scene(srt, oracle, empty_scene(oracle))
    try:
        o, d = camera_rays(oracle, oracle.default_camera())
        s.pt.trace_radiance(o, d, samples=5, bounces=8, count_work=True)
        want, rays = s.oracle_acc(oracle.default_camera(), 5, 8)
        assert same(s.pt.radiance(), want)
        work = s.pt.radiance_work()
        assert work["wave_calls"] == 8 and work["closest_calls"] == rays == N * 5 and work["samples"] == N * 5
    finally:
        s.close()


# ---- 2. mixed origins ---------------------------------------------------------------------------------------------------------------
def test_a_batch_of_two_cameras_rays_equals_the_two_oracle_accumulators_on_their_halves(sc1, oracle):
    cam_a, cam_b = oracle.default_camera(), moved_camera(oracle)
    (oa, da), (ob, db) = camera_rays(oracle, cam_a), camera_rays(oracle, cam_b)
    half = 10 * W  # scene rows 0-9 of A's frame, then rows 10-19 of B's
    o, d = np.concatenate([oa[:half], ob[half:]]), np.concatenate([da[:half], db[half:]])
    wa, _ = sc1.oracle_acc(cam_a, 12, 4, seed=3)
    wb, _ = sc1.oracle_acc(cam_b, 12, 4, seed=3)
    sc1.pt.trace_radiance(o, d, samples=12, bounces=4, seed=3)
    got = sc1.pt.radiance()
    assert same(got[:half], wa[:half]) and same(got[half:], wb[half:])
    assert not same(got[half:], wa[half:])  # (the two cameras see different things)


# ---- 3. continuation ----------------------------------------------------------------------------------------------------------------
def test_continuing_without_reset_equals_one_call(sc1, oracle):
    ocam = moved_camera(oracle)
    o, d = camera_rays(oracle, ocam)
    want, _ = sc1.oracle_acc(ocam, 9, 8, seed=5)
    sc1.pt.trace_radiance(o, d, samples=9, bounces=8, seed=5)
    whole = sc1.pt.radiance()
    assert same(whole, want)
    sc1.pt.trace_radiance(samples=3, bounces=8, seed=5, first_sample=1, reset=True)
    first = sc1.pt.radiance()
    sc1.pt.trace_radiance(samples=6, bounces=8, seed=5, first_sample=4, reset=False)
    assert same(sc1.pt.radiance(), whole) and not same(first, whole)
    # the oracle continues the same way
    w3, _ = sc1.oracle_acc(ocam, 3, 8, seed=5)
    assert same(first, w3)
    w9, _ = sc1.oracle_acc(ocam, 6, 8, seed=5, first_sample=4, reset=False, accumulator=w3.reshape(H, W, 4))
    assert same(whole, w9)


# ---- 4. splitting -------------------------------------------------------------------------------------------------------------------
def test_a_split_batch_with_id_base_gives_the_bits_of_the_whole(sc1, oracle):
    ocam = oracle.default_camera()
    o, d = camera_rays(oracle, ocam)
    want, _ = sc1.oracle_acc(ocam, 7, 8, seed=2)
    sc1.pt.trace_radiance(o, d, samples=7, bounces=8, seed=2)
    assert same(sc1.pt.radiance(), want)
    parts = []
    for a, b in ((0, 200), (200, N)):
        sc1.pt.trace_radiance(o[a:b], d[a:b], samples=7, bounces=8, seed=2, id_base=a)
        parts.append(sc1.pt.radiance())
        assert parts[-1].shape == (b - a, 4)
    assert same(np.concatenate(parts), want)
    sc1.pt.trace_radiance(o[200:], d[200:], samples=7, bounces=8, seed=2)  # (without id_base the streams are others)
    assert not same(sc1.pt.radiance(), want[200:])


# ---- 5. packing ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounces", [8, 4, 1])
def test_one_ray_of_64_samples_fills_the_wave(srt, oracle, bounces):
    """The ray of pixel (4, 4) of an 8 x 8 frame in the closed room: every path runs its full length, so a perfectly packed wave
    needs 1 + B invocations for the 64 samples; one lane per ray would need 1 + 64 * B."""
    s = Scene(srt, oracle, closed_room(oracle), 8, 8)
    try:
        ocam = oracle.default_camera()
        # the precondition, from the oracle: scene row 4 is memory row 8 - 1 - 4
        want, rays = s.oracle_acc(ocam, 64, bounces, rows=(3, 4), cols=(4, 5))
        assert rays == 64 * (1 + bounces)
        o, d = camera_rays(oracle, ocam, 8, 8)
        i = 4 + 4 * 8
        s.pt.trace_radiance(o[i:i + 1], d[i:i + 1], samples=64, bounces=bounces, seed=0, id_base=36, count_work=True)
        got, work = s.pt.radiance(), s.pt.radiance_work()
        print("B=%d: %s" % (bounces, work))
        assert same(got, want[i:i + 1])
        assert work["rays"] == 1 and work["samples"] == 64 and work["closest_calls"] == 64 * (1 + bounces)
        assert work["wave_calls"] <= 1 + 2 * bounces
    finally:
        s.close()


# ---- 6. binding ---------------------------------------------------------------------------------------------------------------------
def test_a_bound_tensor_keeps_its_sentinel_and_normalize_normalizes(sc1, oracle):
    import torch

    ocam = oracle.default_camera()
    o, d = camera_rays(oracle, ocam)
    want, _ = sc1.oracle_acc(ocam, 6, 8, seed=1)
    t = torch.full((N + 64, 4), -7.0, dtype=torch.float32, device="cuda:%d" % sc1.pt.device)
    sc1.pt.bind_radiance(t)
    try:
        sc1.pt.trace_radiance(o, d, samples=6, bounces=8, seed=1)
        got = sc1.pt.radiance()
        host = t.cpu().numpy()
        assert same(got, want) and same(host[:N], want) and (host[N:] == -7.0).all()
        # directions scaled by 3 (exact) and SRT_RADIANCE_NORMALIZE, against the normalized directions as they stand
        dn = d.copy()
        dn[:, :3] = (d[:, :3] * np.float32(3.0)).astype(np.float32)
        x = dn[:, :3]
        length = np.sqrt(((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]).astype(np.float32) + x[:, 2] * x[:, 2]).astype(np.float32)).astype(np.float32)
        pre = dn.copy()
        pre[:, :3] = (x / length[:, None]).astype(np.float32)
        sc1.pt.trace_radiance(o, pre, samples=6, bounces=8, seed=1)
        ref = sc1.pt.radiance()
        sc1.pt.trace_radiance(o, dn, samples=6, bounces=8, seed=1, normalize=True)
        assert same(sc1.pt.radiance(), ref) and (t.cpu().numpy()[N:] == -7.0).all()
        small = torch.zeros((N - 1, 4), dtype=torch.float32, device=t.device)
        sc1.pt.bind_radiance(small)
        with pytest.raises(ValueError):
            sc1.pt.trace_radiance(samples=6, bounces=8)
    finally:
        sc1.pt.bind_radiance(None)
    sc1.pt.trace_radiance(o, d, samples=6, bounces=8, seed=1)  # the own buffer again
    assert same(sc1.pt.radiance(), want)


# ---- 7. side effects, errors --------------------------------------------------------------------------------------------------------
def test_a_radiance_trace_leaves_the_other_outputs_alone(sc1, oracle, srt):
    pt = sc1.pt
    ocam = oracle.default_camera()
    o, d = camera_rays(oracle, ocam)
    pt.set_camera(srt_camera(srt, ocam))
    pt.render(spp=3, bounces=4, seed=9)
    pt.render_gbuffer()
    pt.write_rays(o, d)
    pt.trace_rays()
    L = pt.L
    st = srt.capi.Stats()
    assert L.srt_get_stats(pt._h, C.byref(st)) == 0
    before = dict(fb=pt.framebuffer(), acc=pt.accumulator(), stats=bytes(st), **{"g_" + k: pt.gbuffer(k) for k in srt.capi.GBUFFERS},
                  **{"r_" + k: pt.ray_output(k) for k in srt.capi.RAY_OUTPUTS})
    pt.trace_radiance(samples=5, bounces=8, seed=4, count_work=True)
    rad = pt.radiance()
    st2 = srt.capi.Stats()
    assert L.srt_get_stats(pt._h, C.byref(st2)) == 0
    after = dict(fb=pt.framebuffer(), acc=pt.accumulator(), stats=bytes(st2), **{"g_" + k: pt.gbuffer(k) for k in srt.capi.GBUFFERS},
                 **{"r_" + k: pt.ray_output(k) for k in srt.capi.RAY_OUTPUTS})
    for k in before:
        a, b = before[k], after[k]
        assert (a == b) if isinstance(a, bytes) else np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
    want, _ = sc1.oracle_acc(ocam, 5, 8, seed=4)
    assert same(rad, want)


def test_refusals(srt, oracle):
    c = srt.capi
    pt = srt.PathTracer(W, H)
    try:
        def rc(**kw):
            p = c.RadianceParams()
            pt.L.srt_radiance_params_default(C.byref(p))
            for k, v in kw.items():
                setattr(p, k, v)
            return pt.L.srt_trace_radiance(pt._h, C.byref(p))

        out = np.zeros((4, 4), np.float32)
        fp = out.ctypes.data_as(C.POINTER(C.c_float))
        w = c.RadianceWork()
        assert rc() == c.ERR_STATE  # before srt_set_scene
        assert pt.L.srt_read_radiance(pt._h, fp) == c.ERR_STATE and pt.L.srt_get_radiance_work(pt._h, C.byref(w)) == c.ERR_STATE
        oarr, n = oracle.make_objects(scene1(oracle)[0])
        pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
        assert rc() == c.ERR_STATE  # no rays
        assert rc(flags=8) == c.ERR_INVALID_ARG  # (the arguments before the rays)
        o, d = camera_rays(oracle, oracle.default_camera(), 2, 2)
        pt.write_rays(o, d)
        for kw in (dict(flags=8), dict(first_sample=0), dict(sample_count=0), dict(sample_count=4097), dict(max_bounces=-1),
                   dict(first_sample=0xFFFFFFFF, sample_count=2)):
            assert rc(**kw) == c.ERR_INVALID_ARG, kw
        assert pt.L.srt_read_radiance(pt._h, fp) == c.ERR_STATE  # nothing was traced by the refused calls
        assert rc(first_sample=0xFFFFFFFF, sample_count=1, flags=0) == c.OK
        assert rc() == c.OK and pt.L.srt_read_radiance(pt._h, fp) == c.OK
        assert pt.L.srt_get_radiance_work(pt._h, C.byref(w)) == c.ERR_STATE  # the last trace did not count
        assert rc(flags=c.RADIANCE_RESET | c.RADIANCE_COUNT_WORK) == c.OK and pt.L.srt_get_radiance_work(pt._h, C.byref(w)) == c.OK
        assert (w.valid, w.rays, w.samples) == (1, 4, 64)
    finally:
        pt.close()


# ---- 8. the command line ------------------------------------------------------------------------------------------------------------
def test_the_cli_writes_the_bytes_trace_radiance_returns(srt, oracle, tmp_path):
    ocam = moved_camera(oracle)
    o, d = camera_rays(oracle, ocam)
    rec = np.concatenate([o, d], axis=1).astype(np.float32)
    (tmp_path / "in.f32").write_bytes(rec.tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([CLI, "--scene", scene_path("Scene1"), "--rays", str(tmp_path / "in.f32"), "--rays-out", str(out), "--radiance", "6",
                        "--bounces", "3", "--seed", "13"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    s = Scene(srt, oracle, scene1(oracle))
    try:
        s.pt.trace_radiance(o, d, samples=6, bounces=3, seed=13)
        want = s.pt.radiance()
        oracle_acc, _ = s.oracle_acc(ocam, 6, 3, seed=13)
    finally:
        s.close()
    assert same(want, oracle_acc)
    # host.py over the C++ host's PathTraceRenderer::traceRadiance
    r = srt.host.Renderer(32, 24)
    try:
        r.set_scene(srt.host.Scene(scene_path("Scene1")))
        via_host = r.trace_radiance(o, d, samples=6, bounces=3, seed=13, count_work=True)
        assert r.radiance_work()["samples"] == N * 6
    finally:
        r.close()
    assert via_host.tobytes() == want.tobytes()
    assert out.read_bytes() == want.tobytes()
