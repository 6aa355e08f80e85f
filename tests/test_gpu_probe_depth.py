"""Probe depth moments (srt_trace_probe_depth, ABI 7) on the MI355X.  Every comparison is bit for bit with no probe, direction,
texel or lane left out.  The pass is pinned from two sides: its DISTANCES output must be the clamp (rule 2) of what srt_trace_rays
writes to NORMAL_DEPTH.w for the explicit batch of P*K rays, and its MOMENTS must be the numpy reference
(tests/probe_depth_reference.py: the header's texel table, accumulation order and texel rule) applied to those distances."""
import ctypes as C

import numpy as np
import pytest

import light_probe_reference as LP
import probe_depth_reference as PD
from test_gpu_light_probes import explicit_rays
from test_gpu_radiance import Scene, differing, same
from test_gpu_visibility import memory_scene, mesh_scene, scene1

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = -7.0
# the camera's position; a point beside it; one under the floor (inside Scene1's ground sphere); one inside the mesh scene's box
# floor; one inside the mesh scene's small ball
PROBES = np.array([[0.0, 0.0, 0.0, 9.0], [0.7, 0.4, -1.5, -9.0], [0.5, -3.0, 4.0, 0.0], [0.3, -1.5, 5.2, 0.0], [1.6, -0.6, 4.2, 0.0]], dtype=F)
MAXD = 6.0  # nearer than the sky and than part of every scene: some rays are clamped, some are not
SCENES = {"scene1": scene1, "mesh": mesh_scene, "memory": memory_scene}


def traced_distances(pt, positions, directions, normalize=False):
    """NORMAL_DEPTH.w of srt_trace_rays for the explicit batch: (P, K) float32, +inf on a miss."""
    o, d = explicit_rays(positions, directions)
    pt.write_rays(o, d)
    pt.trace_rays(outputs=["normal_depth"], normalize=normalize)
    return pt.ray_output("normal_depth")[:, 3].reshape(positions.shape[0], directions.shape[0]).copy()


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


# ---- 1. the definition: every K, R and s on every instantiation -------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 63, 64, 65, 100, 256])
def test_distances_are_trace_rays_clamped_and_moments_are_the_reference(sc, srt, k):
    pt = sc.pt
    d = srt.light_probe_sphere(k)
    t = traced_distances(pt, PROBES, d)
    r = PD.clamp_distance(t, MAXD)
    print("%s K %d: t <= 0 at %d rays, clamped at %d, misses %d" % (sc.name, k, int((t <= 0).sum()), int((r >= F(MAXD)).sum()), int(np.isinf(t).sum())))
    if k >= 63:
        assert 0 < int((r >= F(MAXD)).sum()) < r.size  # the clamp decides something
        if sc.name == "scene1":
            assert (t[2] <= 0).any() and (r[2] == 0).any()  # the probe inside the ground sphere: negative distances give r = 0
    first = True
    for R in (4, 8, 16):
        for s in (0, 3, 6):
            pt.trace_probe_depth(PROBES if first else None, d if first else None, resolution=R, sharpness=s, max_distance=MAXD, distances=True, count_work=True)
            first = False
            got_r, got = pt.probe_depth_output("distances"), pt.probe_depth_output("moments")
            assert same(got_r, r), "K %d R %d s %d: %d distances differ from srt_trace_rays" % (k, R, s, int((got_r.view(np.uint32) != r.view(np.uint32)).sum()))
            want = PD.moments(d, r, R, s, MAXD)
            assert got.shape == (5, R * R, 4) and same(got, want), "K %d R %d s %d: %d texels differ from the reference" % (k, R, s, differing(got, want))
            work = pt.probe_depth_work()
            assert work["valid"] == 1 and work["waves"] > 0
            assert (work["probes"], work["rays"], work["far_rays"], work["wave_calls"]) == PD.work_formula(5, k, r, MAXD)
            if k == 1:  # rule 4's empty texel: one direction leaves the texels of the other hemisphere without weight
                empty = want[..., 2] == 0
                assert empty.any() and (~empty).any()
                assert (want[empty] == np.array([MAXD, MAXD * MAXD, 0.0, 1.0], F)).all()


def test_normalize_on_directions_that_are_not_unit(sc, srt):
    pt = sc.pt
    d = srt.light_probe_sphere(100)
    scale = np.random.default_rng(3).uniform(0.25, 7.0, 100).astype(F)
    d[:, :3] = (d[:, :3] * scale[:, None]).astype(F)
    t = traced_distances(pt, PROBES, d, normalize=True)
    r = PD.clamp_distance(t, MAXD)
    pt.trace_probe_depth(PROBES, d, resolution=8, sharpness=3, max_distance=MAXD, distances=True, normalize=True)
    assert same(pt.probe_depth_output("distances"), r)
    want = PD.moments(LP.normalized(d), r, 8, 3, MAXD)
    got = pt.probe_depth_output("moments")
    assert same(got, want), "%d texels differ" % differing(got, want)
    # without the flag the same directions give other moments: the weights are cos^8 of vectors that are not unit
    pt.trace_probe_depth(resolution=8, sharpness=3, max_distance=MAXD)
    assert not same(pt.probe_depth_output("moments"), want)


# ---- 2. more probes than the launch has waves ------------------------------------------------------------------------------------------------
def test_more_probes_than_waves(sc1, srt):
    pt = sc1.pt
    d = srt.light_probe_sphere(70)
    rng = np.random.RandomState(5)

    def positions(p):
        pos = np.zeros((p, 4), dtype=F)
        pos[:, :3] = (rng.rand(p, 3) * np.array([4.0, 2.0, 6.0]) + np.array([-2.0, -0.5, 0.0])).astype(F)
        return pos

    pos = positions(4500)
    pt.trace_probe_depth(pos, d, resolution=4, sharpness=2, max_distance=MAXD, distances=True, count_work=True)
    waves = pt.probe_depth_work()["waves"]
    if pos.shape[0] <= waves:  # a chip with more resident waves: as many probes as it takes
        pos = positions(waves + 9)
        pt.trace_probe_depth(pos, d, resolution=4, sharpness=2, max_distance=MAXD, distances=True, count_work=True)
        waves = pt.probe_depth_work()["waves"]
    assert pos.shape[0] > waves > 0
    got_r, got = pt.probe_depth_output("distances"), pt.probe_depth_output("moments")
    r = PD.clamp_distance(traced_distances(pt, pos, d), MAXD)
    assert same(got_r, r)
    want = PD.moments(d, r, 4, 2, MAXD)
    assert same(got, want), "%d texels differ" % differing(got, want)


# ---- 3. the same bits without the optional parts -------------------------------------------------------------------------------------------
def test_same_bits_without_distances_with_and_without_counting_and_into_bound_tensors(sc1, srt):
    import torch

    pt = sc1.pt
    d = srt.light_probe_sphere(100)
    kw = dict(resolution=16, sharpness=5, max_distance=MAXD)
    pt.trace_probe_depth(PROBES, d, distances=True, **kw)
    want, want_r = pt.probe_depth_output("moments"), pt.probe_depth_output("distances")
    for count_work in (False, True, False):
        pt.trace_probe_depth(PROBES, d, count_work=count_work, **kw)
        assert same(pt.probe_depth_output("moments"), want)
        with pytest.raises(srt.SrtError):
            pt.probe_depth_output("distances")  # the last trace did not write it
        if not count_work:
            with pytest.raises(srt.SrtError):
                pt.probe_depth_work()
        for _ in range(2):  # twice in a row, inputs as they stand
            pt.trace_probe_depth(count_work=count_work, **kw)
            assert same(pt.probe_depth_output("moments"), want)
    dev = "cuda:%d" % pt.device
    tm = torch.full((5 * 256 + 5, 4), SENTINEL, dtype=torch.float32, device=dev)
    tr = torch.full((500 + 7,), SENTINEL, dtype=torch.float32, device=dev)
    pt.bind_probe_depth_output("moments", tm)
    pt.bind_probe_depth_output("distances", tr)
    try:
        pt.trace_probe_depth(distances=True, **kw)
        pt.wait()
        gm, gr = tm.cpu().numpy(), tr.cpu().numpy()
        assert same(gm[:1280].reshape(5, 256, 4), want) and np.all(gm[1280:] == SENTINEL)
        assert same(gr[:500].reshape(5, 100), want_r) and np.all(gr[500:] == SENTINEL)
        assert same(pt.probe_depth_output("moments"), want) and same(pt.probe_depth_output("distances"), want_r)  # the read follows the binding
        # a smaller map leaves the rest of the bound tensor alone
        tm.fill_(SENTINEL)
        pt.trace_probe_depth(resolution=4, sharpness=5, max_distance=MAXD)
        pt.wait()
        gm = tm.cpu().numpy()
        assert same(gm[:80].reshape(5, 16, 4), PD.moments(d, want_r, 4, 5, MAXD)) and np.all(gm[80:] == SENTINEL)
        with pytest.raises(ValueError):
            pt.bind_probe_depth_output("moments", torch.zeros((100, 4), dtype=torch.float32, device=dev))
            pt.trace_probe_depth(**kw)
    finally:
        pt.wait()
        pt.bind_probe_depth_output("moments", None)
        pt.bind_probe_depth_output("distances", None)
    pt.trace_probe_depth(distances=True, **kw)
    assert same(pt.probe_depth_output("moments"), want) and same(pt.probe_depth_output("distances"), want_r)


# ---- 4. neighbours ---------------------------------------------------------------------------------------------------------------------------
def test_the_pass_leaves_the_ray_batch_the_light_probe_outputs_and_the_accumulator_alone(sc1, srt):
    pt = sc1.pt
    rng = np.random.default_rng(95)
    o = np.zeros((200, 4), F)
    o[:, :3] = rng.uniform((-5, -1, 0), (5, 4, 10), (200, 3))
    dd = np.full((200, 4), 4.0, F)
    v = rng.normal(size=(200, 3))
    dd[:, :3] = v / np.linalg.norm(v, axis=1, keepdims=True)
    pt.set_camera(srt.default_camera())
    pt.render(spp=4, bounces=2, seed=5)
    pt.write_rays(o, dd)
    pt.trace_rays()
    d = srt.light_probe_sphere(64)
    pt.trace_light_probes(PROBES, d, samples=2, bounces=2, seed=4, radiance=True, count_work=True)

    def state():
        return ([pt.accumulator(), pt.light_probe_coefficients(), pt.light_probe_radiance()] + [pt.ray_output(k) for k in srt.capi.RAY_OUTPUTS],
                pt.light_probe_work(), pt.framebuffer())

    before = state()
    pt.trace_probe_depth(resolution=16, sharpness=5, max_distance=MAXD, distances=True, count_work=True)
    pt.wait()
    after = state()
    assert all(a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(before[0], after[0]))
    assert before[1] == after[1] and np.array_equal(before[2], after[2])
    # the current rays are still the batch: tracing them again gives the same outputs
    pt.trace_rays()
    assert all(np.array_equal(pt.ray_output(k).view(np.uint32), b.view(np.uint32)) for k, b in zip(srt.capi.RAY_OUTPUTS, before[0][3:]))
    # and the depth outputs outlive a light-probe trace
    m = pt.probe_depth_output("moments")
    pt.trace_light_probes(samples=2, bounces=2, seed=4)
    assert same(pt.probe_depth_output("moments"), m)


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_are_found_in_the_header_s_order(srt, oracle):
    c = srt.capi
    oarr, n = oracle.make_objects(scene1(oracle)[0])
    pt = srt.PathTracer(24, 20)
    L = pt.L
    fptr = C.POINTER(C.c_float)
    nan, inf = float("nan"), float("inf")

    def call(**kw):
        p = c.ProbeDepthParams()
        assert L.srt_probe_depth_params_default(C.byref(p)) == c.OK
        for k, v in kw.items():
            setattr(p, k, v)
        return L.srt_trace_probe_depth(pt._h, C.byref(p))

    def why():
        return L.srt_last_error(pt._h)

    try:
        w = c.ProbeDepthWork()
        buf = np.empty((5, 256, 4), F)
        assert call(flags=4) == c.ERR_STATE and b"srt_set_scene" in why()  # before srt_set_scene, whatever the arguments
        pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
        # the arguments come before the inputs
        for kw in (dict(flags=4), dict(flags=0x80000000), dict(outputs=0), dict(outputs=4), dict(outputs=7), dict(resolution=0), dict(resolution=5),
                   dict(resolution=32), dict(sharpness=7), dict(max_distance=nan), dict(max_distance=inf), dict(max_distance=0.0), dict(max_distance=-1.0),
                   dict(reserved=1)):
            assert call(**kw) == c.ERR_INVALID_ARG, kw
        assert call() == c.ERR_STATE and b"positions" in why()
        assert L.srt_write_light_probes(pt._h, PROBES.ctypes.data_as(fptr), 5) == c.OK
        assert call() == c.ERR_STATE and b"directions" in why()
        assert call(reserved=1) == c.ERR_INVALID_ARG  # still before the inputs
        d = srt.light_probe_sphere(64)
        assert L.srt_write_light_probe_directions(pt._h, d.ctypes.data_as(fptr), 64) == c.OK
        # the sizes come last: bound arrays are not read by a refused call, so any non-null address will do
        assert L.srt_bind_light_probes(pt._h, 4096, (1 << 24) + 1) == c.OK
        assert call() == c.ERR_INVALID_ARG and b"directions exceeds" in why()
        assert L.srt_bind_light_probes(pt._h, 4096, (1 << 22) + 1) == c.OK  # P*K = 2^28 + 64, P*R*R = 2^30 + 256
        assert call() == c.ERR_INVALID_ARG and b"resolution^2" in why()
        assert call(resolution=3) == c.ERR_INVALID_ARG and b"4, 8 or 16" in why()
        assert L.srt_bind_light_probes(pt._h, None, 0) == c.OK
        assert L.srt_read_probe_depth_output(pt._h, c.PROBE_DEPTH_MOMENTS, buf.ctypes.data_as(C.c_void_p)) == c.ERR_STATE
        assert L.srt_get_probe_depth_work(pt._h, C.byref(w)) == c.ERR_STATE
        assert call(flags=c.PROBE_DEPTH_COUNT_WORK) == c.OK
        pt._probe_depth_traced = (5, 64, 16)
        good, work = pt.probe_depth_output("moments"), pt.probe_depth_work()
        assert work["rays"] == 320 and np.isfinite(good).all()
        # every refusal leaves the previous output and record readable
        for kw in (dict(flags=4), dict(outputs=0), dict(resolution=5), dict(sharpness=9), dict(max_distance=nan), dict(reserved=2)):
            assert call(**kw) == c.ERR_INVALID_ARG, kw
            assert same(pt.probe_depth_output("moments"), good) and pt.probe_depth_work() == work, kw
        assert L.srt_read_probe_depth_output(pt._h, c.PROBE_DEPTH_DISTANCES, buf.ctypes.data_as(C.c_void_p)) == c.ERR_STATE  # not written
        assert L.srt_read_probe_depth_output(pt._h, 3, buf.ctypes.data_as(C.c_void_p)) == c.ERR_INVALID_ARG
        assert L.srt_bind_probe_depth_output(pt._h, 3, None) == c.ERR_INVALID_ARG and L.srt_bind_probe_depth_output(pt._h, 0, None) == c.ERR_INVALID_ARG
        assert call() == c.OK and L.srt_get_probe_depth_work(pt._h, C.byref(w)) == c.ERR_STATE  # that call did not count
        assert L.srt_trace_probe_depth(pt._h, None) == c.ERR_INVALID_ARG and L.srt_get_probe_depth_work(pt._h, None) == c.ERR_INVALID_ARG
        assert L.srt_read_probe_depth_output(pt._h, c.PROBE_DEPTH_MOMENTS, None) == c.ERR_INVALID_ARG
        pt.wait()
    finally:
        pt.close()
