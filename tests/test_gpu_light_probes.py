"""Light probes (srt_trace_light_probes, ABI 7) on the MI355X.  Every comparison is bit for bit in all four lanes with no probe,
direction or lane left out (NaN compares as its bits).  The pass is pinned from two sides: its RADIANCE output must be what
srt_trace_radiance writes for the explicit batch of P*K rays (and, for camera directions, the accumulator of the CPU oracle and of
srt_render), and its COEFFICIENTS must be the numpy reference (tests/light_probe_reference.py: the header's basis, term and
tree-and-blocks sum) applied to that RADIANCE."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import light_probe_reference as R
from conftest import ROOT, scene_path
from test_gpu_radiance import SCENES, H, N, Scene, W, camera_rays, differing, moved_camera, same, srt_camera
from test_gpu_visibility import closed_room, scene1

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
F = np.float32
# the camera's position, a point beside it, and one under the floor (inside Scene1's ground sphere): every ray of that probe hits
PROBES = np.array([[0.0, 0.0, 0.0, 9.0], [0.7, 0.4, -1.5, -9.0], [0.5, -3.0, 4.0, 0.0]], dtype=F)


def explicit_rays(positions, directions):
    """The batch of P*K rays the definition names: ray p*K + k = (position_p, direction_k)."""
    P, K = positions.shape[0], directions.shape[0]
    return np.repeat(positions, K, axis=0).astype(F), np.tile(directions, (P, 1)).astype(F)


def radiance_of(pt, positions, directions, **kw):
    o, d = explicit_rays(positions, directions)
    pt.trace_radiance(o, d, **kw)
    return pt.radiance().reshape(positions.shape[0], directions.shape[0], 4)


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


# ---- 1. the oracle pin ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bounces", [(5, 0), (5, 1), (70, 8)])
def test_one_probe_at_the_camera_gives_the_accumulator_of_the_oracle_and_of_srt_render(sc, oracle, srt, n, bounces):
    ocam = oracle.default_camera()
    o, d = camera_rays(oracle, ocam)  # K = 480: 7 blocks of 64 and one of 32 lanes
    d[:, 3] = F(4.0 * np.pi / N)
    want, _ = sc.oracle_acc(ocam, n, bounces, 0)
    sc.pt.trace_light_probes(o[:1], d, samples=n, bounces=bounces, seed=0, radiance=True)
    got = sc.pt.light_probe_radiance()
    assert got.shape == (1, N, 4)
    assert same(got[0], want), "%d of %d rays differ from the oracle" % (differing(got[0], want), N)
    sc.pt.set_camera(srt_camera(srt, ocam))
    sc.pt.render(spp=n, bounces=bounces, seed=0)
    acc = sc.pt.accumulator().reshape(N, 4)
    assert same(got[0], acc), "%d of %d rays differ from srt_render" % (differing(got[0], acc), N)
    assert same(sc.pt.light_probe_coefficients(), R.project(got, d))


# ---- 2. the definition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [100, 64, 1, 65])
def test_radiance_is_trace_radiance_and_coefficients_are_the_reference(sc, srt, k):
    d = srt.light_probe_sphere(k)
    kw = dict(samples=70, bounces=8, seed=11, id_base=1000)
    want = radiance_of(sc.pt, PROBES, d, **kw)
    sc.pt.trace_light_probes(PROBES, d, radiance=True, **kw)
    got, coeff = sc.pt.light_probe_radiance(), sc.pt.light_probe_coefficients()
    assert same(got, want), "%d of %d rays differ from srt_trace_radiance" % (differing(got, want), 3 * k)
    ref = R.project(got, d)
    assert coeff.shape == (3, 9, 4) and same(coeff, ref), "%d of 27 coefficients differ from the reference" % differing(coeff, ref)
    assert np.isfinite(coeff).all()
    if sc.name != "empty" and k > 1:
        assert not same(coeff[0], coeff[2])  # (the probes see different things)


def test_a_probe_inside_the_closed_room(srt, oracle):
    """Every ray of every sample hits until the bounces run out: the pool runs full length for all 64 slots."""
    s = Scene(srt, oracle, closed_room(oracle))
    try:
        pos = np.array([[0.0, 0.0, 1.0, 0.0], [1.0, 0.5, 2.0, 0.0], [-1.0, 0.2, 3.0, 0.0]], dtype=F)
        d = srt.light_probe_sphere(100)
        kw = dict(samples=70, bounces=8, seed=11, id_base=1000)
        want = radiance_of(s.pt, pos, d, **kw)
        s.pt.trace_light_probes(pos, d, radiance=True, **kw)
        got = s.pt.light_probe_radiance()
        assert same(got, want) and same(s.pt.light_probe_coefficients(), R.project(got, d))
    finally:
        s.close()


# ---- 3. more units than the launch has waves ---------------------------------------------------------------------------------------------
def test_more_units_than_waves(sc1, srt):
    k, kw = 130, dict(samples=2, bounces=2, seed=3)
    d = srt.light_probe_sphere(k)
    rng = np.random.RandomState(5)

    def positions(p):
        pos = np.zeros((p, 4), dtype=F)
        pos[:, :3] = (rng.rand(p, 3) * np.array([4.0, 2.0, 6.0]) + np.array([-2.0, -0.5, 0.0])).astype(F)
        return pos

    pos = positions(1400)
    sc1.pt.trace_light_probes(pos, d, count_work=True, radiance=True, **kw)
    waves = sc1.pt.light_probe_work()["waves"]
    if 3 * pos.shape[0] <= waves:  # a chip with more resident waves: as many probes as it takes
        pos = positions(waves // 3 + 1)
        sc1.pt.trace_light_probes(pos, d, count_work=True, radiance=True, **kw)
        waves = sc1.pt.light_probe_work()["waves"]
    assert 3 * pos.shape[0] > waves > 0
    got, coeff = sc1.pt.light_probe_radiance(), sc1.pt.light_probe_coefficients()
    want = radiance_of(sc1.pt, pos, d, **kw)
    assert same(got, want), "%d rays differ" % differing(got, want)
    assert same(coeff, R.project(got, d))


# ---- 4. the same bits without the optional parts ---------------------------------------------------------------------------------------
def test_same_bits_without_radiance_with_and_without_counting_and_into_a_bound_tensor(sc1, srt):
    import torch

    pt = sc1.pt
    d = srt.light_probe_sphere(100)
    kw = dict(samples=9, bounces=4, seed=2, id_base=77)
    pt.trace_light_probes(PROBES, d, radiance=True, **kw)
    want = pt.light_probe_coefficients()
    assert same(want, R.project(pt.light_probe_radiance(), d))
    for count_work in (False, True, False):
        pt.trace_light_probes(PROBES, d, count_work=count_work, **kw)
        assert same(pt.light_probe_coefficients(), want)
        with pytest.raises(srt.SrtError):
            pt.light_probe_radiance()  # the last trace did not write it
        for _ in range(2):  # twice in a row, inputs as they stand
            pt.trace_light_probes(count_work=count_work, **kw)
            assert same(pt.light_probe_coefficients(), want)
    dev = "cuda:%d" % pt.device
    tc = torch.full((27 + 5, 4), -7.0, dtype=torch.float32, device=dev)
    tr = torch.full((300 + 5, 4), -7.0, dtype=torch.float32, device=dev)
    pt.bind_light_probe_output("coefficients", tc)
    pt.bind_light_probe_output("radiance", tr)
    try:
        pt.trace_light_probes(PROBES, d, radiance=True, **kw)
        assert same(pt.light_probe_coefficients(), want)
        hc, hr = tc.cpu().numpy(), tr.cpu().numpy()
        assert same(hc[:27].reshape(3, 9, 4), want) and (hc[27:] == -7.0).all() and (hr[300:] == -7.0).all()
        assert same(R.project(hr[:300].reshape(3, 100, 4), d), want)
        # device inputs: bound, not copied
        tp, td = torch.from_numpy(PROBES).to(dev), torch.from_numpy(d).to(dev)
        pt.trace_light_probes(tp, td, **kw)
        assert same(pt.light_probe_coefficients(), want)
        pt.bind_light_probe_output("coefficients", torch.zeros((26, 4), dtype=torch.float32, device=dev))
        with pytest.raises(ValueError):
            pt.trace_light_probes(**kw)
    finally:
        pt.bind_light_probe_output("coefficients", None)
        pt.bind_light_probe_output("radiance", None)
    pt.trace_light_probes(PROBES, d, **kw)  # the own buffers and arrays again
    assert same(pt.light_probe_coefficients(), want)


# ---- 5. splitting ----------------------------------------------------------------------------------------------------------------------
def test_probes_split_off_with_a_raised_id_base_give_the_bits_of_the_whole(sc1, srt):
    k = 100
    d = srt.light_probe_sphere(k)
    kw = dict(samples=7, bounces=8, seed=2)
    sc1.pt.trace_light_probes(PROBES, d, radiance=True, id_base=500, **kw)
    whole_c, whole_r = sc1.pt.light_probe_coefficients(), sc1.pt.light_probe_radiance()
    for a in (1, 2):
        sc1.pt.trace_light_probes(PROBES[a:], d, radiance=True, id_base=500 + a * k, **kw)
        assert same(sc1.pt.light_probe_coefficients(), whole_c[a:]) and same(sc1.pt.light_probe_radiance(), whole_r[a:])
    sc1.pt.trace_light_probes(PROBES[1:], d, radiance=True, id_base=500, **kw)  # (without the raise the streams are others)
    assert not same(sc1.pt.light_probe_radiance(), whole_r[1:])


# ---- 6. continuation -------------------------------------------------------------------------------------------------------------------
def test_continuing_without_reset_equals_one_call_and_needs_its_radiance(sc1, srt):
    pt, c = sc1.pt, srt.capi
    d = srt.light_probe_sphere(100)
    kw = dict(bounces=8, seed=5, id_base=3)
    pt.trace_light_probes(PROBES, d, samples=9, radiance=True, **kw)
    whole_c, whole_r = pt.light_probe_coefficients(), pt.light_probe_radiance()
    pt.trace_light_probes(samples=3, first_sample=1, radiance=True, **kw)
    first = pt.light_probe_radiance()
    pt.trace_light_probes(samples=6, first_sample=4, reset=False, radiance=True, **kw)
    assert same(pt.light_probe_radiance(), whole_r) and same(pt.light_probe_coefficients(), whole_c) and not same(first, whole_r)
    assert same(whole_r, radiance_of(pt, PROBES, d, samples=9, **kw))

    def state_error(**more):
        with pytest.raises(srt.SrtError) as e:
            pt.trace_light_probes(samples=6, first_sample=4, reset=False, **dict(kw, **more))
        assert e.value.args[0].startswith("srt error %d:" % c.ERR_STATE), e.value
        assert same(pt.light_probe_coefficients(), whole_c)  # nothing was touched

    state_error()  # without the RADIANCE output
    pt.trace_light_probes(PROBES[:2], d, samples=3, radiance=True, **kw)
    pt.trace_light_probes(samples=6, first_sample=4, reset=False, radiance=True, **kw)  # (P = 2 continues P = 2)
    part = pt.light_probe_coefficients()
    assert same(part, whole_c[:2])
    whole_c = part
    state_error(radiance=True, positions=PROBES)              # P changed
    state_error(radiance=True, positions=PROBES[:2], directions=srt.light_probe_sphere(99))  # K changed
    import torch

    t = torch.zeros((200, 4), dtype=torch.float32, device="cuda:%d" % pt.device)
    pt.bind_light_probe_output("radiance", t)
    try:
        state_error(radiance=True, directions=d)  # the same P and K, but another buffer is bound now
    finally:
        pt.bind_light_probe_output("radiance", None)


# ---- 7. NORMALIZE ----------------------------------------------------------------------------------------------------------------------
def test_normalize_equals_the_prenormalised_set_and_leaves_the_weights_alone(sc1, srt):
    d = srt.light_probe_sphere(100)
    scaled = d.copy()
    scaled[:, :3] = (d[:, :3] * F(3.0)).astype(F)
    scaled[:, 3] = (np.arange(100) % 7 + 1).astype(F) * F(0.125)
    pre = R.normalized(scaled)
    assert np.array_equal(pre[:, 3], scaled[:, 3])
    kw = dict(samples=6, bounces=8, seed=1, radiance=True)
    sc1.pt.trace_light_probes(PROBES, pre, **kw)
    want_c, want_r = sc1.pt.light_probe_coefficients(), sc1.pt.light_probe_radiance()
    sc1.pt.trace_light_probes(PROBES, scaled, normalize=True, **kw)
    assert same(sc1.pt.light_probe_radiance(), want_r) and same(sc1.pt.light_probe_coefficients(), want_c)
    assert same(want_c, R.project(want_r, pre))
    sc1.pt.trace_light_probes(PROBES, scaled, **kw)  # (without the flag the basis sees the scaled directions)
    assert not same(sc1.pt.light_probe_coefficients(), want_c)


# ---- 8. work counts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n,bounces", [(100, 5, 4), (64, 3, 0), (130, 2, 2)])
def test_work_counts(sc1, srt, k, n, bounces):
    d = srt.light_probe_sphere(k)
    kw = dict(samples=n, bounces=bounces, seed=4)
    o, dd = explicit_rays(PROBES, d)
    sc1.pt.trace_radiance(o, dd, count_work=True, **kw)
    rw = sc1.pt.radiance_work()
    sc1.pt.trace_light_probes(PROBES, d, count_work=True, **kw)
    w = sc1.pt.light_probe_work()
    j = (k + 63) // 64
    assert w["valid"] == 1 and w["probes"] == 3 and w["rays"] == 3 * k and w["samples"] == 3 * k * n
    assert w["closest_calls"] == rw["closest_calls"]
    assert w["wave_calls"] >= 3 * j and w["waves"] >= 1 and w["waves"] % 4 == 0
    if bounces == 0:
        assert w["wave_calls"] == 3 * j
    sc1.pt.trace_light_probes(**kw)
    with pytest.raises(srt.SrtError):
        sc1.pt.light_probe_work()  # the last trace did not count


# ---- 9. what the call leaves alone -----------------------------------------------------------------------------------------------------
def test_a_probe_trace_leaves_the_other_outputs_alone(sc1, oracle, srt):
    pt = sc1.pt
    ocam = oracle.default_camera()
    o, d = camera_rays(oracle, ocam)
    pt.set_camera(srt_camera(srt, ocam))
    pt.render(spp=3, bounces=4, seed=9)
    pt.render_gbuffer()
    pt.write_rays(o, d)
    pt.trace_rays()
    pt.trace_radiance(samples=4, bounces=3, seed=6)
    st = srt.capi.Stats()
    assert pt.L.srt_get_stats(pt._h, C.byref(st)) == 0

    def snapshot(stats):
        return dict(fb=pt.framebuffer(), acc=pt.accumulator(), rad=pt.radiance(), stats=bytes(stats), **{"g_" + k: pt.gbuffer(k) for k in srt.capi.GBUFFERS},
                    **{"r_" + k: pt.ray_output(k) for k in srt.capi.RAY_OUTPUTS})

    before = snapshot(st)
    pt.trace_light_probes(PROBES, 100, samples=5, bounces=8, seed=4, count_work=True, radiance=True)
    got = pt.light_probe_radiance()
    st2 = srt.capi.Stats()
    assert pt.L.srt_get_stats(pt._h, C.byref(st2)) == 0
    after = snapshot(st2)
    for k in before:
        a, b = before[k], after[k]
        assert (a == b) if isinstance(a, bytes) else np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
    # the current rays are still the camera's: a radiance trace of them continues to work, and the probes' result was right
    pt.trace_radiance(samples=4, bounces=3, seed=6)
    assert same(pt.radiance(), before["rad"])
    assert same(got, radiance_of(pt, PROBES, srt.light_probe_sphere(100), samples=5, bounces=8, seed=4))


# ---- 10. errors ------------------------------------------------------------------------------------------------------------------------
def test_refusals(srt, oracle):
    c = srt.capi
    pt = srt.PathTracer(W, H)
    L = pt.L
    fptr = C.POINTER(C.c_float)
    try:
        def rc(**kw):
            p = c.LightProbeParams()
            L.srt_light_probe_params_default(C.byref(p))
            for k, v in kw.items():
                setattr(p, k, v)
            return L.srt_trace_light_probes(pt._h, C.byref(p))

        out = np.zeros((2, 9, 4), F)
        w = c.LightProbeWork()
        d = srt.light_probe_sphere(5)
        assert rc() == c.ERR_STATE  # before srt_set_scene
        assert L.srt_read_light_probe_output(pt._h, 1, out.ctypes.data) == c.ERR_STATE and L.srt_get_light_probe_work(pt._h, C.byref(w)) == c.ERR_STATE
        oarr, n = oracle.make_objects(scene1(oracle)[0])
        pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
        assert rc() == c.ERR_STATE  # no positions
        assert rc(flags=8) == c.ERR_INVALID_ARG  # (the arguments before the inputs)
        assert L.srt_write_light_probes(pt._h, PROBES.ctypes.data_as(fptr), 2) == c.OK
        assert rc() == c.ERR_STATE  # no directions
        # the limits of the inputs, at the write and at the bind
        assert L.srt_write_light_probes(pt._h, PROBES.ctypes.data_as(fptr), 0) == c.ERR_INVALID_ARG
        assert L.srt_write_light_probe_directions(pt._h, d.ctypes.data_as(fptr), 0) == c.ERR_INVALID_ARG
        assert L.srt_write_light_probe_directions(pt._h, d.ctypes.data_as(fptr), 4097) == c.ERR_INVALID_ARG
        assert L.srt_bind_light_probe_directions(pt._h, 4096, 4097) == c.ERR_INVALID_ARG and L.srt_bind_light_probe_directions(pt._h, None, 3) == c.ERR_INVALID_ARG
        assert L.srt_bind_light_probes(pt._h, 4096, (1 << 30) + 1) == c.ERR_INVALID_ARG
        assert L.srt_bind_light_probe_output(pt._h, 3, None) == c.ERR_INVALID_ARG and L.srt_bind_light_probe_output(pt._h, 0, None) == c.ERR_INVALID_ARG
        assert rc() == c.ERR_STATE  # (the refused calls left no directions)
        assert L.srt_write_light_probe_directions(pt._h, d.ctypes.data_as(fptr), 5) == c.OK
        assert rc() == c.OK and L.srt_read_light_probe_output(pt._h, 1, out.ctypes.data) == c.OK
        good = out.copy()
        probe = np.zeros_like(out)
        for kw in (dict(flags=8), dict(flags=0x80000001), dict(outputs=0), dict(outputs=4), dict(outputs=7), dict(first_sample=0), dict(sample_count=0),
                   dict(sample_count=4097), dict(max_bounces=-1), dict(first_sample=0xFFFFFFFF, sample_count=2), dict(reserved=1)):
            assert rc(**kw) == c.ERR_INVALID_ARG, kw
            assert L.srt_read_light_probe_output(pt._h, 1, probe.ctypes.data) == c.OK and same(probe, good), kw  # the previous output is intact
        # P*K > 2^30: a bound position count (never dereferenced: the call is refused before anything is touched)
        import torch

        t = torch.zeros((4, 4), dtype=torch.float32, device="cuda:%d" % pt.device)
        assert L.srt_bind_light_probes(pt._h, t.data_ptr(), (1 << 30) // 5 + 1) == c.OK
        assert rc() == c.ERR_INVALID_ARG
        assert L.srt_bind_light_probes(pt._h, None, 0) == c.OK
        assert L.srt_read_light_probe_output(pt._h, 1, probe.ctypes.data) == c.OK and same(probe, good)
        # RESET: without it the call needs the RADIANCE output and a previous trace into it
        assert rc(flags=0) == c.ERR_STATE and rc(flags=0, outputs=3) == c.ERR_STATE
        assert L.srt_read_light_probe_output(pt._h, 2, probe.ctypes.data) == c.ERR_STATE  # the last trace wrote no RADIANCE
        assert L.srt_read_light_probe_output(pt._h, 3, probe.ctypes.data) == c.ERR_INVALID_ARG
        assert rc(outputs=3) == c.OK and rc(flags=0, outputs=3, first_sample=17) == c.OK and rc(flags=0, outputs=2, first_sample=33) == c.OK
        assert L.srt_read_light_probe_output(pt._h, 1, probe.ctypes.data) == c.ERR_STATE  # that trace wrote no COEFFICIENTS
        assert L.srt_get_light_probe_work(pt._h, C.byref(w)) == c.ERR_STATE  # the last trace did not count
        assert rc(flags=c.LIGHT_PROBE_RESET | c.LIGHT_PROBE_COUNT_WORK) == c.OK and L.srt_get_light_probe_work(pt._h, C.byref(w)) == c.OK
        assert (w.valid, w.probes, w.rays, w.samples) == (1, 2, 10, 160)
        assert rc(first_sample=0xFFFFFFFF, sample_count=1) == c.OK
    finally:
        pt.close()


# ---- 11. the command line --------------------------------------------------------------------------------------------------------------
def test_the_cli_writes_the_bytes_the_python_call_returns(srt, oracle, tmp_path):
    pos = PROBES[:2]
    (tmp_path / "in.f32").write_bytes(pos.tobytes())
    out, rad = tmp_path / "out.bin", tmp_path / "rad.bin"
    r = subprocess.run([CLI, "--scene", scene_path("Scene1"), "--probes", str(tmp_path / "in.f32"), "--probe-directions", "64", "--probes-out", str(out),
                        "--probe-radiance-out", str(rad), "--radiance", "6", "--bounces", "3", "--seed", "13"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    s = Scene(srt, oracle, scene1(oracle))
    try:
        s.pt.trace_light_probes(pos, 64, samples=6, bounces=3, seed=13, radiance=True)
        want_c, want_r = s.pt.light_probe_coefficients(), s.pt.light_probe_radiance()
    finally:
        s.close()
    assert same(want_c, R.project(want_r, srt.light_probe_sphere(64)))
    assert out.read_bytes() == want_c.tobytes() and rad.read_bytes() == want_r.tobytes()
    # directions from a file: the same set written out
    (tmp_path / "dirs.f32").write_bytes(srt.light_probe_sphere(64).tobytes())
    out2 = tmp_path / "out2.bin"
    r = subprocess.run([CLI, "--scene", scene_path("Scene1"), "--probes", str(tmp_path / "in.f32"), "--probe-directions", str(tmp_path / "dirs.f32"),
                        "--probes-out", str(out2), "--radiance", "6", "--bounces", "3", "--seed", "13"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and out2.read_bytes() == want_c.tobytes(), r.stderr
    # host.py over the C++ host's PathTraceRenderer::traceLightProbes
    hr = srt.host.Renderer(32, 24)
    try:
        hr.set_scene(srt.host.Scene(scene_path("Scene1")))
        via_host = hr.trace_light_probes(pos, 64, samples=6, bounces=3, seed=13, count_work=True, radiance=True)
        assert hr.light_probe_work()["samples"] == 2 * 64 * 6
        assert hr.light_probe_radiance().tobytes() == want_r.tobytes() and hr.light_probe_coefficients().tobytes() == want_c.tobytes()
    finally:
        hr.close()
    assert via_host.tobytes() == want_c.tobytes()
