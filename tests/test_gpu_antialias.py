"""Geometry-supersampled anti-aliasing (srt_render_subsamples, srt_antialias) on the MI355X: the sub-sample first hits against
the oracle's closest hit along the oracle's own rays of the (2kW) x (2kH) virtual frame, exactly; the resolve against the
float64 restatement of include/srt_pathtrace.h (tests/antialias_reference.py) on synthetic inputs and on real frames; its exact
properties; quality against a supersampled ground truth; non-interference, flags, errors and the layers above."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from antialias_reference import resolve
from conftest import ROOT, scene_path

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
VIEWER = os.path.join(ROOT, "software-raytracer_amd", "srt_viewer")
# Derived, not measured: a pixel's result is fewer than 40 binary32 roundings of positive terms (9 taps x (weight, product, sum)
# for the worst sub-sample, its division, the sum over s and the division by K), each at most 2^-24 relative: below 2.4e-6.
# The bound leaves four times that.  No transcendental is involved.
# The kernel's maximum, measured on the MI355X: 2.7e-7 over test_resolve_matches_the_definition (1.2e-7, 1.9e-7 and 2.7e-7 for
# k = 2, 3, 4, either source: what a host transcription of the kernel gives), 5.6e-7 on the real frames of
# test_real_frames_match_the_definition and 4.0e-7 over the shapes of tests/test_gpu_pass_edges.py.
REL_TOL = 1e-5


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _rel_err(got, ref, mask):
    g, r = got[mask][:, :3].astype(np.float64), ref[mask][:, :3]
    return float(np.max(np.abs(g - r) / np.maximum(np.abs(r), 1e-6))) if g.size else 0.0


# ---- sub-samples against the oracle -------------------------------------------------------------------------------------------
SW, SH = 37, 21
BAND = (5, 14)  # memory rows


def _cameras(srt, oracle, case="Scene1", nan=False):
    """A moved and rotated camera (yaw 7 degrees, fov 49), once per library's ctypes class.  In Scene3 it stands behind the box
    that fills the view from the origin, among the spheres."""
    a = np.deg2rad(7.0)
    c, s = float(np.cos(a)), float(np.sin(a))
    fields = dict(position=(0.3, -0.2, 2.4 if case == "Scene3" else 0.4), right=(c, 0.0, -s), up=(0.0, 1.0, 0.0), forward=(float("nan") if nan else s, 0.0, c))
    cams = []
    for mod in (srt, oracle):
        cam = mod.Camera()
        for k, v in fields.items():
            setattr(cam, k, (C.c_float * 3)(*v))
        cam.fov_degrees = 49
        cams.append(cam)
    return cams


def _scene(oracle, case):
    if case == "mesh":  # Scene1 with its big ball tessellated, as tests/test_gpu_mesh.py builds its small one
        objs = oracle.load_scene_json_py(scene_path("Scene1"))
        big = objs[64]
        objs[64] = dict(type=oracle.OBJ_MESH, position=big["position"], mesh=0, base=big["base"], emissive=big["emissive"],
                        smoothness=big["smoothness"], specular_amount=big["specular_amount"], specular=big["specular"])
        return objs, [oracle.uv_sphere(1.0, 8, 12)]
    return oracle.load_scene_json_py(scene_path(case)), None


def _scene_tracer(srt, oracle, case, w, h, cam):
    objs, meshes = _scene(oracle, case)
    oarr, n = oracle.make_objects(objs)
    pt = srt.PathTracer(w, h)
    keep = [oarr]
    marr, mn = None, 0
    if meshes:
        marr, mn, mkeep = oracle.make_meshes(meshes)
        keep += [marr, mkeep]
        pt.set_meshes(C.cast(marr, C.POINTER(srt.Mesh)), mn)
    pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
    pt.set_camera(cam)
    return pt, (oarr, n, marr, mn), keep


_EXPECTED = {}


def _expected(srt, oracle, case, k):
    """The (K, H, W) planes by definition: srt_oracle_closest_m along srt_oracle_ray_direction(cam, 2kW, 2kH, X, Y).  Computed
    once per (scene, k) and shared."""
    if (case, k) not in _EXPECTED:
        _, ocam = _cameras(srt, oracle, case)
        objs, meshes = _scene(oracle, case)
        oarr, n = oracle.make_objects(objs)
        marr, mn, mkeep = oracle.make_meshes(meshes) if meshes else (None, 0, None)
        L = oracle.lib()
        d, nn, pp, t = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)(), C.c_float()
        origin = (C.c_float * 3)(*ocam.position)
        out = np.empty((k * k, SH, SW), np.int32)
        for s in range(k * k):
            i, j = s % k, s // k
            for y in range(SH):
                for x in range(SW):
                    L.srt_oracle_ray_direction(C.byref(ocam), 2 * k * SW, 2 * k * SH, 2 * k * x + 2 * i - (k - 1), 2 * k * y + 2 * j - (k - 1), d)
                    out[s, y, x] = L.srt_oracle_closest_m(oarr, n, marr, mn, origin, d, nn, pp, C.byref(t))
        out.setflags(write=False)
        _EXPECTED[(case, k)] = out
    return _EXPECTED[(case, k)]


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("case", ["Scene1", "Scene3", "mesh"])
def test_subsamples_equal_the_oracle(srt, oracle, case, k):
    import torch

    cam, _ = _cameras(srt, oracle, case)
    want = _expected(srt, oracle, case, k)
    pt, _, keep = _scene_tracer(srt, oracle, case, SW, SH, cam)
    pt.render_subsamples(k)
    got = pt.subsamples()
    assert got.shape == want.shape
    assert np.array_equal(got, want), "%d of %d sub-samples differ" % (int((got != want).sum()), want.size)
    assert len(np.unique(want)) > 10
    # the pixel's own ray: the k = 1 plane, and the centre plane of k = 3
    pt.render_gbuffer(outputs=srt.capi.GBUF_OBJECT)
    obj = pt.gbuffer("object")
    if k == 1:
        assert np.array_equal(got[0], obj)
    if k == 3:
        assert np.array_equal(got[4], obj)
    if k > 1:
        assert (got != obj[None]).any()  # some sub-sample sees another object than the pixel
    # the band of memory rows [5, 14) into a bound buffer pre-filled with a sentinel: scene rows [H - 14, H - 5), nothing else
    sentinel = -77
    buf = torch.full((k * k, SH, SW), sentinel, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    pt.bind_subsamples(buf)
    pt.render_subsamples(k, rows=BAND)
    pt.wait()
    band = buf.cpu().numpy()
    y0, y1 = SH - BAND[1], SH - BAND[0]
    assert np.array_equal(band[:, y0:y1], want[:, y0:y1])
    assert np.all(band[:, :y0] == sentinel) and np.all(band[:, y1:] == sentinel)
    assert np.array_equal(pt.subsamples(), band)  # srt_read_subsamples reads the current (bound) buffer
    pt.bind_subsamples(None)
    assert np.array_equal(pt.subsamples(), want)  # ... and the own one still holds the whole frame
    pt.close()
    del keep, buf


def test_nan_camera_direction_misses_everywhere(srt, oracle):
    cam, _ = _cameras(srt, oracle, nan=True)
    pt, _, keep = _scene_tracer(srt, oracle, "Scene1", SW, SH, cam)
    for k in (1, 4):
        pt.render_subsamples(k)
        assert np.all(pt.subsamples() == -1)
    pt.close()


# ---- the resolve on synthetic inputs ------------------------------------------------------------------------------------------
AW, AH = 45, 29
ABSENT = 99  # an object index no pixel has


def synthetic(w, h, seed, n_objects=5):
    """Object blobs as in test_gpu_upsample.synthetic (5 objects, a block of misses, scattered misses, a one-pixel-wide column
    and row object) with positive colours in [0.05, 4] and alphas of 0, 1 and 0.5."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy = rng.uniform(0, w, n_objects), rng.uniform(0, h, n_objects)
    obj = np.argmin(np.stack([np.hypot(xs - cx[k], ys - cy[k]) for k in range(n_objects)]), axis=0).astype(np.int32)
    obj[rng.random((h, w)) < 0.04] = -1
    obj[(xs < w * 0.2) & (ys > h * 0.6)] = -1
    obj[:, w // 2 + 1] = n_objects
    obj[h // 3 + 1, :] = n_objects + 1
    c = np.concatenate([rng.uniform(0.05, 4.0, (h, w, 3)), rng.choice(np.array([0.0, 1.0, 0.5], np.float32), size=(h, w, 1))],
                       -1).astype(np.float32)
    return c, obj


def draw_subsamples(obj, k, seed):
    """Per pixel: about half keep all planes on their own object; the others draw every plane as own (50%), the object of a
    random pixel of the 3 x 3 neighbourhood (35%, clamped to the frame) or an index no pixel has (15%)."""
    rng = np.random.default_rng(seed)
    h, w = obj.shape
    K = k * k
    ys, xs = np.mgrid[0:h, 0:w]
    ny = np.clip(ys[None] + rng.integers(-1, 2, (K, h, w)), 0, h - 1)
    nx = np.clip(xs[None] + rng.integers(-1, 2, (K, h, w)), 0, w - 1)
    u = rng.random((K, h, w))
    sub = np.where(u < 0.5, obj[None], np.where(u < 0.85, obj[ny, nx], ABSENT)).astype(np.int32)
    interior = rng.random((h, w)) < 0.5
    sub[:, interior] = obj[interior]
    return np.ascontiguousarray(sub)


def _bound_tracer(srt, c, obj, sub, denoised=None):
    """A tracer whose accumulator is c, whose OBJECT guide and sub-sample buffer are torch tensors, and whose denoised buffer
    (when given) is a bound tensor after one srt_denoise has marked it written."""
    import torch

    h, w = obj.shape
    pt = srt.PathTracer(w, h)
    t = {"object": torch.from_numpy(obj).to("cuda:0"), "sub": torch.from_numpy(sub).to("cuda:0")}
    pt.bind_gbuffer("object", t["object"])
    pt.bind_subsamples(t["sub"])
    pt.write_accumulator(c)
    if denoised is not None:
        # srt_denoise needs its other guides once; afterwards the bound buffer is overwritten with the colours of the test
        z4 = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
        t["z4"] = z4
        for name in ("normal_depth", "position", "albedo"):
            pt.bind_gbuffer(name, z4)
        t["dn"] = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
        pt.bind_denoised(t["dn"])
        torch.cuda.synchronize()
        pt.denoise(iterations=1, gbuffer=False)
        pt.wait()
        t["dn"].copy_(torch.from_numpy(denoised).to("cuda:0"))
    torch.cuda.synchronize()
    return pt, t


@pytest.mark.parametrize("source", ["accumulator", "denoised"])
@pytest.mark.parametrize("k", [2, 3, 4])
def test_resolve_matches_the_definition(srt, k, source):
    c, obj = synthetic(AW, AH, seed=11)
    sub = draw_subsamples(obj, k, seed=20 + k)
    other = np.random.default_rng(5).uniform(0.05, 4.0, c.shape).astype(np.float32)  # what the source NOT chosen holds
    den = source == "denoised"
    pt, keep = _bound_tracer(srt, other if den else c, obj, sub, denoised=c if den else other)
    pt.antialias(k, denoised=den, guides=False)
    got = pt.antialiased()
    ref, foreign, changed = resolve(c, obj, sub)
    interior = ~foreign
    assert 0.3 < interior.mean() < 0.8 and changed.sum() >= 50 and (foreign & ~changed).sum() > 0
    err = _rel_err(got, ref, changed)
    print("k %d %s: max relative error %.3g over %d changed pixels (%d interior, %d fallback only)" %
          (k, source, err, changed.sum(), interior.sum(), (foreign & ~changed).sum()))
    assert err <= REL_TOL
    # exact: interior pixels and pixels whose foreign sub-samples all fall back keep their bits; alpha everywhere
    assert _same_bits(got[~changed], c[~changed])
    assert _same_bits(got[..., 3], c[..., 3])
    # a second call gives the same bits
    pt.antialias(k, denoised=den, guides=False)
    assert _same_bits(pt.antialiased(), got)
    pt.close()
    del keep


def test_k1_is_the_identity(srt):
    c, obj = synthetic(AW, AH, seed=12)
    sub = draw_subsamples(obj, 1, seed=3)  # even with a foreign plane value: its footprint is the pixel itself
    assert (sub[0] != obj).any()
    pt, keep = _bound_tracer(srt, c, obj, sub)
    pt.antialias(1, guides=False)
    assert _same_bits(pt.antialiased(), c)
    pt.close()
    del keep


@pytest.mark.parametrize("k", [2, 4])
def test_non_finite_colours_of_another_object_do_not_spread(srt, k):
    c, obj = synthetic(AW, AH, seed=13)
    sub = draw_subsamples(obj, k, seed=40 + k)
    pt, keep = _bound_tracer(srt, c, obj, sub)
    pt.antialias(k, guides=False)
    clean = pt.antialiased()
    for victim, value in ((2, np.nan), (-1, np.inf), (6, -np.inf)):  # an object, the misses, the one-pixel-wide row
        bad = c.copy()
        bad[obj == victim, :3] = value
        pt.write_accumulator(bad)
        pt.antialias(k, guides=False)
        got = pt.antialiased()
        untouched = (obj != victim) & ~(sub == victim).any(axis=0)
        assert untouched.sum() > AW * AH // 4
        assert _same_bits(got[untouched], clean[untouched]), (victim, value)
    pt.close()
    del keep


def test_taps_outside_the_frame_are_skipped(srt):
    """The four corner pixels with sub-samples that point outward (and one that points inward, for contrast)."""
    import torch

    k, w, h = 2, 11, 9
    rng = np.random.default_rng(2)
    c = rng.uniform(0.05, 4.0, (h, w, 4)).astype(np.float32)
    obj = np.arange(w * h, dtype=np.int32).reshape(h, w)  # every pixel its own object
    sub = np.broadcast_to(obj, (4, h, w)).copy()
    for (x, y) in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)):
        sx, sy = (1 if x == 0 else -1), (1 if y == 0 else -1)  # towards the inside
        out_plane = (0 if sy > 0 else 1) * 2 + (0 if sx > 0 else 1)
        in_plane = (1 if sy > 0 else 0) * 2 + (1 if sx > 0 else 0)
        sub[out_plane, y, x] = obj[y, x + sx]       # the horizontal neighbour's object, but the footprint lies outside: fallback
        sub[in_plane, y, x] = obj[y + sy, x + sx]   # the diagonal neighbour inside: one tap
    pt, keep = _bound_tracer(srt, c, obj, sub)
    pt.antialias(k, guides=False)
    got = pt.antialiased()
    ref, foreign, changed = resolve(c, obj, sub)
    assert foreign.sum() == 4 and changed.sum() == 4
    assert _rel_err(got, ref, changed) <= REL_TOL
    d = c[..., :3].astype(np.float64)
    assert np.allclose(ref[0, 0, :3], (3 * d[0, 0] + d[1, 1]) / 4, rtol=1e-14)
    assert np.all(np.isfinite(got)) and _same_bits(got[~changed], c[~changed])
    # all four planes of the corners pointing at objects no pixel inside has: nothing changes, nothing outside is read
    sub[:, 0, 0] = sub[:, 0, w - 1] = sub[:, h - 1, 0] = sub[:, h - 1, w - 1] = ABSENT + w * h
    keep["sub"].copy_(torch.from_numpy(sub))
    pt.antialias(k, guides=False)
    assert _same_bits(pt.antialiased(), c)
    pt.close()
    del keep


# ---- real frames ----------------------------------------------------------------------------------------------------------------
def _host_scene_tracer(srt, name, w, h):
    scene = srt.host.Scene(scene_path(name))
    objs, n = scene.objects_copy()
    pt = srt.PathTracer(w, h)
    pt.set_scene(objs, n)
    pt.set_camera(srt.default_camera())
    return pt, (objs, n)


@pytest.mark.parametrize("denoise", [False, True])
def test_real_frames_match_the_definition(srt, denoise):
    w, h, k = 64, 40, 4
    pt, keep = _host_scene_tracer(srt, "Scene1", w, h)
    pt.render(spp=8, bounces=4, seed=5)
    pt.render_gbuffer()
    pt.render_subsamples(k)
    if denoise:
        pt.denoise(gbuffer=False)
    pt.antialias(k, denoised=denoise, guides=False)
    got = pt.antialiased()
    c = pt.denoised() if denoise else pt.accumulator()
    obj, sub = pt.gbuffer("object"), pt.subsamples()
    ref, foreign, changed = resolve(c, obj, sub)
    err = _rel_err(got, ref, changed)
    print("Scene1 %dx%d k %d denoise %d: max relative error %.3g, %d foreign, %d changed pixels" % (w, h, k, denoise, err, foreign.sum(), changed.sum()))
    assert err <= REL_TOL
    differs = (_bits(got) != _bits(c)).any(axis=2)
    assert differs.any()
    assert not (differs & ~foreign).any()  # every changed pixel has a foreign sub-sample
    assert _same_bits(got[~changed], c[~changed]) and _same_bits(got[..., 3], c[..., 3])
    pt.close()


def _tool():
    spec = importlib.util.spec_from_file_location("antialias_time", os.path.join(ROOT, "tools", "antialias_time.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_quality_against_supersampled_ground_truth(srt):
    """tools/antialias_time.py's procedure: Scene1 at 96 x 54, k = 4, 64 spp, against the mean of the 16 pixels of a 768 x 432
    render (another seed) whose rays are the sub-samples' rays.  No measured number is asserted: the anti-aliased frame's
    summed squared error over the edge pixels is below the raw frame's.
    The two figures on the MI355X have NOT been recorded yet (the test prints them)."""
    q = _tool().quality_figures(srt)
    print("edge pixels %d: summed squared error raw %.6g, anti-aliased %.6g (mse %.4g -> %.4g)" %
          (q["edge_pixels"], q["sse_raw"], q["sse_antialiased"], q["mse_raw"], q["mse_antialiased"]))
    assert q["edge_pixels"] > 100
    assert q["sse_antialiased"] < q["sse_raw"]


# ---- non-interference and flags -------------------------------------------------------------------------------------------------
def cvtt(f):
    """(int)f with x86 cvttss2si semantics: NaN and out-of-range give INT_MIN."""
    f = np.asarray(f, np.float32)
    bad = np.isnan(f) | (f >= np.float32(2147483648.0)) | (f < np.float32(-2147483648.0))
    return np.where(bad, np.int64(-2147483648), np.trunc(np.where(bad, 0, f)).astype(np.int64))


def tone_map(img):
    """The render's packing of float4 pixels (c / (1 + c), alpha a / (0 + a), x 255, truncated, capped, low byte), in float32."""
    c = np.asarray(img, np.float32)
    with np.errstate(all="ignore"):
        r, g, b = (c[..., k] / (np.float32(1) + c[..., k]) for k in range(3))
        a = c[..., 3] / (np.float32(0) + c[..., 3])
    ch = [(np.minimum(cvtt(v * np.float32(255)), 255) & 0xFF).astype(np.uint32) for v in (a, r, g, b)]
    return ch[0] << 24 | ch[1] << 16 | ch[2] << 8 | ch[3]


def test_non_interference_and_the_framebuffer_flag(srt):
    w, h, k = 64, 40, 2
    pt, keep = _host_scene_tracer(srt, "Scene1", w, h)
    pt.render(spp=4, bounces=4, seed=9, count_rays=True, count_work=True)
    pt.render_gbuffer()
    pt.temporal(samples=4, gbuffer=False)
    pt.denoise(gbuffer=False)
    pt.render_subsamples(k)

    def state():
        st, wc = pt.stats(), pt.work_counts()
        return dict(acc=pt.accumulator(), dn=pt.denoised(), fb=pt.framebuffer(), sub=pt.subsamples(), hist=pt.history_length(),
                    g={n: pt.gbuffer(n) for n in ("object", "normal_depth", "position", "albedo")},
                    st=bytes(st), wc=wc.as_dict())

    def same(a, b, fb=True):
        assert _same_bits(a["acc"], b["acc"]) and _same_bits(a["dn"], b["dn"]) and np.array_equal(a["sub"], b["sub"])
        assert _same_bits(a["hist"], b["hist"])
        assert np.array_equal(a["g"]["object"], b["g"]["object"])
        assert all(_same_bits(a["g"][n], b["g"][n]) for n in ("normal_depth", "position", "albedo"))
        assert a["st"] == b["st"] and a["wc"] == b["wc"]
        if fb:
            assert np.array_equal(a["fb"], b["fb"])

    before = state()
    for den in (False, True):
        pt.antialias(k, denoised=den, guides=False)
        res = pt.antialiased()
        after = state()
        same(before, after)  # without SRT_AA_FRAMEBUFFER the framebuffer is unchanged too
        pt.antialias(k, denoised=den, framebuffer=True, guides=False)
        assert _same_bits(pt.antialiased(), res)
        after = state()
        same(before, after, fb=False)
        assert np.array_equal(after["fb"], tone_map(res)[::-1])  # memory row H - 1 - y
        assert not np.array_equal(after["fb"], before["fb"])
        before = after
    # srt_render_subsamples leaves them alone as well (the sub-sample buffer aside)
    pt.render_subsamples(k)
    same(before, state())
    pt.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def _code(srt, call):
    with pytest.raises(srt.SrtError) as e:
        call()
    return e.value.code


def test_errors(srt):
    import torch

    w, h = 40, 24
    STATE, ARG = srt.capi.ERR_STATE, srt.capi.ERR_INVALID_ARG
    pt = srt.PathTracer(w, h)
    assert _code(srt, lambda: pt.render_subsamples(2)) == STATE  # no scene, no camera
    assert _code(srt, pt.subsamples) == STATE and _code(srt, pt.antialiased) == STATE
    pt.close()
    pt, keep = _host_scene_tracer(srt, "Scene1", w, h)
    pt.render(spp=1, bounces=2)
    for kw in (dict(k=0), dict(k=5), dict(k=-1), dict(k=2, rows=(3, 3)), dict(k=2, rows=(-1, 4)), dict(k=2, rows=(0, h + 1)), dict(k=2, flags=1)):
        assert _code(srt, lambda: pt.render_subsamples(**kw)) == ARG, kw
    for k in (0, 5, -3):
        assert _code(srt, lambda: pt.antialias(k, guides=False)) == ARG
    for source, flags in ((2, 0), (-1, 0), (0, 1), (0, 4), (0, 3)):
        p = srt.capi.AntialiasParams(2, source, flags)
        assert pt.L.srt_antialias(pt._h, C.byref(p)) == ARG, (source, flags)
    # OBJECT never bound or rendered; then the sub-samples never bound or rendered
    assert _code(srt, lambda: pt.antialias(2, guides=False)) == STATE
    pt.render_gbuffer(outputs=srt.capi.GBUF_OBJECT)
    assert _code(srt, lambda: pt.antialias(2, guides=False)) == STATE
    # the own buffer rendered for a band only
    pt.render_subsamples(2, rows=(0, h // 2))
    assert _code(srt, lambda: pt.antialias(2, guides=False)) == STATE
    pt.render_subsamples(2, rows=(h // 2, h))  # ... the other band completes the frame
    pt.antialias(2, guides=False)
    # the denoised source before the first srt_denoise
    assert _code(srt, lambda: pt.antialias(2, denoised=True, guides=False)) == STATE
    # the own buffer rendered with another k
    assert _code(srt, lambda: pt.antialias(3, guides=False)) == STATE
    pt.render_subsamples(3)
    assert _code(srt, lambda: pt.antialias(2, guides=False)) == STATE
    pt.antialias(3, guides=False)
    # srt_set_camera after the sub-sample render; a band with the new camera does not make a frame
    cam = srt.default_camera()
    cam.position = (C.c_float * 3)(0.1, 0.0, 0.0)
    pt.set_camera(cam)
    assert _code(srt, lambda: pt.antialias(3, guides=False)) == STATE
    pt.render_subsamples(3, rows=(0, 5))
    assert _code(srt, lambda: pt.antialias(3, guides=False)) == STATE
    pt.render_subsamples(3)
    pt.antialias(3, guides=False)
    # a scene change
    pt.set_scene(*keep)
    assert _code(srt, lambda: pt.antialias(3, guides=False)) == STATE
    # a bound buffer is the caller's responsibility: no such check
    buf = torch.zeros((9, h, w), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    pt.bind_subsamples(buf)
    pt.antialias(3, guides=False)
    assert pt.antialiased().shape == (h, w, 4)
    # tensors of the wrong kind are refused before any native call
    for t in (torch.empty((9, h, w), dtype=torch.int64, device="cuda:0"), torch.empty((9, h, w), dtype=torch.int32),
              torch.empty((5, h, w), dtype=torch.int32, device="cuda:0"), torch.empty((9, h, 2 * w), dtype=torch.int32, device="cuda:0")[:, :, ::2],
              np.zeros((9, h, w), np.int32)):
        with pytest.raises((TypeError, ValueError, AttributeError)):
            pt.bind_subsamples(t)
    for t in (torch.empty((h, w, 4), dtype=torch.float64, device="cuda:0"), torch.empty((h, w, 3), device="cuda:0"), torch.empty((h, w, 4))):
        with pytest.raises((TypeError, ValueError)):
            pt.bind_antialiased(t)
    pt.close()
    # a frame whose virtual size reaches 2^24
    big = srt.PathTracer(2 ** 21, 1)
    big.set_scene(*keep)
    big.set_camera(srt.default_camera())
    assert _code(srt, lambda: big.render_subsamples(4)) == ARG
    big.close()
    del buf


# ---- the layers above -------------------------------------------------------------------------------------------------------------
def test_torch_bound_output_and_subsamples(srt):
    import torch

    w, h, k = 61, 35, 3
    pt, keep = _host_scene_tracer(srt, "Scene1", w, h)
    pt.render(spp=4, bounces=4, seed=3)
    pt.antialias(k)
    own, own_sub = pt.antialiased(), pt.subsamples()
    stream = torch.cuda.Stream(device=0)
    pt.set_stream(stream.cuda_stream)
    out = torch.full((h, w, 4), -5.0, dtype=torch.float32, device="cuda:0")
    sub = torch.full((k * k, h, w), -9, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    pt.bind_antialiased(out)
    pt.bind_subsamples(sub)
    pt.antialias(k)
    stream.synchronize()
    assert _same_bits(out.cpu().numpy(), own) and np.array_equal(sub.cpu().numpy(), own_sub)
    assert _same_bits(pt.antialiased(), own)
    assert not _same_bits(own, pt.accumulator())
    pt.bind_antialiased(None)
    pt.bind_subsamples(None)
    pt.set_stream(0)
    assert _same_bits(pt.antialiased(), own)  # the own buffer still holds the first result
    pt.close()


def _rgb(fb):
    return np.stack([(fb >> 16) & 255, (fb >> 8) & 255, fb & 255], -1).astype(np.uint8)


def _ppm_rgb(path, w, h):
    data = open(path, "rb").read()
    head = b"P6\n%d %d\n255\n" % (w, h)
    assert data.startswith(head)
    return np.frombuffer(data[len(head):], np.uint8).reshape(h, w, 3)


def test_host_renderer_equals_the_c_calls(srt):
    """RenderFrame with antialias on: the start-up frame, the frame after an edit and the one after that (as
    test_gpu_upsample.test_render_frame_with_and_without_guided_upsample restates them), each followed by the resolve."""
    w, h, k = 96, 54, 2
    sw = w // 16 + 1
    frames = [dict(reset=False, steps=2), dict(reset=True, steps=8), dict(reset=True, steps=2)]
    pt, keep = _host_scene_tracer(srt, "Scene1", w, h)
    want = []
    for f in frames:
        pt.render(spp=1, bounces=2, seed=0, first_sample=1, preview=True, stripe_width=sw, selected=-1, **f)
        plain = pt.framebuffer()
        pt.antialias(k, framebuffer=True)
        want.append((plain, pt.framebuffer(), pt.antialiased(), pt.accumulator()))
    pt.close()
    assert any(not np.array_equal(p, a) for p, a, _, _ in want)
    scene = srt.host.Scene(scene_path("Scene1"))
    for on in (False, True):
        r = srt.host.Renderer(w, h)
        r.set_scene(scene)
        r.set_antialias(k if on else 0)
        for i, (plain, aa_fb, aa, acc) in enumerate(want):
            if i == 1:
                r.invalidate()
            assert r.render_frame()
            assert np.array_equal(r.framebuffer(), aa_fb if on else plain), (on, i)
            assert _same_bits(r.accumulator(), acc), (on, i)
            if on:
                assert _same_bits(r.antialiased(), aa), i
        if on:  # the single call, and whole frame only
            r.antialias(k)
            assert _same_bits(r.antialiased(), want[-1][2])
            r.set_band(0, h // 2)
            with pytest.raises(RuntimeError):
                r.render_frame()
        r.close()


def test_cli_writes_the_antialiased_ppm(srt, tmp_path):
    w, h = 96, 54
    base = [CLI, "--scene", scene_path("Scene1"), "--width", str(w), "--height", str(h), "--spp", "4", "--bounces", "2"]
    r1 = subprocess.run(base + ["--aa", "2", "--out", str(tmp_path / "a.ppm"), "--denoise", str(tmp_path / "d.ppm")], capture_output=True,
                        text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr[-2000:]
    pt, keep = _host_scene_tracer(srt, "Scene1", w, h)
    pt.render(spp=4, bounces=2, seed=0, count_rays=True)
    plain = _rgb(pt.framebuffer())
    pt.antialias(2, framebuffer=True)
    aa = _rgb(pt.framebuffer())
    assert np.array_equal(_ppm_rgb(tmp_path / "a.ppm", w, h), aa) and not np.array_equal(aa, plain)
    pt.denoise()
    pt.antialias(2, denoised=True, framebuffer=True, guides=False)
    assert np.array_equal(_ppm_rgb(tmp_path / "d.ppm", w, h), _rgb(pt.framebuffer()))
    pt.close()
    for bad in (["--aa", "5"], ["--aa", "2", "--devices", "0,0"]):
        r = subprocess.run(base + bad + ["--out", str(tmp_path / "x.ppm")], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "--aa" in r.stderr and not (tmp_path / "x.ppm").exists()


def test_scripted_viewer_antialias(srt, tmp_path):
    if not os.path.exists(VIEWER):
        pytest.fail("srt_viewer not built (make -C software-raytracer_amd/host)")
    w, h = 96, 54
    outs = [str(tmp_path / ("%s.ppm" % n)) for n in "abc"]
    script = tmp_path / "session.txt"
    script.write_text("frames 1\nsave %s\nantialias 2\nframes 2\nsave %s\nantialias off\nframes 1\nsave %s\n" % tuple(outs))
    r = subprocess.run([VIEWER, "--scene", scene_path("Scene1"), "--width", str(w), "--height", str(h), "--script", str(script)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [_ppm_rgb(p, w, h) for p in outs]
    rr = srt.host.Renderer(w, h)
    rr.set_scene(srt.host.Scene(scene_path("Scene1")))
    rr.render_frame()
    want = [_rgb(rr.framebuffer())]
    rr.set_antialias(2)
    rr.render_frame()
    rr.render_frame()
    want.append(_rgb(rr.framebuffer()))
    rr.set_antialias(0)
    rr.render_frame()
    want.append(_rgb(rr.framebuffer()))
    rr.close()
    for i in range(3):
        assert np.array_equal(got[i], want[i]), i
    assert not np.array_equal(got[0], got[1])
