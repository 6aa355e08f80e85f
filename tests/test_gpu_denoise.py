"""Denoiser (srt_denoise) on the MI355X: the à-trous filter of include/srt_pathtrace.h against a float64 numpy restatement on
synthetic guides, miss pass-through and object isolation, the framebuffer flag, non-interference and determinism, the noise
it removes from real renders, errors, torch binding, the host layer and the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
NAMES = ["object", "normal_depth", "position", "albedo"]
# the kernel against reference() over test_filter_matches_the_definition: measured maximum relative error 1.1e-5 on the MI355X
# (the weights use the hardware exp2 / log2)
REL_TOL = 1e-4
H5 = np.array([1, 4, 6, 4, 1], np.float64) / 16


# ---- the definition ---------------------------------------------------------------------------------------------------
def reference(acc, obj, nd, pos, alb, iterations, sigma_color, sigma_normal, sigma_plane, albedo):
    """The filter of include/srt_pathtrace.h in float64 (the guides and colour as float32 arrays, scene rows)."""
    H, W = obj.shape
    hit = obj >= 0
    m = np.ones((H, W, 3))
    if albedo:
        a = alb[..., :3]
        m = np.where(a >= np.float32(1e-3), a.astype(np.float64), 1.0)
    with np.errstate(all="ignore"):
        c = acc[..., :3].astype(np.float64) / m
    n = nd[..., :3].astype(np.float64)
    d = nd[..., 3].astype(np.float64)
    x = pos[..., :3].astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    for i in range(iterations):
        s = 1 << i
        sw = np.zeros((H, W))
        sc = np.zeros((H, W, 3))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + s * dy, xs + s * dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                w = np.full((H, W), H5[dx + 2] * H5[dy + 2])
                cq = c[qy, qx]
                if dx or dy:
                    take = inside & hit & (obj[qy, qx] == obj)
                    with np.errstate(all="ignore"):
                        if sigma_normal > 0:
                            w = w * np.maximum(0.0, np.sum(n * n[qy, qx], axis=2)) ** sigma_normal
                        if sigma_plane > 0:
                            w = w * np.exp(-np.abs(np.sum(n * (x[qy, qx] - x), axis=2)) / (sigma_plane * d))
                        if sigma_color > 0:
                            w = w * np.exp(-np.sum((c - cq) ** 2, axis=2) / (sigma_color * 2.0 ** -i) ** 2)
                else:
                    take = inside
                w = np.where(take, w, 0.0)
                sw += w
                sc += np.where(take[..., None], w[..., None] * np.where(take[..., None], cq, 0.0), 0.0)
        with np.errstate(all="ignore"):
            c = np.where(hit[..., None], sc / sw[..., None], c)
    out = np.empty((H, W, 4))
    out[..., :3] = c * m
    out[..., 3] = acc[..., 3]
    out[~hit] = acc[~hit]
    return out


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


# ---- synthetic guides ---------------------------------------------------------------------------------------------------
def synthetic(w, h, seed, n_objects=5, miss_fraction=0.15):
    """Objects as blobs of smoothly varying normals, points and depths, with noisy colours; about miss_fraction misses; some
    albedo channels below 1e-3."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy = rng.uniform(0, w, n_objects), rng.uniform(0, h, n_objects)
    dist = np.stack([np.hypot(xs - cx[k], ys - cy[k]) for k in range(n_objects)])
    obj = np.argmin(dist, axis=0).astype(np.int32)
    obj[rng.random((h, w)) < miss_fraction * 0.3] = -1
    obj[(xs < w * 0.12) & (ys > h * 0.7)] = -1
    base_n = rng.normal(size=(n_objects, 3))
    nrm = base_n[np.maximum(obj, 0)] + 0.25 * np.stack([np.sin(xs / 7.0), np.cos(ys / 5.0), np.sin((xs + ys) / 11.0)], -1)
    nrm += 0.05 * rng.normal(size=nrm.shape)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    depth = 2.0 + 3.0 * rng.random(n_objects)[np.maximum(obj, 0)] + 0.01 * xs
    pnt = np.stack([xs * 0.01, ys * 0.01, depth], -1) + 0.01 * rng.normal(size=(h, w, 3))
    nd = np.concatenate([nrm, depth[..., None]], -1).astype(np.float32)
    pos = np.concatenate([pnt, np.ones((h, w, 1))], -1).astype(np.float32)
    alb = np.concatenate([rng.uniform(0.05, 0.9, (n_objects, 3))[np.maximum(obj, 0)] * (1 + 0.2 * rng.random((h, w, 3))),
                          np.zeros((h, w, 1))], -1).astype(np.float32)
    small = rng.random((h, w, 3)) < 0.1
    alb[..., :3] = np.where(small, rng.choice(np.array([0.0, 5e-4, 9.99e-4, 1e-3], np.float32), size=(h, w, 3)), alb[..., :3])
    acc = np.concatenate([alb[..., :3] * rng.uniform(0.2, 4.0, (h, w, 3)) + rng.uniform(0.01, 0.2, (h, w, 3)),
                          rng.choice(np.array([0.0, 1.0], np.float32), size=(h, w, 1))], -1).astype(np.float32)
    miss = obj < 0
    nd[miss] = np.array([0, 0, 0, np.inf], np.float32)
    pos[miss] = 0
    alb[miss] = 0
    return acc, obj, nd, pos, alb


def _bind(pt, obj, nd, pos, alb):
    import torch

    t = {"object": torch.from_numpy(obj).to("cuda:0"), "normal_depth": torch.from_numpy(nd).to("cuda:0"),
         "position": torch.from_numpy(pos).to("cuda:0"), "albedo": torch.from_numpy(alb).to("cuda:0")}
    torch.cuda.synchronize()
    for k, v in t.items():
        pt.bind_gbuffer(k, v)
    return t


def _rel_err(got, ref, hit):
    g, r = got[hit][:, :3].astype(np.float64), ref[hit][:, :3]
    return float(np.max(np.abs(g - r) / np.maximum(np.abs(r), 1e-6)))


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


CASES = [  # iterations, sigma_color, sigma_normal, sigma_plane, albedo
    (1, 0.0, 0.0, 0.0, False), (1, 0.5, 128.0, 0.05, True), (2, 0.0, 128.0, 0.0, True), (3, 0.0, 0.0, 0.05, False),
    (3, 1.0, 0.0, 0.0, True), (4, 0.5, 16.0, 0.05, False), (5, 0.0, 128.0, 0.02, True), (5, 2.0, 64.0, 0.1, True),
    # levels 6..8: steps 32, 64 and 128 (at 67 x 45, step 64 leaves only taps of one row or column, step 128 only the centre)
    (6, 0.5, 32.0, 0.02, True), (7, 1.0, 128.0, 0.05, False), (8, 0.0, 32.0, 0.02, True), (8, 2.0, 64.0, 0.0, False),
]


@pytest.mark.parametrize("w,h", [(67, 45), (256, 160)])
def test_filter_matches_the_definition(srt, w, h):
    acc, obj, nd, pos, alb = synthetic(w, h, seed=w)
    hit = obj >= 0
    pt = srt.PathTracer(w, h)
    keep = _bind(pt, obj, nd, pos, alb)
    pt.write_accumulator(acc)
    worst = 0.0
    for it, sc, sn, sx, albedo in CASES:
        pt.denoise(iterations=it, sigma_color=sc, sigma_normal=sn, sigma_plane=sx, albedo=albedo, gbuffer=False)
        got = pt.denoised()
        ref = reference(acc, obj, nd, pos, alb, it, sc, sn, sx, albedo)
        err = _rel_err(got, ref, hit)
        worst = max(worst, err)
        assert err <= REL_TOL, (it, sc, sn, sx, albedo, err)
        assert _same_bits(got[..., 3], acc[..., 3]), "alpha is not the input's"
        assert _same_bits(got[~hit], acc[~hit]), "miss pixels are not the input"
    print("max relative error %.3g" % worst)
    pt.close()
    del keep


def test_isolation_and_constant_objects(srt):
    w, h = 96, 72
    acc, obj, nd, pos, alb = synthetic(w, h, seed=3, n_objects=4)
    pt = srt.PathTracer(w, h)
    keep = _bind(pt, obj, nd, pos, alb)
    params = dict(iterations=5, sigma_color=0.5, sigma_normal=64.0, sigma_plane=0.05, gbuffer=False)
    pt.write_accumulator(acc)
    pt.denoise(**params)
    base = pt.denoised()
    rng = np.random.default_rng(9)
    for k in range(4):
        # every other object's colours perturbed, NaN and inf among them: object k's output keeps its bits
        other = (obj >= 0) & (obj != k)
        bad = acc.copy()
        noise = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -3.0, 0.0], np.float32), size=bad.shape)
        bad[other] = noise[other]
        pt.write_accumulator(bad)
        pt.denoise(**params)
        got = pt.denoised()
        assert _same_bits(got[obj == k], base[obj == k]), k
        assert _same_bits(got[obj < 0], bad[obj < 0])
    # a constant-colour object stays constant (albedo constant on it too, so the demodulated colour is constant)
    const = acc.copy()
    alb2 = alb.copy()
    alb2[obj == 1] = np.array([0.3, 0.5, 0.7, 0.0], np.float32)
    keep = _bind(pt, obj, nd, pos, alb2)
    const[obj == 1] = np.array([0.8, 1.7, 0.25, 1.0], np.float32)
    pt.write_accumulator(const)
    for albedo in (False, True):
        pt.denoise(albedo=albedo, **params)
        got = pt.denoised()[obj == 1]
        assert np.max(np.abs(got[:, :3] / np.array([0.8, 1.7, 0.25]) - 1)) <= 1e-6
    pt.close()
    del keep


def test_framebuffer_flag(srt):
    w, h = 67, 45
    acc, obj, nd, pos, alb = synthetic(w, h, seed=11)
    acc[5, 7, :3] = [np.inf, 1e30, 0.0]
    pt = srt.PathTracer(w, h)
    keep = _bind(pt, obj, nd, pos, alb)
    pt.write_accumulator(acc)
    before = pt.framebuffer()
    pt.denoise(gbuffer=False)
    assert np.array_equal(pt.framebuffer(), before), "the framebuffer was written without SRT_DENOISE_FRAMEBUFFER"
    pt.denoise(gbuffer=False, framebuffer=True)
    fb = pt.framebuffer()
    assert np.array_equal(fb, tone_map(pt.denoised())[::-1])
    assert not np.array_equal(fb, before)
    pt.close()
    del keep


def _scene_tracer(srt, oracle, name, w, h):
    oarr, n = oracle.make_objects(oracle.load_scene_json_py(scene_path(name)))
    pt = srt.PathTracer(w, h)
    pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
    pt.set_camera(srt.default_camera())
    return pt, oarr


def test_non_interference_and_determinism(srt, oracle):
    w, h = 320, 256
    fields = ("rays", "sample_chunks", "tile_rows", "chunk_samples", "shape_source", "path_samples")
    runs = []
    for with_denoise in (False, True):
        pt, oarr = _scene_tracer(srt, oracle, "Scene1", w, h)
        pt.render(spp=8, bounces=4, seed=5, count_rays=True, count_work=True)
        first = pt.stats()
        pt.render_gbuffer()
        if with_denoise:
            acc, g = pt.accumulator(), {k: pt.gbuffer(k) for k in NAMES}
            pt.denoise(gbuffer=False)
            one = pt.denoised()
            pt.denoise(gbuffer=False, framebuffer=True)
            pt.denoise(gbuffer=False)
            assert _same_bits(pt.denoised(), one), "two denoises differ"
            assert _same_bits(pt.accumulator(), acc)
            for k in NAMES:
                assert np.array_equal(pt.gbuffer(k).view(np.uint32), g[k].view(np.uint32)), k
            after = pt.stats()
            assert all(getattr(after, f) == getattr(first, f) for f in fields) and after.kernel_ms == first.kernel_ms
        pt.render(spp=8, first_sample=9, reset=False, bounces=4, seed=5, count_rays=True, count_work=True)
        st = pt.stats()
        runs.append(([getattr(st, f) for f in fields], pt.work_counts().as_dict(), pt.framebuffer(), pt.accumulator()))
        pt.close()
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1]
    assert np.array_equal(a[2], b[2]) and _same_bits(a[3], b[3])


# measured on the MI355X with the defaults: MSE ratio 0.143 / 0.130, mean shift 0.53 % / 0.06 %
# (Scene1 / Scene_indirect)
MSE_RATIO_MAX = 0.5
MEAN_SHIFT_MAX = 0.02


@pytest.mark.parametrize("name", ["Scene1", "Scene_indirect"])
def test_it_denoises(srt, oracle, name):
    w, h = 320, 180
    pt, oarr = _scene_tracer(srt, oracle, name, w, h)
    pt.render(spp=1024, bounces=4, seed=777)
    ref = pt.accumulator()
    pt.render(spp=4, bounces=4, seed=1)
    noisy = pt.accumulator()
    pt.denoise()
    den = pt.denoised()
    hit = pt.gbuffer("object") >= 0
    tm = lambda a: (a[..., :3] / (1.0 + a[..., :3]))[hit].astype(np.float64)  # noqa: E731
    mse_noisy = float(np.mean((tm(noisy) - tm(ref)) ** 2))
    mse_den = float(np.mean((tm(den) - tm(ref)) ** 2))
    # the mean of the linear colour (what a normalised filter keeps; the tone map's concavity alone would move the
    # tone-mapped mean of a noisy frame up once it is smoothed)
    shift = abs(float(np.mean(den[..., :3][hit], dtype=np.float64)) / float(np.mean(noisy[..., :3][hit], dtype=np.float64)) - 1)
    print("%s: mse noisy %.4g denoised %.4g ratio %.3f, mean shift %.4f" % (name, mse_noisy, mse_den, mse_den / mse_noisy, shift))
    assert mse_den <= MSE_RATIO_MAX * mse_noisy
    assert shift <= MEAN_SHIFT_MAX
    pt.close()


def test_errors(srt):
    import torch

    w, h = 40, 24
    pt = srt.PathTracer(w, h)
    with pytest.raises(srt.SrtError) as e:
        pt.denoise(gbuffer=False)
    assert e.value.code == srt.capi.ERR_STATE
    with pytest.raises(srt.SrtError) as e:
        pt.denoised()
    assert e.value.code == srt.capi.ERR_STATE
    acc, obj, nd, pos, alb = synthetic(w, h, seed=1)
    keep = _bind(pt, obj, nd, pos, alb)
    pt.bind_gbuffer("albedo", None)  # never rendered: needed with albedo=True only
    with pytest.raises(srt.SrtError) as e:
        pt.denoise(gbuffer=False, albedo=True)
    assert e.value.code == srt.capi.ERR_STATE
    pt.denoise(gbuffer=False, albedo=False)
    pt.wait()
    bad = [dict(iterations=0), dict(iterations=9), dict(sigma_color=-1.0), dict(sigma_normal=-0.5), dict(sigma_plane=-1e-9),
           dict(sigma_color=float("nan")), dict(sigma_normal=float("nan")), dict(sigma_plane=float("nan"))]
    for kw in bad:
        with pytest.raises(srt.SrtError) as e:
            pt.denoise(gbuffer=False, albedo=False, **kw)
        assert e.value.code == srt.capi.ERR_INVALID_ARG, kw
    p = srt.capi.denoise_params(albedo=False)
    p.flags = 4
    assert pt.L.srt_denoise(pt._h, C.byref(p)) == srt.capi.ERR_INVALID_ARG
    for t in (torch.empty((h, w, 4), dtype=torch.float64, device="cuda:0"), torch.empty((h, w, 3), device="cuda:0"),
              torch.empty((h, w, 4)), torch.empty((h, 2 * w, 4), device="cuda:0")[:, ::2], np.zeros((h, w, 4), np.float32)):
        with pytest.raises((TypeError, ValueError)):
            pt.bind_denoised(t)
    pt.close()
    del keep


def test_torch_bound_output_on_a_torch_stream(srt, oracle):
    import torch

    w, h = 200, 120
    pt, oarr = _scene_tracer(srt, oracle, "Scene_indirect", w, h)
    pt.render(spp=4, bounces=4, seed=3)
    pt.denoise(iterations=4)
    own = pt.denoised()
    stream = torch.cuda.Stream(device=0)
    pt.set_stream(stream.cuda_stream)
    out = torch.full((h, w, 4), -5.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    pt.bind_denoised(out)
    pt.render(spp=4, bounces=4, seed=3)
    pt.denoise(iterations=4)
    stream.synchronize()
    assert _same_bits(out.cpu().numpy(), own)
    assert _same_bits(pt.denoised(), own)
    pt.bind_denoised(None)
    pt.set_stream(0)
    assert _same_bits(pt.denoised(), own)  # the own buffer still holds the first result
    pt.close()


def test_host_renderer_equals_path_tracer(srt):
    w, h = 160, 90
    scene = srt.host.Scene(scene_path("Scene1"))
    r = srt.host.Renderer(w, h)
    r.set_scene(scene)
    r.render_samples(4)
    r.denoise()
    got = r.denoised()
    acc = r.accumulator()
    g = {k: r.gbuffer(k) for k in NAMES}
    r.close()
    pt = srt.PathTracer(w, h)
    keep = _bind(pt, g["object"], g["normal_depth"], g["position"], g["albedo"])
    pt.write_accumulator(acc)
    pt.denoise(gbuffer=False)
    assert _same_bits(pt.denoised(), got)
    pt.close()
    del keep


def _ppm_rgb(path, w, h):
    data = open(path, "rb").read()
    head = b"P6\n%d %d\n255\n" % (w, h)
    assert data.startswith(head)
    return np.frombuffer(data[len(head):], np.uint8).reshape(h, w, 3)


def test_cli_writes_the_denoised_ppm(srt, tmp_path):
    w, h = 160, 90
    base = [CLI, "--scene", scene_path("Scene1"), "--width", str(w), "--height", str(h), "--spp", "4", "--bounces", "2"]
    r1 = subprocess.run(base + ["--out", str(tmp_path / "a.ppm")], capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr[-2000:]
    r2 = subprocess.run(base + ["--out", str(tmp_path / "b.ppm"), "--denoise", str(tmp_path / "d.ppm")], capture_output=True,
                        text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr[-2000:]
    assert (tmp_path / "a.ppm").read_bytes() == (tmp_path / "b.ppm").read_bytes()
    # the host layer's renderer with the CLI's settings, denoised with the defaults, tone-mapped and flipped to top-down rows
    scene = srt.host.Scene(scene_path("Scene1"))
    r = srt.host.Renderer(w, h)
    r.set_scene(scene)
    r.settings(fov=55, max_bounces=2, seed=0)
    r.render_samples(4, count_rays=True)
    r.denoise()
    px = tone_map(r.denoised())[::-1]
    r.close()
    want = np.stack([(px >> 16) & 255, (px >> 8) & 255, px & 255], -1).astype(np.uint8)
    assert np.array_equal(_ppm_rgb(tmp_path / "d.ppm", w, h), want)
    assert not np.array_equal(_ppm_rgb(tmp_path / "d.ppm", w, h), _ppm_rgb(tmp_path / "a.ppm", w, h))
    r3 = subprocess.run(base + ["--devices", "0,0", "--out", str(tmp_path / "c.ppm"), "--denoise", str(tmp_path / "e.ppm")],
                        capture_output=True, text=True, timeout=300)
    assert r3.returncode != 0 and "one device" in r3.stderr and not (tmp_path / "e.ppm").exists()
