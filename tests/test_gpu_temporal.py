"""Temporal reprojection (srt_temporal_accumulate) on the MI355X: the definition of include/srt_pathtrace.h against a float64
numpy restatement on analytic guides and known cameras, the invariants on real renders (misses, alpha, resets, invalidation,
disocclusion, the running mean of a still camera, determinism, the framebuffer flag, non-interference), errors, the noise it
removes from a moving camera, and the layers above (PathTracer, PathTraceRenderer, srt_render --temporal, srt_viewer T mode)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
VIEWER = os.path.join(ROOT, "software-raytracer_amd", "srt_viewer")
REL_TOL = 1e-4
GUIDES = ["object", "normal_depth", "position"]


# ---- cameras ------------------------------------------------------------------------------------------------------------
def camera(srt, pos, yaw_deg=0.0, fov=55, basis=None):
    """An srt_camera at pos, turned by yaw_deg about world up (or with an explicit right / up / forward basis)."""
    if basis is None:
        a = math.radians(yaw_deg)
        basis = [(math.cos(a), 0.0, -math.sin(a)), (0.0, 1.0, 0.0), (math.sin(a), 0.0, math.cos(a))]
    c = srt.Camera()
    c.position = (C.c_float * 3)(*[float(v) for v in pos])
    c.right = (C.c_float * 3)(*[float(v) for v in basis[0]])
    c.up = (C.c_float * 3)(*[float(v) for v in basis[1]])
    c.forward = (C.c_float * 3)(*[float(v) for v in basis[2]])
    c.fov_degrees = int(fov)
    return c


def ray_basis(cam, w, h):
    """The float32 columns right * rd, up * ld, forward * clip that srt_render folds (srt_capi.hip, fold_camera)."""
    f32 = np.float32
    clip = f32(0.01)
    aspect = f32(w) / f32(h)
    hfov = f32(cam.fov_degrees * 3.14159265358979323846 / 180.0)
    t = f32(math.tan(float(hfov / f32(2))))
    rd, ld = (clip * t) * aspect, clip * t
    r = np.array(cam.right[:], f32) * rd
    u = np.array(cam.up[:], f32) * ld
    f = np.array(cam.forward[:], f32) * clip
    return np.stack([r, u, f], 1).astype(np.float64)


# ---- analytic guides ----------------------------------------------------------------------------------------------------
SPHERES = [((0.3, 0.0, 4.0), 0.8), ((-1.2, -0.3, 6.0), 1.0), ((1.6, 0.4, 7.0), 0.9)]


def cast(cam, w, h):
    """First hits of the primary rays of `cam` on a ground plane y = -1 (object 0) and three spheres (objects 1..3), in float64,
    returned as the G-buffer's float32 guides (object, normal_depth, position), scene rows.  Rays that go up past the spheres
    miss."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    B = ray_basis(cam, w, h)
    nx, ny = xs / w * 2 - 1, ys / h * 2 - 1
    d = nx[..., None] * B[:, 0] + ny[..., None] * B[:, 1] + B[:, 2]
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    o = np.array(cam.position[:], np.float64)
    best = np.full((h, w), np.inf)
    obj = np.full((h, w), -1, np.int32)
    nrm = np.zeros((h, w, 3))
    with np.errstate(all="ignore"):
        t = (-1.0 - o[1]) / d[..., 1]
        take = (t > 1e-4) & (t < best)
        best = np.where(take, t, best)
        obj[take] = 0
        nrm[take] = (0.0, 1.0, 0.0)
        for k, (c, r) in enumerate(SPHERES):
            oc = o - np.array(c)
            b = np.sum(d * oc, axis=2)
            disc = b * b - (np.dot(oc, oc) - r * r)
            t = -b - np.sqrt(disc)
            take = (disc > 0) & (t > 1e-4) & (t < best)
            best = np.where(take, t, best)
            obj[take] = k + 1
            p = o + t[..., None] * d
            nrm = np.where(take[..., None], (p - np.array(c)) / r, nrm)
    hit = obj >= 0
    p = o + np.where(hit, best, 0)[..., None] * d
    nd = np.zeros((h, w, 4), np.float32)
    nd[..., :3] = nrm
    nd[..., 3] = np.where(hit, best, np.inf)
    pos = np.zeros((h, w, 4), np.float32)
    pos[..., :3] = np.where(hit[..., None], p, 0)
    pos[..., 3] = hit
    return obj, nd, pos


# ---- the definition -----------------------------------------------------------------------------------------------------
def exact_f32_dot(a, b):
    """Where a . b (float32 values, last axis 3) is exact in float32 whatever the order and fusing of its operations: every
    product and the running sums x, x + y, x + y + z are float32 values."""
    t = a * b
    parts = [t[..., 0], t[..., 1], t[..., 2], t[..., 0] + t[..., 1], t[..., 0] + t[..., 1] + t[..., 2]]
    with np.errstate(all="ignore"):
        return np.logical_and.reduce([np.isfinite(v) & (v.astype(np.float32).astype(np.float64) == v) for v in parts])


def reference(acc, obj, nd, pos, hist, n, max_samples, sigma_t, thr):
    """The blend of include/srt_pathtrace.h in float64.  hist: None (no history) or dict(cam, color (H,W,4) f32 with rgb = the
    previous result, L (H,W), obj, nd, pos).  Returns (result rgb, L, sensitive, scale, counted W, footprint of other objects
    only)."""
    H, W = obj.shape
    hit = obj >= 0
    out = acc[..., :3].astype(np.float64).copy()
    L = np.where(hit, float(n), 0.0)
    sens = np.zeros((H, W), bool)
    scale = np.max(np.abs(acc[..., :3]), axis=2).astype(np.float64)
    sw = np.zeros((H, W))
    others = np.zeros((H, W), bool)
    if hist is None:
        return out, L, sens, scale, sw, others
    Bi = np.linalg.inv(ray_basis(hist["cam"], W, H)).astype(np.float32).astype(np.float64)
    rel = pos[..., :3].astype(np.float64) - np.array(hist["cam"].position[:], np.float32).astype(np.float64)
    abg = rel @ Bi.T
    a, b, g = abg[..., 0], abg[..., 1], abg[..., 2]
    with np.errstate(all="ignore"):
        u = (a / g + 1) * W / 2
        v = (b / g + 1) * H / 2
    front = hit & (g > 0)
    sens |= hit & (np.abs(g) <= 1e-3 * np.linalg.norm(rel, axis=2))
    for e in (-1.0, 0.0, W - 1.0, float(W)):
        sens |= front & (np.abs(u - e) <= 1e-3)
    for e in (-1.0, 0.0, H - 1.0, float(H)):
        sens |= front & (np.abs(v - e) <= 1e-3)
    ok = front & (u > -1) & (u < W) & (v > -1) & (v < H)
    uu, vv = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
    x0, y0 = np.floor(uu).astype(np.int64), np.floor(vv).astype(np.int64)
    fx, fy = uu - x0, vv - y0
    n_p, d_p, x_p = nd[..., :3].astype(np.float64), nd[..., 3].astype(np.float64), pos[..., :3].astype(np.float64)
    tol = sigma_t * d_p
    sc = np.zeros((H, W, 3))
    sl = np.zeros((H, W))
    inside_any = np.zeros((H, W), bool)
    same_any = np.zeros((H, W), bool)
    for k in range(4):
        qx, qy = x0 + (k & 1), y0 + (k >> 1)
        wq = np.where(k & 1, fx, 1 - fx) * np.where(k >> 1, fy, 1 - fy)
        inside = ok & (wq > 0) & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
        cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
        same = inside & (hist["obj"][cy, cx] == obj)
        inside_any |= inside
        same_any |= same
        dist = np.abs(np.sum(n_p * (hist["pos"][cy, cx, :3].astype(np.float64) - x_p), axis=2))
        dot = np.sum(n_p * hist["nd"][cy, cx, :3].astype(np.float64), axis=2)
        # (an infinite tolerance or threshold has no rounding band: |x - inf| <= 1e-3 * inf would mark every tap)
        sens |= same & np.isfinite(tol) & (np.abs(dist - tol) <= 1e-3 * tol)
        counted = same & (dist <= tol)
        if thr > -1:
            # a dot product that float32 computes exactly (an exact tie such as two equal axis normals) compares as here
            exact = exact_f32_dot(n_p, hist["nd"][cy, cx, :3].astype(np.float64))
            if math.isfinite(thr):
                sens |= counted & ~exact & (np.abs(dot - thr) <= 1e-3 * max(abs(thr), 1e-3))
            counted &= dot >= thr
        w = np.where(counted, wq, 0.0)
        hq = hist["color"][cy, cx, :3].astype(np.float64)
        sw += w
        sc += w[..., None] * np.where(counted[..., None], hq, 0.0)
        sl += w * np.where(counted, hist["L"][cy, cx], 0.0)
        scale = np.maximum(scale, np.where(counted, np.max(np.abs(hq), axis=2), 0.0))
    others = inside_any & ~same_any
    sens |= (sw > 0) & (sw < 1e-3)
    # (u, v) within rounding of a pixel: the float footprint may be the neighbouring one, which matters only when the taps of
    # large weight do not count
    near = (np.minimum(fx, 1 - fx) < 1e-4) | (np.minimum(fy, 1 - fy) < 1e-4)
    sens |= ok & near & (sw < 0.5)
    blend = sw > 0
    with np.errstate(all="ignore"):
        Hp = sc / sw[..., None]
        Lh = sl / sw
        Lb = np.minimum(Lh + n, max_samples)
        al = n / Lb
        res = (1 - al)[..., None] * Hp + al[..., None] * acc[..., :3].astype(np.float64)
    out = np.where(blend[..., None], res, out)
    L = np.where(blend, Lb, L)
    return out, L, sens, scale, sw, others


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


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _bind(pt, guides):
    import torch

    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:%d" % pt.device) for k, v in zip(GUIDES, guides)}
    torch.cuda.synchronize()
    for k, v in t.items():
        pt.bind_gbuffer(k, v)
    return t


PARAMS = [  # samples, max_samples, plane_tolerance, normal_threshold
    (1, 32.0, 0.02, 0.9), (2, 7.0, 0.05, -1.0), (1, float("inf"), 0.003, 0.99), (3, 3.0, 0.02, 0.5),
]
# translations, yaws, a change of fov, and all at once
MOVES = [((0.0, 0.0, 0.0), 0.0, 55), ((0.04, 0.01, 0.12), 0.0, 55), ((0.04, 0.01, 0.12), 2.5, 55), ((0.04, 0.01, 0.12), 2.5, 49),
         ((-0.1, 0.03, 0.2), -1.5, 62), ((-0.1, 0.03, 0.2), -1.5, 62)]


@pytest.mark.parametrize("w,h", [(67, 45), (256, 160)])
@pytest.mark.parametrize("n,max_samples,sigma_t,thr", PARAMS)
def test_blend_matches_the_definition(srt, w, h, n, max_samples, sigma_t, thr):
    rng = np.random.default_rng(w + 7 * n)
    pt = srt.PathTracer(w, h)
    hist = None
    checked = blended = 0
    keep = None
    for k, (p, yaw, fov) in enumerate(MOVES):
        cam = camera(srt, p, yaw, fov)
        obj, nd, pos = cast(cam, w, h)
        keep = _bind(pt, (obj, nd, pos))
        pt.set_camera(cam)
        acc = np.concatenate([rng.uniform(0.02, 3.0, (h, w, 3)), rng.choice([0.0, 1.0], (h, w, 1))], -1).astype(np.float32)
        pt.write_accumulator(acc)
        pt.temporal(samples=n, max_samples=max_samples, plane_tolerance=sigma_t, normal_threshold=thr, gbuffer=False)
        got, L = pt.accumulator(), pt.history_length()
        ref, refL, sens, scale, sw, _ = reference(acc, obj, nd, pos, hist, n, max_samples, sigma_t, thr)
        hit = obj >= 0
        assert _same_bits(got[~hit], acc[~hit]) and np.all(L[~hit] == 0)
        assert _same_bits(got[..., 3], acc[..., 3]), "alpha was written"
        chk = hit & ~sens
        err = np.max(np.abs(got[..., :3].astype(np.float64) - ref), axis=2)
        bad = chk & (err > REL_TOL * scale)
        assert not bad.any(), (k, int(bad.sum()), float(np.max(err[chk] / scale[chk])))
        assert np.all(np.abs(L[chk] - refL[chk]) <= REL_TOL * refL[chk]), k
        kept = chk & (sw == 0)
        assert _same_bits(got[kept], acc[kept]) and np.all(L[kept] == n)
        checked += int(chk.sum())
        blended += int((chk & (sw > 0)).sum())
        hist = dict(cam=cam, color=got, L=L, obj=obj, nd=nd, pos=pos)
    assert blended > 0.3 * checked, (blended, checked)  # the moves keep most of the history
    pt.close()
    del keep


# ---- real renders ---------------------------------------------------------------------------------------------------------
def _scene_tracer(srt, oracle, name, w, h):
    oarr, cnt = oracle.make_objects(oracle.load_scene_json_py(scene_path(name)))
    pt = srt.PathTracer(w, h)
    pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), cnt)
    pt.set_camera(srt.default_camera())
    return pt, oarr, cnt


def _frame(pt, cam, spp, bounces, seed, **kw):
    pt.set_camera(cam)
    pt.render(spp=spp, bounces=bounces, seed=seed)
    pt.render_gbuffer()
    acc = pt.accumulator()
    pt.temporal(samples=spp, gbuffer=False, **kw)
    return acc


def _guides(pt):
    return tuple(pt.gbuffer(k) for k in GUIDES)


@pytest.mark.parametrize("name", ["Scene1", "Scene_indirect"])
def test_invariants_on_real_renders(srt, oracle, name):
    w, h = 160, 96
    pt, oarr, cnt = _scene_tracer(srt, oracle, name, w, h)
    cams = [camera(srt, (0.02 * k, 0.0, 0.05 * k), 0.4 * k) for k in range(4)]
    # the first call and SRT_TEMPORAL_RESET keep every input bit, L = samples on hits, 0 on misses
    for k, reset in ((0, False), (1, True)):
        acc = _frame(pt, cams[k], 2, 4, k, reset=reset)
        obj = pt.gbuffer("object")
        assert _same_bits(pt.accumulator(), acc)
        assert np.array_equal(pt.history_length(), np.where(obj >= 0, 2.0, 0.0).astype(np.float32))
    # a move: misses and alpha keep their bits, pixels whose footprint only meets other objects keep theirs with L = n
    prev = dict(cam=cams[1], color=pt.accumulator(), L=pt.history_length())
    prev.update(zip(("obj", "nd", "pos"), _guides(pt)))
    acc = _frame(pt, cams[2], 2, 4, 2)
    got, L = pt.accumulator(), pt.history_length()
    obj, nd, pos = _guides(pt)
    assert _same_bits(got[obj < 0], acc[obj < 0]) and np.all(L[obj < 0] == 0)
    assert _same_bits(got[..., 3], acc[..., 3])
    ref, refL, sens, scale, sw, others = reference(acc, obj, nd, pos, prev, 2, 32.0, 0.02, 0.9)
    chk = (obj >= 0) & ~sens
    assert np.all(np.max(np.abs(got[..., :3] - ref), axis=2)[chk] <= REL_TOL * scale[chk])
    dis = chk & others
    assert dis.sum() > 0, "no disocclusion in the move"
    assert _same_bits(got[dis], acc[dis]) and np.all(L[dis] == 2)
    assert (chk & (sw > 0)).sum() > 0.5 * chk.sum()
    # srt_set_scene, srt_set_meshes and srt_set_environment each drop the history: the next call is a reset
    for drop in ("scene", "meshes", "environment"):
        _frame(pt, cams[2], 2, 4, 3)
        assert (pt.history_length() > 2).any()
        if drop == "scene":
            pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), cnt)
        elif drop == "meshes":
            pt.set_meshes([], 0)
        else:
            pt.set_environment(srt.default_environment())
        acc = _frame(pt, cams[3], 2, 4, 4)
        assert _same_bits(pt.accumulator(), acc), drop
        obj = pt.gbuffer("object")
        assert np.array_equal(pt.history_length(), np.where(obj >= 0, 2.0, 0.0).astype(np.float32)), drop
    # srt_set_camera alone keeps it
    _frame(pt, cams[2], 2, 4, 5)
    assert (pt.history_length() > 2).any()
    pt.close()


@pytest.mark.parametrize("name", ["Scene1", "Scene_indirect"])
def test_still_camera_is_the_running_mean(srt, oracle, name):
    w, h = 128, 80
    pt, _, _ = _scene_tracer(srt, oracle, name, w, h)
    K, n = 6, 2
    accs = []
    for k in range(K):
        accs.append(_frame(pt, srt.default_camera(), n, 4, 100 + k, max_samples=float(K * n)))
    got, L = pt.accumulator(), pt.history_length()
    obj = pt.gbuffer("object")
    hit = obj >= 0
    mean = np.mean(np.stack(accs).astype(np.float64), axis=0)
    err = np.abs(got[..., :3] - mean[..., :3])[hit]
    # relative to the largest colour of the pixel and its neighbours over the K frames (the reprojection of a still camera
    # lands within a rounding error of the pixel itself, so a neighbour may take a weight of that size)
    m = np.max(np.abs(np.stack(accs)[..., :3]), axis=(0, 3))
    p = np.pad(m, 1)
    s = np.max(np.stack([p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]), axis=0)[hit]
    assert np.all(err.max(axis=1) <= REL_TOL * np.maximum(s, 1e-6)), float(np.max(err.max(axis=1) / np.maximum(s, 1e-6)))
    assert np.allclose(L[hit], K * n, rtol=1e-5)
    pt.close()


def test_determinism_framebuffer_and_non_interference(srt, oracle):
    w, h = 200, 120
    fields = ("rays", "sample_chunks", "tile_rows", "chunk_samples", "shape_source", "path_samples")
    cams = [camera(srt, (0.03 * k, 0.0, 0.04 * k), 0.5 * k) for k in range(3)]
    runs = []
    for with_temporal in (False, True, True):
        pt, _, _ = _scene_tracer(srt, oracle, "Scene1", w, h)
        out = []
        for k, cam in enumerate(cams):
            pt.set_camera(cam)
            pt.render(spp=2, bounces=4, seed=k, count_rays=True, count_work=True)
            first = pt.stats()
            pt.render_gbuffer()
            if with_temporal:
                g = {n: pt.gbuffer(n) for n in ("object", "normal_depth", "position", "albedo")}
                fb0 = pt.framebuffer()
                last = k == len(cams) - 1
                pt.temporal(samples=2, gbuffer=False, framebuffer=last)
                res = pt.accumulator()
                if last:  # the framebuffer flag: exactly the render's packing of the result
                    assert np.array_equal(pt.framebuffer(), tone_map(res)[::-1])
                    assert not np.array_equal(pt.framebuffer(), fb0)
                else:
                    assert np.array_equal(pt.framebuffer(), fb0), "the framebuffer was written without SRT_TEMPORAL_FRAMEBUFFER"
                for n in g:
                    assert np.array_equal(pt.gbuffer(n).view(np.uint32), g[n].view(np.uint32)), n
                after = pt.stats()
                assert all(getattr(after, f) == getattr(first, f) for f in fields) and after.kernel_ms == first.kernel_ms
                out.append((res, pt.history_length()))
        pt.set_camera(cams[0])
        pt.render(spp=4, bounces=4, seed=9, count_rays=True, count_work=True)
        st = pt.stats()
        runs.append(([getattr(st, f) for f in fields], pt.work_counts().as_dict(), pt.framebuffer(), pt.accumulator(), out))
        pt.close()
    a, b, c = runs
    for x in (b, c):
        assert a[0] == x[0] and a[1] == x[1]
        assert np.array_equal(a[2], x[2]) and _same_bits(a[3], x[3])
    for (r1, l1), (r2, l2) in zip(b[4], c[4]):
        assert _same_bits(r1, r2) and _same_bits(l1, l2), "two identical sequences differ"


def test_errors(srt, oracle):
    w, h = 40, 24
    pt = srt.PathTracer(w, h)
    with pytest.raises(srt.SrtError) as e:
        pt.history_length()
    assert e.value.code == srt.capi.ERR_STATE
    pt.set_camera(srt.default_camera())
    with pytest.raises(srt.SrtError) as e:
        pt.temporal(gbuffer=False)
    assert e.value.code == srt.capi.ERR_STATE
    obj, nd, pos = cast(srt.default_camera(), w, h)
    keep = _bind(pt, (obj, nd, pos))
    pt.bind_gbuffer("position", None)  # never rendered
    with pytest.raises(srt.SrtError) as e:
        pt.temporal(gbuffer=False)
    assert e.value.code == srt.capi.ERR_STATE
    keep = _bind(pt, (obj, nd, pos))
    pt.temporal(gbuffer=False)
    pt.wait()
    bad = [dict(samples=0), dict(samples=4, max_samples=3.5), dict(max_samples=float("nan")), dict(plane_tolerance=0.0),
           dict(plane_tolerance=-0.1), dict(plane_tolerance=float("nan")), dict(normal_threshold=float("nan"))]
    for kw in bad:
        with pytest.raises(srt.SrtError) as e:
            pt.temporal(gbuffer=False, **kw)
        assert e.value.code == srt.capi.ERR_INVALID_ARG, kw
    p = srt.capi.temporal_params()
    p.flags = 4
    assert pt.L.srt_temporal_accumulate(pt._h, C.byref(p)) == srt.capi.ERR_INVALID_ARG
    pt.close()
    del keep
    # the handle's own guides rendered with another camera than the current one
    pt, _, _ = _scene_tracer(srt, oracle, "Scene1", w, h)
    pt.render_gbuffer()
    pt.set_camera(camera(srt, (0.1, 0.0, 0.0)))
    with pytest.raises(srt.SrtError) as e:
        pt.temporal(gbuffer=False)
    assert e.value.code == srt.capi.ERR_STATE
    pt.temporal()  # (renders the guides with the current camera first)
    pt.wait()
    pt.close()


# ---- value --------------------------------------------------------------------------------------------------------------
# measured on the MI355X with the defaults (profiles/temporal/temporal_quality.jsonl): MSE ratio 0.066 / 0.105,
# mean shift 0.28 % / 0.95 % (Scene1 / Scene_indirect; the plain 1-spp frame's mean is 2.5 % / 2.7 % off)
MSE_RATIO_MAX = 0.2
MEAN_SHIFT_MAX = 0.015


def moving_cameras(srt, frames):
    return [camera(srt, (0.004 * k, 0.0, 0.01 * k), 0.15 * k) for k in range(frames)]


@pytest.mark.parametrize("name", ["Scene1", "Scene_indirect"])
def test_it_keeps_samples_while_the_camera_moves(srt, oracle, name):
    w, h, bounces, frames = 320, 180, 8, 16
    pt, _, _ = _scene_tracer(srt, oracle, name, w, h)
    cams = moving_cameras(srt, frames)
    for k, cam in enumerate(cams):
        noisy = _frame(pt, cam, 1, bounces, 1000 + k)
    got = pt.accumulator()
    hit = pt.gbuffer("object") >= 0
    pt.render(spp=1024, bounces=bounces, seed=777)
    ref = pt.accumulator()
    tm = lambda a: (a[..., :3] / (1.0 + a[..., :3]))[hit].astype(np.float64)  # noqa: E731
    mse_noisy = float(np.mean((tm(noisy) - tm(ref)) ** 2))
    mse_t = float(np.mean((tm(got) - tm(ref)) ** 2))
    shift = abs(float(np.mean(got[..., :3][hit], dtype=np.float64)) / float(np.mean(ref[..., :3][hit], dtype=np.float64)) - 1)
    print("%s: mse 1 spp %.4g temporal %.4g ratio %.3f, mean shift %.4f" % (name, mse_noisy, mse_t, mse_t / mse_noisy, shift))
    assert mse_t <= MSE_RATIO_MAX * mse_noisy
    assert shift <= MEAN_SHIFT_MAX
    pt.close()


# ---- layers ---------------------------------------------------------------------------------------------------------------
CAM_RE = re.compile(r"camera((?: +[-+0-9.eE]+){12})")


def _parse_cameras(text):
    out = []
    for m in CAM_RE.finditer(text):
        v = [float(x) for x in m.group(1).split()]
        out.append((v[0:3], [v[3:6], v[6:9], v[9:12]]))
    return out


def path_tracer_sequence(srt, oracle, name, w, h, cams, spp, bounces, seed, denoise, denoise_every=False):
    """What RenderTemporalFrame does, through the C-ABI: frame k renders with seed + k and RESET, the guides, the reprojection
    (RESET on the first frame) and, with `denoise`, the denoiser into the framebuffer."""
    pt, _, _ = _scene_tracer(srt, oracle, name, w, h)
    for k, (p, basis) in enumerate(cams):
        pt.set_camera(camera(srt, p, basis=basis, fov=55))
        pt.render(spp=spp, bounces=bounces, seed=seed + k)
        last = k == len(cams) - 1
        dn = denoise and (denoise_every or last)
        pt.render_gbuffer(outputs=15 if dn else srt.capi.TEMPORAL_GUIDES)
        pt.temporal(samples=spp, max_samples=max(32.0, spp), reset=k == 0, framebuffer=not dn, gbuffer=False)
        if dn:
            pt.denoise(gbuffer=False, framebuffer=True)
    fb = pt.framebuffer()
    pt.close()
    return fb


def _ppm_rgb(path, w, h):
    data = open(path, "rb").read()
    head = b"P6\n%d %d\n255\n" % (w, h)
    assert data.startswith(head)
    return np.frombuffer(data[len(head):], np.uint8).reshape(h, w, 3)


def _rgb(fb):
    return np.stack([(fb >> 16) & 255, (fb >> 8) & 255, fb & 255], -1).astype(np.uint8)


@pytest.mark.parametrize("denoise", [False, True])
def test_layers_give_the_same_frame(srt, oracle, tmp_path, denoise):
    w, h, spp, bounces, seed, frames = 160, 90, 2, 3, 5, 5
    # srt_render --temporal
    cmd = [CLI, "--scene", scene_path("Scene1"), "--width", str(w), "--height", str(h), "--spp", str(spp), "--bounces", str(bounces),
           "--seed", str(seed), "--temporal", str(frames), "--move", "0.01,0.005,0.03", "--turn", "0.7", "--out", str(tmp_path / "t.ppm")]
    if denoise:
        cmd += ["--denoise", str(tmp_path / "d.ppm")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    cams = _parse_cameras(r.stderr)
    assert len(cams) == frames and cams[0][0] == [0.0, 0.0, 0.0] and cams[-1][0] != cams[0][0]
    plain = path_tracer_sequence(srt, oracle, "Scene1", w, h, cams, spp, bounces, seed, False)
    assert np.array_equal(_ppm_rgb(tmp_path / "t.ppm", w, h), _rgb(plain))
    want = plain
    if denoise:
        want = path_tracer_sequence(srt, oracle, "Scene1", w, h, cams, spp, bounces, seed, True)
        assert np.array_equal(_ppm_rgb(tmp_path / "d.ppm", w, h), _rgb(want))
        assert not np.array_equal(want, plain)
    # PathTraceRenderer::RenderTemporalFrame, the camera moved without Invalidate()
    scene = srt.host.Scene(scene_path("Scene1"))
    hr = srt.host.Renderer(w, h)
    hr.set_scene(scene)
    hr.settings(fov=55, max_bounces=bounces, seed=seed)
    for p, basis in cams:
        hr.move_camera(p, [x for row in basis for x in row])
        hr.render_temporal_frame(spp, denoise)
    hr.wait()
    got = hr.framebuffer()
    assert np.array_equal(got, path_tracer_sequence(srt, oracle, "Scene1", w, h, cams, spp, bounces, seed, denoise, denoise_every=True))
    assert np.array_equal(got, want)
    # Invalidate() drops the history, a camera move does not
    hr.invalidate()
    hr.render_temporal_frame(spp, False)
    assert np.all(hr.history_length()[hr.gbuffer("object") >= 0] == spp)
    hr.move_camera(cams[-1][0], [x for row in cams[-1][1] for x in row])
    hr.render_temporal_frame(spp, False)
    assert (hr.history_length() > spp).any()
    hr.close()
    bad = subprocess.run(cmd + ["--devices", "0,0"], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "one device" in bad.stderr


def test_viewer_temporal_mode(srt, oracle, tmp_path):
    w, h = 128, 72
    lines = ["press T", "frames 1", "camera", "hold D", "frames 1", "camera", "release D", "rmb down", "move 6 -2", "frames 1", "camera",
             "rmb up", "hold W", "frames 1", "camera", "frames 1", "camera", "save %s" % (tmp_path / "v.ppm")]
    script = tmp_path / "s.txt"
    script.write_text("\n".join(lines) + "\n")
    r = subprocess.run([VIEWER, "--scene", scene_path("Scene1"), "--width", str(w), "--height", str(h), "--script", str(script)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    cams = _parse_cameras(r.stdout)
    assert len(cams) == 5 and all(" temporal 1" in ln for ln in r.stdout.splitlines() if ln.startswith("camera"))
    # the viewer's defaults: FOV 55, MAXBOUNCES 2, seed 0, one sample per temporal frame
    want = path_tracer_sequence(srt, oracle, "Scene1", w, h, cams, 1, 2, 0, False)
    assert np.array_equal(_ppm_rgb(tmp_path / "v.ppm", w, h), _rgb(want))
