"""The first-hit, denoise and temporal kernels (and the render itself) at the edges of their contracts on the MI355X: frames of
one pixel, one row or one column and around the 8 x 8 tile, denoise levels up to 8, sigmas and tolerances at the ends of what
the calls accept on guides with exact ties, real G-buffers against the denoiser's definition, negative first-hit distances
(the camera inside a sphere) and a bound accumulator.  The float64 definitions are the ones of test_gpu_denoise.py,
test_gpu_temporal.py and test_gpu_gbuffer.py."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import scene_path
import test_gpu_denoise as dn
import test_gpu_temporal as tp
from test_gpu_gbuffer import _check_against_oracle, _scene1_with_mesh

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 37), (37, 1), (2, 3), (7, 5), (8, 8), (9, 9), (16, 16), (17, 15), (15, 17), (300, 1), (1, 300)]
NAMES = ["object", "normal_depth", "position", "albedo"]
ORACLE_THREADS = 16
INF = float("inf")
F32_MAX = float(np.finfo(np.float32).max)


# ---- scenes -------------------------------------------------------------------------------------------------------------
def _scene(oracle, kind):
    """Oracle arrays of Scene1, Scene3, Scene_indirect, "Scene1 mesh" (the r = 1 ball as the uv-sphere mesh) or "Scene1 inside"
    (Scene1 in an emissive sphere of radius 50 around the default camera: every first hit lies behind the camera, at a
    negative distance)."""
    meshes = None
    if kind == "Scene1 mesh":
        objs, meshes = _scene1_with_mesh(oracle)
    elif kind == "Scene1 inside":
        objs = oracle.load_scene_json_py(scene_path("Scene1"))
        objs.append(dict(type=oracle.OBJ_SPHERE, position=(0.0, 0.0, 0.0), radius=50.0, base=(0.7, 0.6, 0.5), emissive=(0.6, 0.5, 0.4)))
    else:
        objs = oracle.load_scene_json_py(scene_path(kind))
    oarr, n = oracle.make_objects(objs)
    sc = dict(oarr=oarr, n=n, meshes=None, keep=None)
    if meshes:
        marr, mn, keep = oracle.make_meshes(meshes)
        sc.update(meshes=(marr, mn), keep=keep)
    return sc


def _tracer(srt, sc, w, h, cam=None):
    pt = srt.PathTracer(w, h)
    if sc["meshes"]:
        pt.set_meshes(C.cast(sc["meshes"][0], C.POINTER(srt.Mesh)), sc["meshes"][1])
    pt.set_scene(C.cast(sc["oarr"], C.POINTER(srt.Object)), sc["n"])
    pt.set_camera(cam if cam is not None else srt.default_camera())
    return pt


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


# ---- 1. degenerate frame shapes: G-buffer and render against the oracle ---------------------------------------------------
@pytest.mark.parametrize("kind", ["Scene1", "Scene1 mesh"])
def test_gbuffer_matches_the_oracle_at_every_shape(srt, oracle, kind):
    import torch

    sc = _scene(oracle, kind)
    cam = oracle.default_camera()
    hits = 0
    for w, h in SHAPES:
        pt = _tracer(srt, sc, w, h)
        pt.render_gbuffer()
        g = {k: pt.gbuffer(k) for k in NAMES}
        ys, xs = np.mgrid[0:h, 0:w]
        hits += _check_against_oracle(g, oracle, sc["oarr"], sc["n"], cam, w, h, xs.ravel(), ys.ravel(), meshes=sc["meshes"])[0]
        # one-row bands at memory rows 0 and H - 1 (scene rows H - 1 and 0) into buffers filled with a sentinel
        for r in sorted({0, h - 1}):
            bufs = {"object": torch.full((h, w), -7, dtype=torch.int32, device="cuda:0")}
            for k in NAMES[1:]:
                bufs[k] = torch.full((h, w, 4), 12345.0, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            for k in NAMES:
                pt.bind_gbuffer(k, bufs[k])
            pt.render_gbuffer(rows=(r, r + 1))
            pt.wait()
            row = np.zeros(h, bool)
            row[h - 1 - r] = True
            for k in NAMES:
                got = bufs[k].cpu().numpy()
                assert np.array_equal(got[row].view(np.uint32), g[k][row].view(np.uint32)), (w, h, r, k)
                assert np.all(got[~row] == (-7 if k == "object" else 12345.0)), (w, h, r, k)
            for k in NAMES:
                pt.bind_gbuffer(k, None)
        pt.close()
    assert hits > 0


@pytest.mark.parametrize("kind", ["Scene1", "Scene1 mesh"])
@pytest.mark.parametrize("w,h", SHAPES)
def test_render_matches_the_oracle_at_every_shape(srt, oracle, kind, w, h):
    """1, 16 (the tile-height rule) and 70 samples (sample chunks), each followed by a resumed launch: accumulator bits,
    framebuffer and ray count."""
    sc = _scene(oracle, kind)
    pt = _tracer(srt, sc, w, h)
    for spp in (1, 16, 70):
        oacc = None
        for kw in (dict(spp=spp, bounces=4, seed=spp + w), dict(spp=3, bounces=4, seed=spp + w, first_sample=spp + 1, reset=False)):
            ofb, oacc, orays = oracle.render(sc["oarr"], sc["n"], oracle.default_environment(), oracle.default_camera(), w, h,
                                             accumulator=oacc, meshes=sc["meshes"], threads=ORACLE_THREADS, **kw)
            pt.render(count_rays=True, **kw)
            acc = pt.accumulator()
            bad = (acc.view(np.uint32) != oacc.view(np.uint32)).any(-1)
            assert not bad.any(), (kw, int(bad.sum()), np.argwhere(bad)[:8].tolist())
            assert np.array_equal(pt.framebuffer(), ofb), kw
            assert pt.stats().rays == orays, kw
    pt.close()


# ---- the denoiser's definition, and which pixels it cannot decide --------------------------------------------------------
def _demod(alb, albedo, shape):
    if not albedo:
        return np.ones(shape + (3,))
    a = alb[..., :3]
    return np.where(a >= np.float32(1e-3), a.astype(np.float64), 1.0)


def _exact_f32(terms):
    """Where sum(terms) (float64 arrays of products of float32 values) is exact in float32 whatever the order and fusing of its
    operations: every term and the running sums are float32 values."""
    parts = list(terms) + [sum(terms[:k]) for k in range(2, len(terms) + 1)]
    with np.errstate(all="ignore"):
        return np.logical_and.reduce([np.isfinite(v) & (v.astype(np.float32).astype(np.float64) == v) for v in parts])


def _log_interval(lo, hi, sign):
    """The log of exp(-x) (sign +1) or exp(+x) (sign -1) for x in [lo, hi], with the hardware exp's error."""
    e = 2.0 ** -21
    return (-hi * (1 + e) - e, -lo * (1 - e) + e) if sign > 0 else (lo * (1 - e) - e, hi * (1 + e) + e)


def sensitive(acc, obj, nd, pos, alb, iterations, sigma_color, sigma_normal, sigma_plane, albedo):
    """The hit pixels whose result the definition cannot pin down to REL_TOL in float32: a level-i tap whose weight float32
    rounding can change enough to move the level's result by half of REL_TOL (a dot product within rounding of 1 under a
    huge exponent, a plane distance or colour difference within rounding of 0 under a tiny sigma, the kernel's scale that stops
    at FLT_MAX), or that can pass e^80; and every pixel that takes a tap which was sensitive at an earlier level.
    Exact ties (float32 computes the term exactly) are never sensitive."""
    H, W = obj.shape
    hit = obj >= 0
    m = _demod(alb, albedo, (H, W))
    n = nd[..., :3].astype(np.float64)
    d = nd[..., 3].astype(np.float64)
    x = pos[..., :3].astype(np.float64)
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        cin = acc[..., :3].astype(np.float64) / m
        s32 = np.float32(sigma_plane) * nd[..., 3]
        pscale = np.float32(1) / s32
    pscale = np.where(np.isinf(pscale), np.copysign(np.float32(F32_MAX), pscale), pscale).astype(np.float64)
    sens = np.zeros((H, W), bool)
    for i in range(iterations):
        with np.errstate(all="ignore"):
            out = dn.reference(acc, obj, nd, pos, alb, i + 1, sigma_color, sigma_normal, sigma_plane, albedo)[..., :3] / m
        s = 1 << i
        ctol = (2.0 ** -23 if i == 0 else 4e-6 * i) * np.abs(cin)  # the kernel's working colour against this one
        new = sens.copy()
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if not (dx or dy):
                    continue
                qy, qx = ys + s * dy, xs + s * dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                take = inside & hit & (obj[qy, qx] == obj)
                lo, hi = np.zeros((H, W)), np.zeros((H, W))
                with np.errstate(all="ignore"):
                    if sigma_normal > 0:
                        t = [n[..., k] * n[qy, qx, k] for k in range(3)]
                        dot = t[0] + t[1] + t[2]
                        err = np.where(_exact_f32(t), 0.0, 2.0 ** -23 * (np.abs(t[0]) + np.abs(t[1]) + np.abs(t[2])))
                        a, b = dot - err, dot + err
                        if math.isinf(sigma_normal):
                            l_lo = np.where(a > 1, INF, np.where(a == 1, 0.0, -INF))
                            l_hi = np.where(b > 1, INF, np.where(b == 1, 0.0, -INF))
                        else:
                            l_lo = np.where(a > 0, sigma_normal * np.log(np.maximum(a, 1e-300)), -INF)
                            l_hi = np.where(b > 0, sigma_normal * np.log(np.maximum(b, 1e-300)), -INF)
                            l_lo = np.where(np.isfinite(l_lo), l_lo - 2.0 ** -22 * np.abs(l_lo), l_lo)  # (log2, exp2)
                            l_hi = np.where(np.isfinite(l_hi), l_hi + 2.0 ** -22 * np.abs(l_hi), l_hi)
                        lo, hi = lo + l_lo, hi + l_hi
                    if sigma_plane > 0:
                        dl = [x[qy, qx, k] - x[..., k] for k in range(3)]
                        t = [n[..., k] * dl[k] for k in range(3)]
                        pd = np.abs(t[0] + t[1] + t[2])
                        exact = _exact_f32(t) & np.logical_and.reduce([dl[k].astype(np.float32).astype(np.float64) == dl[k] for k in range(3)])
                        err = np.where(exact, 0.0, 2.0 ** -22 * (np.abs(t[0]) + np.abs(t[1]) + np.abs(t[2])))
                        xdef = pd / np.abs(sigma_plane * d)
                        k_lo = np.maximum(pd - err, 0.0) * np.abs(pscale) * (1 - 2.0 ** -22)
                        k_hi = (pd + err) * np.abs(pscale) * (1 + 2.0 ** -22)
                        xl, xh = np.fmin(xdef, k_lo), np.fmax(xdef, k_hi)
                        l_lo, l_hi = _log_interval(xl, xh, 1)
                        n_lo, n_hi = _log_interval(xl, xh, -1)
                        neg = d < 0
                        lo, hi = lo + np.where(neg, n_lo, l_lo), hi + np.where(neg, n_hi, l_hi)
                    if sigma_color > 0:
                        cq = cin[qy, qx]
                        dc = np.abs(cin - cq)
                        tol = np.where(dc == 0 if i == 0 else False, 0.0, ctol + ctol[qy, qx])
                        e_lo = np.sum(np.maximum(dc - tol, 0.0) ** 2, axis=2)
                        e_hi = np.sum((dc + tol) ** 2, axis=2)
                        scale = float(np.float32(1) / np.float32(np.float32(np.float32(sigma_color) * np.float32(2.0 ** -i)) ** 2))
                        scale = min(scale, F32_MAX)
                        xdef = np.sum(dc ** 2, axis=2) / (sigma_color * 2.0 ** -i) ** 2
                        k_lo = np.where(e_lo < 1e-44, 0.0, e_lo * scale * (1 - 2.0 ** -21))
                        k_hi = e_hi * scale * (1 + 2.0 ** -21)
                        l_lo, l_hi = _log_interval(np.fmin(xdef, k_lo), np.fmax(xdef, k_hi), 1)
                        lo, hi = lo + l_lo, hi + l_hi
                    # what the uncertain part of the tap's weight can move the result by (the weights sum to at least the
                    # centre's 36/256), against half of REL_TOL; a weight past e^80 is sensitive whatever it multiplies
                    unc = np.where(hi == -INF, 0.0, -np.expm1(lo - hi) * np.exp(np.minimum(hi, 80.0))) * (dn.H5[dx + 2] * dn.H5[dy + 2] / (36 / 256))
                    move = unc[..., None] * np.abs(cin[qy, qx] - out)  # per channel, as the error is measured
                    loose = ~(np.all(move <= 0.5 * dn.REL_TOL * np.maximum(np.abs(out), 1e-6), axis=2) & (hi <= 80))
                new |= take & (loose | sens[qy, qx])
        sens = new
        cin = out
    return sens & hit


def check_denoise(got, acc, obj, nd, pos, alb, params, min_checked=0.5):
    """The result against the definition on the hit pixels that are not sensitive (at least `min_checked` of them); alpha and
    miss pixels bit for bit.  Returns (worst relative error, checked, sensitive)."""
    it, sc, sn, sx, albedo = params
    hit = obj >= 0
    ref = dn.reference(acc, obj, nd, pos, alb, it, sc, sn, sx, albedo)
    sens = sensitive(acc, obj, nd, pos, alb, it, sc, sn, sx, albedo)
    chk = hit & ~sens
    assert chk.sum() >= min_checked * hit.sum(), (params, int(chk.sum()), int(hit.sum()))
    err = 0.0
    if chk.any():
        g, r = got[chk][:, :3].astype(np.float64), ref[chk][:, :3]
        with np.errstate(all="ignore"):
            rel = np.abs(g - r) / np.maximum(np.abs(r), 1e-6)
        assert np.all(np.isfinite(g)), (params, "non-finite result at %d checked pixels" % int((~np.isfinite(g)).any(1).sum()))
        err = float(np.max(rel))
        assert err <= dn.REL_TOL, (params, err, int((rel > dn.REL_TOL).any(1).sum()))
    assert _same_bits(got[..., 3], acc[..., 3]), "alpha is not the input's"
    assert _same_bits(got[~hit], acc[~hit]), "miss pixels are not the input"
    return err, int(chk.sum()), int(sens.sum())


def _shape_guides(w, h, seed):
    """synthetic() guides of a small frame with at least one hit pixel."""
    acc, obj, nd, pos, alb = dn.synthetic(w, h, seed=seed, n_objects=min(5, max(1, w * h // 4)))
    if not (obj >= 0).any():
        acc, obj, nd, pos, alb = dn.synthetic(w, h, seed=seed, n_objects=1, miss_fraction=0.0)
    if not (obj >= 0).any():  # (the corner rule of synthetic() can miss every pixel of a one-column frame)
        obj[...] = 0
        nd[..., :3] = np.array([0.0, 0.6, 0.8], np.float32)
        nd[..., 3] = 3.0
        pos[..., 3] = 1.0
        alb[..., :3] = 0.5
    return acc, obj, nd, pos, alb


# ---- 1. degenerate frame shapes: denoiser and reprojection ----------------------------------------------------------------
DENOISE_SHAPE_PARAMS = [(0.0, 32.0, 0.02, True), (0.5, 128.0, 0.05, False)]


def test_denoise_matches_the_definition_at_every_shape(srt):
    cases = [(w, h, _shape_guides(w, h, seed=w * 31 + h)) for w, h in SHAPES]
    acc, obj, nd, pos, alb = _shape_guides(1, 1, seed=5)
    assert obj[0, 0] >= 0
    miss = (acc.copy(), np.full((1, 1), -1, np.int32), np.array([[[0, 0, 0, INF]]], np.float32), np.zeros((1, 1, 4), np.float32),
            np.zeros((1, 1, 4), np.float32))
    cases.append((1, 1, miss))
    worst = 0.0
    for w, h, (acc, obj, nd, pos, alb) in cases:
        pt = srt.PathTracer(w, h)
        keep = dn._bind(pt, obj, nd, pos, alb)
        pt.write_accumulator(acc)
        for it in range(1, 9):
            for sc, sn, sx, albedo in DENOISE_SHAPE_PARAMS:
                pt.denoise(iterations=it, sigma_color=sc, sigma_normal=sn, sigma_plane=sx, albedo=albedo, gbuffer=False)
                err, _, _ = check_denoise(pt.denoised(), acc, obj, nd, pos, alb, (it, sc, sn, sx, albedo), min_checked=0.8)
                worst = max(worst, err)
        pt.close()
        del keep
    print("denoise at every shape: max relative error %.3g" % worst)


def _temporal_sequence(srt, pt, w, h, n, max_samples, sigma_t, thr, seed):
    """test_blend_matches_the_definition's sequence along MOVES on cast() guides: per frame (checked, blended, hit, kept)
    after the per-pixel checks against the definition."""
    rng = np.random.default_rng(seed)
    hist, keep, out = None, None, []
    for k, (p, yaw, fov) in enumerate(tp.MOVES):
        cam = tp.camera(srt, p, yaw, fov)
        obj, nd, pos = tp.cast(cam, w, h)
        keep = tp._bind(pt, (obj, nd, pos))
        pt.set_camera(cam)
        acc = np.concatenate([rng.uniform(0.02, 3.0, (h, w, 3)), rng.choice([0.0, 1.0], (h, w, 1))], -1).astype(np.float32)
        pt.write_accumulator(acc)
        pt.temporal(samples=n, max_samples=max_samples, plane_tolerance=sigma_t, normal_threshold=thr, reset=k == 0, gbuffer=False)
        got, L = pt.accumulator(), pt.history_length()
        ref, refL, sens, scale, sw, _ = tp.reference(acc, obj, nd, pos, hist, n, max_samples, sigma_t, thr)
        hit = obj >= 0
        what = (w, h, k, n, max_samples, sigma_t, thr)
        assert _same_bits(got[~hit], acc[~hit]) and np.all(L[~hit] == 0), what
        assert _same_bits(got[..., 3], acc[..., 3]), what
        chk = hit & ~sens
        err = np.max(np.abs(got[..., :3].astype(np.float64) - ref), axis=2)
        bad = chk & ~(err <= tp.REL_TOL * scale)
        assert not bad.any(), (what, int(bad.sum()))
        assert np.all(np.abs(L[chk] - refL[chk]) <= tp.REL_TOL * refL[chk]), what
        kept = chk & (sw == 0)
        assert _same_bits(got[kept], acc[kept]) and np.all(L[kept] == n), what
        unchanged = hit & _bits_equal_px(got, acc) & (L == n)
        out.append(dict(checked=int(chk.sum()), blended=int((chk & (sw > 0)).sum()), hit=int(hit.sum()), unchanged=int(unchanged.sum()),
                        ground=int((chk & (obj == 0)).sum()), ground_blended=int((chk & (sw > 0) & (obj == 0)).sum())))
        hist = dict(cam=cam, color=got, L=L, obj=obj, nd=nd, pos=pos)
    del keep
    return out


def _bits_equal_px(a, b):
    return np.all(np.asarray(a, np.float32).view(np.uint32) == np.asarray(b, np.float32).view(np.uint32), axis=-1)


def test_reprojection_matches_the_definition_at_every_shape(srt):
    checked = blended = 0
    for w, h in SHAPES:
        pt = srt.PathTracer(w, h)
        for n, max_samples, sigma_t, thr in ((1, 32.0, 0.02, 0.9), (2, 7.0, 0.05, -1.0)):
            for f in _temporal_sequence(srt, pt, w, h, n, max_samples, sigma_t, thr, seed=w + 7 * h):
                checked += f["checked"]
                blended += f["blended"]
        pt.close()
    print("reprojection at every shape: %d checked, %d blended" % (checked, blended))
    assert checked > 2000 and blended > 0.3 * checked


# ---- 1. degenerate shapes: row bands of the multi-device renderer ----------------------------------------------------------
@pytest.mark.parametrize("equal", [True, False])
@pytest.mark.parametrize("n_parts,h", [(1, 1), (3, 3), (7, 7), (1, 2), (3, 4), (7, 8)])
def test_multi_renderer_with_one_row_bands(srt, oracle, n_parts, h, equal):
    w, spp = 9, 3
    scene = srt.host.Scene(scene_path("Scene1"))
    m = srt.host.MultiRenderer([0] * n_parts, w, h)
    m.set_scene(scene)
    m.configure(fov=55, max_bounces=4, seed=11)
    if equal:
        m.use_equal_bands()
    else:
        m.balance_bands()
    m.render_samples(spp)
    bands = [m.band(i) for i in range(n_parts)]
    assert bands[0][0] == 0 and bands[-1][1] == h and all(bands[i][1] == bands[i + 1][0] for i in range(n_parts - 1)), bands
    assert all(b > a for a, b in bands), bands
    fb = m.framebuffer()
    objs, n = scene.objects_copy()
    pt = srt.PathTracer(w, h)
    pt.set_scene(objs, n)
    pt.set_camera(srt.default_camera())
    pt.render(spp=spp, bounces=4, seed=11)
    assert np.array_equal(fb, pt.framebuffer()), bands
    ofb, _, _ = oracle.render(C.cast(objs, C.POINTER(oracle.Object)), n, oracle.default_environment(), oracle.default_camera(), w, h,
                              spp=spp, bounces=4, seed=11, threads=ORACLE_THREADS)
    assert np.array_equal(fb, ofb), bands
    m.render_samples(2)  # resumed on every band
    pt.render(spp=2, bounces=4, seed=11, first_sample=spp + 1, reset=False)
    assert np.array_equal(m.framebuffer(), pt.framebuffer()), bands
    m.close()
    pt.close()


# ---- 3. parameter edges on guides with exact ties ------------------------------------------------------------------------
def tie_guides(w, h, seed):
    """synthetic() guides plus one more object (a band of rows) whose normals are exactly (0, 1, 0), whose points share one y
    bit for bit and whose colour and albedo are constant: n.n == 1, n.(x_q - x_p) == 0 and c_p - c_q == 0 occur exactly.
    The other objects' neighbouring normals stay clearly below a dot product of 1."""
    acc, obj, nd, pos, alb = dn.synthetic(w, h, seed=seed, n_objects=4)
    ys, xs = np.mgrid[0:h, 0:w]
    band = (ys >= h // 3) & (ys < h // 3 + max(h // 4, 3)) & (xs >= w // 8)
    obj[band] = 4
    nd[band] = np.array([0.0, 1.0, 0.0, 0.0], np.float32)
    nd[..., 3] = np.where(band, np.float32(2.5) + np.float32(0.01) * xs, nd[..., 3])
    pos[band] = np.stack([np.float32(0.01) * xs, np.full((h, w), -1.25), np.float32(2.0) + np.float32(0.02) * ys, np.ones((h, w))],
                         -1).astype(np.float32)[band]
    alb[band] = np.array([0.3, 0.5, 0.7, 0.0], np.float32)
    acc[band] = np.array([0.8, 1.7, 0.25, 1.0], np.float32)
    return acc, obj, nd, pos, alb


def _f32(v):
    return float(np.float32(v))


DENOISE_EDGES = ([(_f32(v), 32.0, 0.02) for v in (1e-45, 1e-30, 1e-19, 4e-19, 1e38, INF)] +
                 [(0.5, _f32(v), 0.02) for v in (1e-30, 1e30, INF)] +
                 [(0.5, 32.0, _f32(v)) for v in (1e-45, 1e-39, 1e-30, 1e30, INF)])


@pytest.mark.parametrize("sc,sn,sx", DENOISE_EDGES, ids=["c%g-n%g-x%g" % e for e in DENOISE_EDGES])
def test_denoise_parameter_edges(srt, sc, sn, sx):
    w, h = 67, 45
    acc, obj, nd, pos, alb = tie_guides(w, h, seed=21)
    tie = obj == 4
    pt = srt.PathTracer(w, h)
    keep = dn._bind(pt, obj, nd, pos, alb)
    pt.write_accumulator(acc)
    for it in (4, 8):
        for albedo in (False, True):
            pt.denoise(iterations=it, sigma_color=sc, sigma_normal=sn, sigma_plane=sx, albedo=albedo, gbuffer=False)
            got = pt.denoised()
            err, checked, nsens = check_denoise(got, acc, obj, nd, pos, alb, (it, sc, sn, sx, albedo), min_checked=0.9)
            print("sigma_color %g sigma_normal %g sigma_plane %g L %d albedo %d: max relative error %.3g, %d checked, %d sensitive"
                  % (sc, sn, sx, it, albedo, err, checked, nsens))
            # the constant object stays constant whatever the weights
            assert np.max(np.abs(got[tie][:, :3] / np.array([0.8, 1.7, 0.25]) - 1)) <= 1e-6, (it, albedo)
    pt.close()
    del keep


NEXT_BELOW_1 = float(np.nextafter(np.float32(-1), np.float32(0)))
NEXT_ABOVE_1 = float(np.nextafter(np.float32(1), np.float32(2)))
TEMPORAL_EDGES = ([(1, 32.0, _f32(v), 0.9, "ground blends") for v in (1e-45, 1e-30)] +
                  [(1, 32.0, _f32(v), 0.9, "blend") for v in (1e30, INF)] +
                  [(1, 32.0, 0.02, v, "blend") for v in (-INF, -1.0, NEXT_BELOW_1)] + [(1, 32.0, 0.02, 1.0, "ground blends")] +
                  [(1, 32.0, 0.02, NEXT_ABOVE_1, "ground keeps"), (1, 32.0, 0.02, INF, "keep")] +
                  [(4, 4.0, 0.02, 0.9, "keep"), (1000, INF, 0.05, -1.0, "blend")])


@pytest.mark.parametrize("n,max_samples,sigma_t,thr,expect", TEMPORAL_EDGES, ids=["n%d-max%g-t%g-thr%r-%s" % e for e in TEMPORAL_EDGES])
def test_reprojection_parameter_edges(srt, n, max_samples, sigma_t, thr, expect):
    """The plane tolerance and the normal threshold at the ends of what the call accepts, max_samples == samples and a large
    samples, along MOVES on the analytic guides (the ground's normals are exactly (0, 1, 0) and its points share
    y = -1: n.n == 1 and n.(x_q - x_p) == 0 exactly).  A case that should blend blends at many checked pixels; one that should not leaves every hit pixel's bits and L = n."""
    w, h = 67, 45
    pt = srt.PathTracer(w, h)
    frames = _temporal_sequence(srt, pt, w, h, n, max_samples, sigma_t, thr, seed=3)
    pt.close()
    checked = sum(f["checked"] for f in frames[1:])
    blended = sum(f["blended"] for f in frames[1:])
    print("n %d max %g tolerance %g threshold %r: %d checked, %d blended" % (n, max_samples, sigma_t, thr, checked, blended))
    # (a threshold within rounding of 1 leaves the taps of the spheres to the sensitivity mask)
    cover = 0.6 if 0.999 <= thr <= 1.001 else 0.8
    assert checked >= cover * sum(f["hit"] for f in frames[1:]), (checked, [f["hit"] for f in frames])
    if expect == "blend":
        assert blended > 0.3 * checked, (blended, checked)
    elif expect == "ground blends":  # only the exact ties count: n.(x_q - x_p) == 0 or n.n == 1 on the ground
        ground = sum(f["ground"] for f in frames[1:])
        assert sum(f["ground_blended"] for f in frames[1:]) > 0.5 * ground > 0, frames
    elif expect == "keep":
        assert all(f["unchanged"] == f["hit"] for f in frames), frames
    else:  # normal_threshold just above 1: the ground's exact n.n == 1 never reaches it
        assert sum(f["ground_blended"] for f in frames) == 0 and checked > 0, frames


# ---- 4. real guides against the denoiser's definition --------------------------------------------------------------------
REAL_PARAMS = [  # iterations, sigma_color, sigma_normal, sigma_plane, albedo
    (4, 0.0, 32.0, 0.02, True), (4, 0.5, 32.0, 0.02, True), (8, 0.5, 32.0, 0.02, False),
    (4, _f32(1e-30), 32.0, 0.02, True), (8, _f32(4e-19), 32.0, 0.02, False), (4, 0.0, INF, 0.02, True), (8, 0.0, _f32(1e30), 0.02, False),
    (4, 0.0, 32.0, _f32(1e-45), True), (8, 0.5, 32.0, _f32(1e-39), True), (4, 0.0, 32.0, INF, False),
]


@pytest.mark.parametrize("kind", ["Scene_indirect", "Scene3", "Scene1 mesh", "Scene1 inside"])
def test_denoise_real_guides_match_the_definition(srt, oracle, kind):
    w, h = 160, 96
    sc = _scene(oracle, kind)
    pt = _tracer(srt, sc, w, h)
    pt.render(spp=4, bounces=4, seed=9)
    pt.render_gbuffer()
    acc = pt.accumulator()
    obj, nd, pos, alb = (pt.gbuffer(k) for k in NAMES)
    hit = obj >= 0
    assert hit.sum() > w * h // 4
    if kind == "Scene1 inside":
        ys, xs = np.mgrid[0:h, 0:w]
        g = dict(zip(NAMES, (obj, nd, pos, alb)))
        assert _check_against_oracle(g, oracle, sc["oarr"], sc["n"], oracle.default_camera(), w, h, xs.ravel(), ys.ravel())[0] == w * h
        assert np.all(nd[..., 3] < 0), "a first hit in front of the camera"
    worst = 0.0
    for params in REAL_PARAMS:
        it, sgc, sgn, sgx, albedo = params
        if kind == "Scene1 inside" and sgx < 1e-30:
            continue  # (behind the camera d_p < 0: the plane term is exp(+|n.dx| / (sigma_plane |d_p|)), inf for a tiny sigma)
        pt.denoise(iterations=it, sigma_color=sgc, sigma_normal=sgn, sigma_plane=sgx, albedo=albedo, gbuffer=False)
        # (a noisy 4-spp frame leaves more taps of the colour term within rounding of their result than synthetic guides)
        err, checked, nsens = check_denoise(pt.denoised(), acc, obj, nd, pos, alb, params, min_checked=0.1)
        worst = max(worst, err)
        print("%s %s: max relative error %.3g, %d checked, %d sensitive of %d hits" % (kind, params, err, checked, nsens, int(hit.sum())))
    print("%s: max relative error %.3g" % (kind, worst))
    if kind == "Scene1 inside":
        # a small move: the tolerance plane_tolerance * d_p is negative, so no tap counts; every hit keeps its bits, L = n
        pt.temporal(samples=4)
        pt.set_camera(tp.camera(srt, (0.03, 0.01, 0.05), 0.5))
        pt.render(spp=4, bounces=4, seed=10)
        before = pt.accumulator()
        pt.temporal(samples=4)
        o2 = pt.gbuffer("object")
        assert (o2 >= 0).all()
        assert _same_bits(pt.accumulator(), before) and np.all(pt.history_length() == 4)
    pt.close()


# ---- 5. a bound accumulator ------------------------------------------------------------------------------------------------
def test_bound_accumulator_through_reprojection_and_denoise(srt, oracle):
    import torch

    w, h = 120, 72
    sc = _scene(oracle, "Scene_indirect")
    cams = [tp.camera(srt, (0.0, 0.0, 0.0)), tp.camera(srt, (0.03, 0.0, 0.06), 0.6)]

    def sequence(pt):
        res = []
        for k, cam in enumerate(cams):
            pt.set_camera(cam)
            pt.render(spp=2, bounces=4, seed=k)
            pt.temporal(samples=2)
            pt.denoise(iterations=5, sigma_color=0.5)
            res.append((pt.accumulator(), pt.history_length(), pt.denoised()))
        return res

    own = _tracer(srt, sc, w, h)
    want = sequence(own)
    own.close()
    pt = _tracer(srt, sc, w, h)
    sentinel = np.full((h, w, 4), 7.5, np.float32)
    pt.write_accumulator(sentinel)
    t = torch.full((h, w, 4), -3.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    pt.bind_output(d_accumulator=t.data_ptr())
    got = sequence(pt)
    pt.wait()
    for (a1, l1, d1), (a2, l2, d2) in zip(want, got):
        assert _same_bits(a1, a2) and _same_bits(l1, l2) and _same_bits(d1, d2)
    assert _same_bits(t.cpu().numpy(), want[-1][0]), "the bound tensor does not hold the blend"
    assert (want[-1][1] > 2).any(), "the second frame blended nothing"
    pt.bind_output()
    assert _same_bits(pt.accumulator(), sentinel), "the handle's own accumulator was written"
    pt.close()
