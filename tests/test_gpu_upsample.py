"""Guided upsampler (srt_upsample) on the MI355X: the joint-bilateral interpolation of block anchors of include/srt_pathtrace.h
against a float64 numpy restatement on synthetic guides, its exact properties (identity, anchors, pixels without a tap, linear
fields), object isolation, the in-place form, the framebuffer flag and non-interference, what it reconstructs of real block
renders, errors, torch binding, the host layer, the CLI and the viewer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
VIEWER = os.path.join(ROOT, "software-raytracer_amd", "srt_viewer")
GUIDES = ["object", "normal_depth", "position"]
# The denoiser's bound (tests/test_gpu_denoise.py REL_TOL): the same hardware exp2 / log2 weights with four taps instead of 25.
# The kernel's maximum over test_upsample_matches_the_definition, measured on the MI355X: 1.5e-5 at 67 x 45 and 1.2e-5 at
# 256 x 160 (a host transcription with libm's exp2f / log2f / expf in place of the hardware ones gives 1.5e-5 too); over the
# shapes and extremes of tests/test_gpu_pass_edges.py 2.3e-6.
REL_TOL = 1e-4
FLT_MAX = float(np.finfo(np.float32).max)


def host_stripe(w):
    """The stripe width PathTraceRenderer::RenderFrame passes: ceil(W / 16) + 1 with the integer divide first."""
    return w // 16 + 1


# ---- the definition ---------------------------------------------------------------------------------------------------
def anchors(n, steps, stripe):
    """The anchor coordinates of an axis of n pixels: k*S + j*steps inside stripe k and inside the axis (rows: stripe = 0)."""
    s = stripe if stripe > 0 else n
    out = []
    for k in range((n + s - 1) // s):
        j = 0
        while k * s + j * steps < min((k + 1) * s, n):
            out.append(k * s + j * steps)
            j += 1
    return np.array(sorted(set(out)), np.int64)


def around(n, steps, stripe):
    """Per coordinate v: a0 = the largest anchor <= v, a1 = the smallest anchor > v or -1, f = (v - a0) / (a1 - a0) in binary32."""
    a = anchors(n, steps, stripe)
    v = np.arange(n)
    i = np.searchsorted(a, v, side="right")
    a0 = a[i - 1]
    a1 = np.where(i < len(a), a[np.minimum(i, len(a) - 1)], -1)
    f = np.where(a1 < 0, np.float32(0), (v - a0).astype(np.float32) / np.maximum(a1 - a0, 1).astype(np.float32)).astype(np.float32)
    return a0, a1, f


def reference(acc, obj, nd, pos, steps, stripe, sigma_normal, sigma_plane):
    """The upsampler of include/srt_pathtrace.h in float64 (guides and colour as float32 arrays, scene rows).  Returns the
    result (H, W, 4), the anchor mask and the mask of pixels whose counted weights sum to something (the others keep c_p)."""
    H, W = obj.shape
    x0, x1, fx = around(W, steps, stripe)
    y0, y1, fy = around(H, steps, 0)
    hit = obj >= 0
    c = acc[..., :3].astype(np.float64)
    n = nd[..., :3].astype(np.float64)
    d = nd[..., 3].astype(np.float64)
    x = pos[..., :3].astype(np.float64)
    sw = np.zeros((H, W))
    sc = np.zeros((H, W, 3))
    for ky in (0, 1):
        qy = np.broadcast_to((y1 if ky else y0)[:, None], (H, W))
        by = (fy if ky else 1.0 - fy.astype(np.float64))[:, None]
        for kx in (0, 1):
            qx = np.broadcast_to((x1 if kx else x0)[None, :], (H, W))
            b = by * (fx if kx else 1.0 - fx.astype(np.float64))[None, :]
            cy, cx = np.maximum(qy, 0), np.maximum(qx, 0)
            take = (qy >= 0) & (qx >= 0) & (b != 0) & (obj[cy, cx] == obj)
            w = b.astype(np.float64)
            with np.errstate(all="ignore"):
                if sigma_normal > 0:
                    w = np.where(hit, w * np.maximum(0.0, np.sum(n * n[cy, cx], axis=2)) ** sigma_normal, w)
                if sigma_plane > 0:
                    # the header's clamping: a sigma above FLT_MAX counts as FLT_MAX, the reciprocal scale stops at +-FLT_MAX
                    # (d_p = 0 included) and an exact tie keeps its weight 1
                    scale = np.clip(1.0 / (min(float(sigma_plane), FLT_MAX) * d), -FLT_MAX, FLT_MAX)
                    dist = np.abs(np.sum(n * (x[cy, cx] - x), axis=2))
                    w = np.where(hit, w * np.where(dist == 0, 1.0, np.exp(-dist * scale)), w)
                w = np.where(take, w, 0.0)
                sw += w
                sc += np.where(take[..., None], w[..., None] * np.where(take[..., None], c[cy, cx], 0.0), 0.0)
    anchor = (np.arange(H) == y0)[:, None] & (np.arange(W) == x0)[None, :]
    solved = (sw != 0) & ~anchor
    out = acc.astype(np.float64).copy()
    with np.errstate(all="ignore"):
        out[..., :3] = np.where(solved[..., None], sc / sw[..., None], out[..., :3])
    return out, anchor, solved


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
def synthetic(w, h, seed, n_objects=5):
    """Objects as blobs of smoothly varying normals, points and depths with noisy positive colours; a block of misses, some
    scattered ones, and a few objects one pixel wide."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy = rng.uniform(0, w, n_objects), rng.uniform(0, h, n_objects)
    obj = np.argmin(np.stack([np.hypot(xs - cx[k], ys - cy[k]) for k in range(n_objects)]), axis=0).astype(np.int32)
    obj[rng.random((h, w)) < 0.04] = -1
    obj[(xs < w * 0.2) & (ys > h * 0.6)] = -1
    obj[:, w // 2 + 1] = n_objects       # one-pixel-wide objects: a column, a row
    obj[h // 3 + 1, :] = n_objects + 1
    k = np.maximum(obj, 0)
    base_n = rng.normal(size=(n_objects + 2, 3))
    base_n *= 2.0 / np.linalg.norm(base_n, axis=1, keepdims=True)  # (normals of one object stay within an acute angle)
    nrm = base_n[k] + 0.25 * np.stack([np.sin(xs / 7.0), np.cos(ys / 5.0), np.sin((xs + ys) / 11.0)], -1)
    nrm += 0.02 * rng.normal(size=nrm.shape)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    depth = 2.0 + 3.0 * rng.random(n_objects + 2)[k] + 0.01 * xs
    pnt = np.stack([xs * 0.01, ys * 0.01, depth], -1) + 0.002 * rng.normal(size=(h, w, 3))
    nd = np.concatenate([nrm, depth[..., None]], -1).astype(np.float32)
    pos = np.concatenate([pnt, np.ones((h, w, 1))], -1).astype(np.float32)
    acc = np.concatenate([rng.uniform(0.05, 4.0, (h, w, 3)), rng.choice(np.array([0.0, 1.0, 0.5], np.float32), size=(h, w, 1))],
                         -1).astype(np.float32)
    miss = obj < 0
    nd[miss] = np.array([0, 0, 0, np.inf], np.float32)
    pos[miss] = 0
    return acc, obj, nd, pos


def _bind(pt, obj, nd, pos):
    import torch

    t = {"object": torch.from_numpy(obj).to("cuda:0"), "normal_depth": torch.from_numpy(nd).to("cuda:0"),
         "position": torch.from_numpy(pos).to("cuda:0")}
    torch.cuda.synchronize()
    for k, v in t.items():
        pt.bind_gbuffer(k, v)
    return t


def _rel_err(got, ref, mask):
    g, r = got[mask][:, :3].astype(np.float64), ref[mask][:, :3]
    return float(np.max(np.abs(g - r) / np.maximum(np.abs(r), 1e-6))) if g.size else 0.0


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


SIGMAS = [(0.0, 0.0), (32.0, 0.0), (0.0, 0.02), (32.0, 0.02), (128.0, 0.05)]  # each term off and on
STEPS = [1, 2, 3, 8, 64]


# ---- the definition, and what it implies exactly ------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(67, 45), (256, 160)])
def test_upsample_matches_the_definition(srt, w, h):
    acc, obj, nd, pos = synthetic(w, h, seed=w)
    pt = srt.PathTracer(w, h)
    keep = _bind(pt, obj, nd, pos)
    pt.write_accumulator(acc)
    worst = 0.0
    for steps in STEPS:
        for stripe in (0, 17, host_stripe(w)):
            for sn, sx in SIGMAS:
                pt.upsample(steps=steps, stripe_width=stripe, sigma_normal=sn, sigma_plane=sx, gbuffer=False)
                got = pt.upsampled()
                ref, anchor, solved = reference(acc, obj, nd, pos, steps, stripe, sn, sx)
                err = _rel_err(got, ref, solved)
                worst = max(worst, err)
                case = (steps, stripe, sn, sx)
                assert err <= REL_TOL, (case, err)
                assert _same_bits(got[..., 3], acc[..., 3]), ("alpha is not the input's", case)
                assert _same_bits(got[anchor], acc[anchor]), ("an anchor pixel changed", case)
                assert _same_bits(got[~solved], acc[~solved]), ("a pixel without a counting tap changed", case)
                if steps == 1:
                    assert _same_bits(got, acc), ("steps = 1 is not the identity", case)
    print("max relative error %.3g" % worst)
    pt.close()
    del keep


def test_pixels_without_a_counting_tap_keep_their_bits(srt):
    w, h, steps = 64, 48, 4
    rng = np.random.default_rng(5)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    obj = np.zeros((h, w), np.int32)
    nd = np.broadcast_to(np.array([0, 0, -1, 3], np.float32), (h, w, 4)).copy()
    pos = np.stack([xs * 0.01, ys * 0.01, np.full_like(xs, 3), np.ones_like(xs)], -1).astype(np.float32)
    acc = rng.uniform(0.05, 4.0, (h, w, 4)).astype(np.float32)
    obj[:, 9] = 1    # a column and a row between the anchors (multiples of 4): no anchor of theirs exists
    obj[14, :] = 2
    obj[14, 9] = 3   # and a single pixel
    pt = srt.PathTracer(w, h)
    keep = _bind(pt, obj, nd, pos)
    pt.write_accumulator(acc)
    for sn, sx in SIGMAS:
        pt.upsample(steps=steps, sigma_normal=sn, sigma_plane=sx, gbuffer=False)
        got = pt.upsampled()
        thin = obj > 0
        assert _same_bits(got[thin], acc[thin])
        _, anchor, solved = reference(acc, obj, nd, pos, steps, 0, sn, sx)
        assert not solved[thin].any() and solved[~thin & ~anchor].all()
        assert not _same_bits(got[~thin & ~anchor], acc[~thin & ~anchor])
    pt.close()
    del keep


def test_linear_fields_are_reproduced(srt):
    w, h = 96, 72
    acc, obj, nd, pos = synthetic(w, h, seed=8, n_objects=4)
    rng = np.random.default_rng(2)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    coef = rng.uniform(0.01, 0.05, (obj.max() + 2, 3, 2))
    k = obj + 1  # (misses are a field of their own: the sky is interpolated too)
    lin = 1.0 + coef[k][..., 0] * xs[..., None] + coef[k][..., 1] * ys[..., None]
    acc[..., :3] = lin.astype(np.float32)
    want = acc[..., :3].astype(np.float64)  # (the float32 field: its rounding is within the bound)
    pt = srt.PathTracer(w, h)
    keep = _bind(pt, obj, nd, pos)
    # every non-anchor pixel poisoned: only the anchors' values may matter
    for steps, stripe in ((2, 0), (4, 0), (8, 0), (3, 17), (4, host_stripe(w))):
        x0, x1, _ = around(w, steps, stripe)
        y0, y1, _ = around(h, steps, 0)
        full = (x1 >= 0)[None, :] & (y1 >= 0)[:, None]
        cy0, cy1, cx0, cx1 = y0[:, None], np.maximum(y1, 0)[:, None], x0[None, :], np.maximum(x1, 0)[None, :]
        for qy in (cy0, cy1):
            for qx in (cx0, cx1):
                full = full & (obj[np.broadcast_to(qy, (h, w)), np.broadcast_to(qx, (h, w))] == obj)
        anchor = (np.arange(h) == y0)[:, None] & (np.arange(w) == x0)[None, :]
        poisoned = acc.copy()
        poisoned[~anchor, :3] = -7.0
        pt.write_accumulator(poisoned)
        pt.upsample(steps=steps, stripe_width=stripe, sigma_normal=0.0, sigma_plane=0.0, gbuffer=False)
        got = pt.upsampled()[..., :3].astype(np.float64)
        assert full.sum() > w * h // 8
        err = float(np.max(np.abs(got[full] - want[full]) / want[full]))
        print("steps %d stripe %d: %d pixels with four taps of their object, max relative error %.3g" % (steps, stripe, full.sum(), err))
        assert err <= REL_TOL, (steps, stripe, err)
    pt.close()
    del keep


def test_isolation(srt):
    """Non-finite colours and guides on every pixel of another object (its anchors included), and non-finite colours on every
    non-anchor pixel of the object itself, change no pixel of the object that has a counting tap: those read the object's own
    anchors and their own guides, nothing else.  (A pixel's own guides are inputs of its weights, and a pixel without a
    counting tap keeps its own colour, so those two cannot be poisoned without changing the definition's result.)"""
    w, h, steps, stripe = 96, 72, 4, 17
    acc, obj, nd, pos = synthetic(w, h, seed=3, n_objects=4)
    pt = srt.PathTracer(w, h)
    keep = _bind(pt, obj, nd, pos)
    params = dict(steps=steps, stripe_width=stripe, sigma_normal=32.0, sigma_plane=0.02, gbuffer=False)
    pt.write_accumulator(acc)
    pt.upsample(**params)
    base = pt.upsampled()
    _, anchor, solved = reference(acc, obj, nd, pos, steps, stripe, 32.0, 0.02)
    assert np.isfinite(base[..., :3]).all()
    rng = np.random.default_rng(9)
    junk = np.array([np.nan, np.inf, -np.inf, 1e30, -3.0], np.float32)
    for k in (-1, 0, 1, 2, 3):
        mine = obj == k
        bad_acc, bad_nd, bad_pos = acc.copy(), nd.copy(), pos.copy()
        bad_acc[..., :3] = np.where((~mine | ~anchor)[..., None], rng.choice(junk, size=(h, w, 3)), acc[..., :3])
        bad_nd[~mine] = rng.choice(junk, size=(h, w, 4))[~mine]
        bad_pos[~mine] = rng.choice(junk, size=(h, w, 4))[~mine]
        keep = _bind(pt, obj, bad_nd, bad_pos)
        pt.write_accumulator(bad_acc)
        pt.upsample(**params)
        got = pt.upsampled()
        check = mine & (solved | anchor)
        assert check.sum() > 50, k
        assert _same_bits(got[check], base[check]), k
        assert _same_bits(got[..., 3], acc[..., 3])
    pt.close()
    del keep


def test_in_place_framebuffer_and_non_interference(srt):
    w, h, steps, stripe = 67, 45, 3, 17
    acc, obj, nd, pos = synthetic(w, h, seed=11)
    acc[6, 7, :3] = [np.inf, 1e30, 0.0]  # a non-anchor pixel's own colour does not matter; (6, 6) is an anchor
    acc[6, 6, :3] = [50.0, 1e30, 0.0]
    pt = srt.PathTracer(w, h)
    keep = _bind(pt, obj, nd, pos)
    pt.write_accumulator(acc)
    before = pt.framebuffer()
    kw = dict(steps=steps, stripe_width=stripe, gbuffer=False)
    pt.upsample(**kw)
    out = pt.upsampled()
    assert np.array_equal(pt.framebuffer(), before), "the framebuffer was written without SRT_UPSAMPLE_FRAMEBUFFER"
    assert _same_bits(pt.accumulator(), acc), "the out-of-place form wrote the accumulator"
    pt.upsample(framebuffer=True, **kw)
    assert _same_bits(pt.upsampled(), out)
    fb = pt.framebuffer()
    assert np.array_equal(fb, tone_map(out)[::-1]) and not np.array_equal(fb, before)
    # in place: the same rgb on the non-anchors, anchors and alphas untouched, the upsampled buffer untouched, idempotent
    _, anchor, solved = reference(acc, obj, nd, pos, steps, stripe, 32.0, 0.02)
    marker = np.full((h, w, 4), -5.0, np.float32)
    import torch

    bound = torch.from_numpy(marker).to("cuda:0")
    torch.cuda.synchronize()
    pt.bind_upsampled(bound)
    pt.upsample(in_place=True, **kw)
    one = pt.accumulator()
    assert _same_bits(one[..., :3][~anchor], out[..., :3][~anchor])
    assert _same_bits(one[anchor], acc[anchor]) and _same_bits(one[..., 3], acc[..., 3])
    assert _same_bits(one[~solved], acc[~solved])
    pt.upsample(in_place=True, framebuffer=True, **kw)
    assert _same_bits(pt.accumulator(), one), "a second in-place call changed the accumulator"
    assert np.array_equal(pt.framebuffer(), tone_map(one)[::-1])
    assert _same_bits(bound.cpu().numpy(), marker), "the in-place form wrote the bound result buffer"
    pt.bind_upsampled(None)
    assert _same_bits(pt.upsampled(), out)  # the own buffer still holds the out-of-place result
    pt.close()
    del keep


def _scene_tracer(srt, oracle, name, w, h):
    oarr, n = oracle.make_objects(oracle.load_scene_json_py(scene_path(name)))
    pt = srt.PathTracer(w, h)
    pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
    pt.set_camera(srt.default_camera())
    return pt, oarr


def test_stats_gbuffer_history_and_later_renders_are_left_alone(srt, oracle):
    w, h = 320, 256
    fields = ("rays", "sample_chunks", "tile_rows", "chunk_samples", "shape_source", "path_samples")
    runs = []
    for with_upsample in (False, True):
        pt, oarr = _scene_tracer(srt, oracle, "Scene1", w, h)
        pt.render(spp=8, bounces=4, seed=5, steps=2, count_rays=True, count_work=True)
        first = pt.stats()
        pt.render_gbuffer()
        pt.temporal(samples=8, gbuffer=False, reset=True)
        if with_upsample:
            acc, g, hist = pt.accumulator(), {k: pt.gbuffer(k) for k in GUIDES + ["albedo"]}, pt.history_length()
            work = pt.work_counts().as_dict()
            pt.upsample(gbuffer=False)
            one = pt.upsampled()
            pt.upsample(gbuffer=False, framebuffer=True)
            pt.upsample(gbuffer=False)
            assert _same_bits(pt.upsampled(), one), "two calls differ"
            assert _same_bits(pt.accumulator(), acc)
            pt.upsample(gbuffer=False, in_place=True)
            for k in g:
                assert np.array_equal(pt.gbuffer(k).view(np.uint32), g[k].view(np.uint32)), k
            assert _same_bits(pt.history_length(), hist)
            after = pt.stats()
            assert all(getattr(after, f) == getattr(first, f) for f in fields) and after.kernel_ms == first.kernel_ms
            assert pt.work_counts().as_dict() == work
        pt.render(spp=8, bounces=4, seed=6, count_rays=True, count_work=True)  # (reset: the in-place form asks for it)
        st = pt.stats()
        runs.append(([getattr(st, f) for f in fields], pt.work_counts().as_dict(), pt.framebuffer(), pt.accumulator()))
        pt.close()
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1]
    assert np.array_equal(a[2], b[2]) and _same_bits(a[3], b[3])


# ---- it reconstructs ------------------------------------------------------------------------------------------------------
def _near_edges(obj, reach):
    """Pixels within `reach` (Chebyshev) of a pixel whose object index differs from a 4-neighbour's."""
    edge = np.zeros(obj.shape, bool)
    edge[:, 1:] |= obj[:, 1:] != obj[:, :-1]
    edge[:, :-1] |= obj[:, 1:] != obj[:, :-1]
    edge[1:, :] |= obj[1:, :] != obj[:-1, :]
    edge[:-1, :] |= obj[1:, :] != obj[:-1, :]
    h, w = obj.shape
    for axis, n in ((0, h), (1, w)):
        grown = edge.copy()
        for s in range(1, reach + 1):
            a = [slice(None)] * 2
            b = [slice(None)] * 2
            a[axis], b[axis] = slice(s, n), slice(0, n - s)
            grown[tuple(a)] |= edge[tuple(b)]
            grown[tuple(b)] |= edge[tuple(a)]
        edge = grown
    return edge


def _mse(a, b, mask):
    tm = lambda v: (v[..., :3] / (1.0 + v[..., :3]))[mask].astype(np.float64)  # noqa: E731
    return float(np.mean((tm(a) - tm(b)) ** 2))


# "Strictly below" is the condition.  No ratio has been measured yet (tools/upsample_time.py quality writes the lines meant for
# profiles/upsample/upsample_quality.jsonl); a ratio bound would be tightened only to what such lines clear with room.
@pytest.mark.parametrize("name", ["Scene1", "Scene_indirect"])
def test_it_reconstructs_the_preview(srt, oracle, name):
    w, h = 320, 180
    pt, oarr = _scene_tracer(srt, oracle, name, w, h)
    pt.render(spp=1, preview=True)  # no RNG in the preview shader: the exact ground truth
    truth = pt.accumulator()
    pt.render_gbuffer()
    obj = pt.gbuffer("object")
    everywhere = np.ones((h, w), bool)
    for steps in (2, 4, 8):
        pt.render(spp=1, preview=True, steps=steps)
        blocks = pt.accumulator()
        pt.upsample(steps=steps, gbuffer=False)
        up = pt.upsampled()
        for what, mask in (("all", everywhere), ("edges", _near_edges(obj, steps))):
            mb, mu = _mse(blocks, truth, mask), _mse(up, truth, mask)
            print("%s steps %d %s: mse blocks %.4g upsampled %.4g ratio %.3f (%d pixels)" % (name, steps, what, mb, mu, mu / mb, mask.sum()))
            assert mu < mb, (name, steps, what, mu, mb)
    pt.close()


@pytest.mark.parametrize("name", ["Scene1", "Scene_indirect"])
def test_it_reconstructs_path_traced_edges(srt, oracle, name):
    w, h, steps = 320, 180, 2
    pt, oarr = _scene_tracer(srt, oracle, name, w, h)
    pt.render(spp=64, bounces=4, seed=21)
    full = pt.accumulator()
    pt.render_gbuffer()
    edges = _near_edges(pt.gbuffer("object"), steps)
    pt.render(spp=64, bounces=4, seed=21, steps=steps)
    blocks = pt.accumulator()
    pt.upsample(steps=steps, gbuffer=False)
    up = pt.upsampled()
    mb, mu = _mse(blocks, full, edges), _mse(up, full, edges)
    print("%s 64 spp steps %d edges: mse blocks %.4g upsampled %.4g ratio %.3f" % (name, steps, mb, mu, mu / mb))
    assert mu < mb, (name, mu, mb)
    pt.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_errors(srt):
    import torch

    w, h = 40, 24
    pt = srt.PathTracer(w, h)
    with pytest.raises(srt.SrtError) as e:
        pt.upsample(gbuffer=False)
    assert e.value.code == srt.capi.ERR_STATE
    with pytest.raises(srt.SrtError) as e:
        pt.upsampled()
    assert e.value.code == srt.capi.ERR_STATE
    acc, obj, nd, pos = synthetic(w, h, seed=1)
    keep = _bind(pt, obj, nd, pos)
    for name in GUIDES:  # each guide is needed
        pt.bind_gbuffer(name, None)
        with pytest.raises(srt.SrtError) as e:
            pt.upsample(gbuffer=False)
        assert e.value.code == srt.capi.ERR_STATE, name
        pt.bind_gbuffer(name, keep[name])
    pt.write_accumulator(acc)
    pt.upsample(gbuffer=False, in_place=True)
    with pytest.raises(srt.SrtError) as e:  # the in-place form wrote no result buffer
        pt.upsampled()
    assert e.value.code == srt.capi.ERR_STATE
    bad = [dict(steps=0), dict(steps=-1), dict(steps=32769), dict(stripe_width=-1), dict(sigma_normal=-0.5), dict(sigma_plane=-1e-9),
           dict(sigma_normal=float("nan")), dict(sigma_plane=float("nan"))]
    for kw in bad:
        with pytest.raises(srt.SrtError) as e:
            pt.upsample(gbuffer=False, **kw)
        assert e.value.code == srt.capi.ERR_INVALID_ARG, kw
    p = srt.capi.upsample_params()
    p.flags = 4
    assert pt.L.srt_upsample(pt._h, C.byref(p)) == srt.capi.ERR_INVALID_ARG
    with pytest.raises(srt.SrtError):
        pt.upsampled()
    # the largest arguments are accepted
    pt.upsample(gbuffer=False, steps=32768, stripe_width=2**31 - 1, sigma_normal=float("inf"), sigma_plane=float("inf"))
    assert pt.upsampled().shape == (h, w, 4)
    for t in (torch.empty((h, w, 4), dtype=torch.float64, device="cuda:0"), torch.empty((h, w, 3), device="cuda:0"),
              torch.empty((h, w, 4)), torch.empty((h, 2 * w, 4), device="cuda:0")[:, ::2], np.zeros((h, w, 4), np.float32)):
        with pytest.raises((TypeError, ValueError)):
            pt.bind_upsampled(t)
    pt.close()
    del keep


# ---- integration ----------------------------------------------------------------------------------------------------------
def test_torch_bound_output_on_a_torch_stream(srt, oracle):
    import torch

    w, h = 200, 120
    pt, oarr = _scene_tracer(srt, oracle, "Scene_indirect", w, h)
    pt.render(spp=4, bounces=4, seed=3, steps=4)
    pt.upsample(steps=4)
    own = pt.upsampled()
    stream = torch.cuda.Stream(device=0)
    pt.set_stream(stream.cuda_stream)
    out = torch.full((h, w, 4), -5.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    pt.bind_upsampled(out)
    pt.render(spp=4, bounces=4, seed=3, steps=4)
    pt.upsample(steps=4)
    stream.synchronize()
    assert _same_bits(out.cpu().numpy(), own)
    assert _same_bits(pt.upsampled(), own)
    pt.bind_upsampled(None)
    pt.set_stream(0)
    assert _same_bits(pt.upsampled(), own)  # the own buffer still holds the first result
    pt.close()


def _host_scene_tracer(srt, name, w, h):
    scene = srt.host.Scene(scene_path(name))
    objs, n = scene.objects_copy()
    pt = srt.PathTracer(w, h)
    pt.set_scene(objs, n)
    pt.set_camera(srt.default_camera())
    return pt, objs


def test_host_renderer_equals_path_tracer(srt):
    w, h = 160, 90
    scene = srt.host.Scene(scene_path("Scene1"))
    r = srt.host.Renderer(w, h)
    r.set_scene(scene)
    r.render_frame()  # the start-up frame: preview shader, 2 x 2 blocks anchored at the 16 stripes
    r.upsample(steps=2, stripe_width=host_stripe(w))
    got = r.upsampled()
    acc = r.accumulator()
    g = {k: r.gbuffer(k) for k in GUIDES}
    r.close()
    pt = srt.PathTracer(w, h)
    keep = _bind(pt, g["object"], g["normal_depth"], g["position"])
    pt.write_accumulator(acc)
    pt.upsample(steps=2, stripe_width=host_stripe(w), gbuffer=False)
    assert _same_bits(pt.upsampled(), got)
    assert not _same_bits(got, acc)
    pt.close()
    del keep


def test_render_frame_with_and_without_guided_upsample(srt):
    """RenderFrame's calls, restated through PathTracer: the start-up frame (sample 1, no reset, steps 2), the frame after an
    edit (reset, steps 8) and the one after that (reset, steps 2), all with the preview shader and the host's stripe width.
    With guidedUpsample off the framebuffer is the render's; with it on it is the explicit render, guides, upsample sequence;
    the accumulator is the render's either way."""
    w, h = 160, 90
    sw = host_stripe(w)
    frames = [dict(reset=False, steps=2), dict(reset=True, steps=8), dict(reset=True, steps=2)]
    pt, objs = _host_scene_tracer(srt, "Scene1", w, h)
    want = []
    for f in frames:
        pt.render(spp=1, bounces=2, seed=0, first_sample=1, preview=True, stripe_width=sw, selected=-1, **f)
        plain, acc = pt.framebuffer(), pt.accumulator()
        pt.upsample(steps=f["steps"], stripe_width=sw, framebuffer=True)
        want.append((plain, pt.framebuffer(), acc))
        assert not np.array_equal(want[-1][0], want[-1][1])
    pt.close()
    for guided in (False, True):
        scene = srt.host.Scene(scene_path("Scene1"))
        r = srt.host.Renderer(w, h)
        r.set_scene(scene)
        r.guided_upsample(guided)
        for k, (plain, up, acc) in enumerate(want):
            if k == 1:
                r.invalidate()
            assert r.render_frame()
            assert np.array_equal(r.framebuffer(), up if guided else plain), (guided, k)
            assert _same_bits(r.accumulator(), acc), (guided, k)
        if guided:  # whole frame only
            r.set_band(0, h // 2)
            with pytest.raises(RuntimeError, match="error|band"):
                r.render_frame()
        r.close()


def _ppm_rgb(path, w, h):
    data = open(path, "rb").read()
    head = b"P6\n%d %d\n255\n" % (w, h)
    assert data.startswith(head)
    return np.frombuffer(data[len(head):], np.uint8).reshape(h, w, 3)


def _rgb(fb):
    return np.stack([(fb >> 16) & 255, (fb >> 8) & 255, fb & 255], -1).astype(np.uint8)


def test_cli_writes_the_upsampled_ppm(srt, tmp_path):
    w, h = 160, 90
    base = [CLI, "--scene", scene_path("Scene1"), "--width", str(w), "--height", str(h), "--spp", "4", "--bounces", "2", "--steps", "4"]
    r1 = subprocess.run(base + ["--out", str(tmp_path / "a.ppm"), "--upsample", str(tmp_path / "u.ppm")], capture_output=True, text=True,
                        timeout=300)
    assert r1.returncode == 0, r1.stderr[-2000:]
    r2 = subprocess.run(base + ["--out", str(tmp_path / "b.ppm"), "--upsample", str(tmp_path / "v.ppm"), "--denoise", str(tmp_path / "d.ppm")],
                        capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr[-2000:]
    pt, objs = _host_scene_tracer(srt, "Scene1", w, h)
    pt.render(spp=4, bounces=2, seed=0, steps=4, count_rays=True)
    blocks = _rgb(pt.framebuffer())
    pt.upsample(steps=4, framebuffer=True)
    up = _rgb(pt.framebuffer())
    assert np.array_equal(_ppm_rgb(tmp_path / "a.ppm", w, h), blocks) and np.array_equal(_ppm_rgb(tmp_path / "b.ppm", w, h), blocks)
    assert np.array_equal(_ppm_rgb(tmp_path / "u.ppm", w, h), up)
    assert not np.array_equal(up, blocks)
    # with --denoise: the in-place form (the same pixels), then the denoiser on the accumulator it left
    pt.upsample(steps=4, in_place=True, framebuffer=True)
    assert np.array_equal(_ppm_rgb(tmp_path / "v.ppm", w, h), _rgb(pt.framebuffer()))
    assert np.array_equal(_ppm_rgb(tmp_path / "v.ppm", w, h), up)
    pt.denoise(framebuffer=True)
    assert np.array_equal(_ppm_rgb(tmp_path / "d.ppm", w, h), _rgb(pt.framebuffer()))
    pt.close()
    r3 = subprocess.run(base + ["--devices", "0,0", "--out", str(tmp_path / "c.ppm"), "--upsample", str(tmp_path / "e.ppm")],
                        capture_output=True, text=True, timeout=300)
    assert r3.returncode != 0 and "one device" in r3.stderr and not (tmp_path / "e.ppm").exists()


def test_scripted_viewer_toggle(srt, tmp_path):
    if not os.path.exists(VIEWER):
        pytest.fail("srt_viewer not built (make -C software-raytracer_amd/host)")
    w, h = 320, 180
    outs = [str(tmp_path / ("%s.ppm" % n)) for n in "abc"]
    script = tmp_path / "session.txt"
    script.write_text("frames 1\nsave %s\npress R\nframes 2\nsave %s\nupsample off\nframes 1\nsave %s\n" % tuple(outs))
    r = subprocess.run([VIEWER, "--scene", scene_path("Scene_indirect"), "--width", str(w), "--height", str(h), "--script", str(script)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [_ppm_rgb(p, w, h) for p in outs]
    sc = srt.host.Scene(scene_path("Scene_indirect"))
    rr = srt.host.Renderer(w, h)
    rr.set_scene(sc)
    rr.render_frame()
    want = [_rgb(rr.framebuffer())]
    rr.guided_upsample(True)
    rr.render_frame()
    rr.render_frame()
    want.append(_rgb(rr.framebuffer()))
    rr.guided_upsample(False)
    rr.render_frame()
    want.append(_rgb(rr.framebuffer()))
    rr.close()
    for k in range(3):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got[0], got[2]) and not np.array_equal(got[0], got[1])  # preview frames of 2 x 2 blocks, reconstructed in between
