"""Variance estimate and variance-guided denoiser (srt_variance, srt_denoise_variance) on the MI355X: the estimate's exact
identities and its float64 definition, the filter against tests/variance_reference.py on real first-hit buffers, its bit-for-bit
link to srt_denoise, isolation, repeatability and the limits of the variance, state and errors, torch binding, srt_antialias on
its result, non-interference, the host layer, the CLI, the viewer and the noise it removes from a real frame."""
import ctypes as C
import importlib.util
import json
import os
import subprocess

import numpy as np
import pytest

import variance_reference as vr
from conftest import ROOT, scene_path
# REL_TOL: the bound srt_denoise is held to against its reference, at every level count (one hardware exp per term: the same
# arithmetic class).  The filter's maximum, measured on the MI355X (profiles/denoise/variance_error.jsonl, the lines
# test_filter_matches_the_definition and test_real_frame_links_to_srt_denoise_and_repeats print): 1.3e-6 on the first-hit buffers
# at 1, 3 and 5 levels, 2.1e-6 on the rendered frame; over the shapes, seams and extremes of tests/test_gpu_pass_edges.py
# 5.1e-6.  The estimate's maximum is 7.7e-8 of S^2 (8.0e-8 over those shapes) against the derived bound of 9.5e-7.
from test_gpu_denoise import REL_TOL, synthetic, tone_map

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
VIEWER = os.path.join(ROOT, "software-raytracer_amd", "srt_viewer")
NAMES = ["object", "normal_depth", "position", "albedo"]
U = 2.0 ** -24  # half an ulp of binary32, relative: the most one rounding adds
# The estimate against the float64 definition.  Derived, not measured: lA and lB are each at most 4 roundings deep (the
# division by m_p, the product with the weight, two additions; the halvings are exact), the subtraction and the square add
# two more: 8 roundings on the longest chain, no transcendental.  With positive inputs every intermediate is at most
# S = 0.5 lA + 0.5 lB, so d is off by at most 8 U S, and v = d*d, whose slope is 2 |d| <= 2 S, by at most 16 U S^2 (the
# second-order term is below U^2 S^2).  v itself can cancel to 0, so the bound is absolute in S^2, not relative to v.
EST_ROUNDINGS = 8


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _rel_err(got, ref, hit):
    g, r = got[hit][:, :3].astype(np.float64), ref[hit][:, :3]
    return float(np.max(np.abs(g - r) / np.maximum(np.abs(r), 1e-6)))


def _code(srt, call):
    with pytest.raises(srt.SrtError) as e:
        call()
    return e.value.code


def _cuda(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _bind(pt, obj, nd, pos, alb):
    t = {"object": _cuda(obj), "normal_depth": _cuda(nd), "position": _cuda(pos), "albedo": _cuda(alb)}
    for k, v in t.items():
        pt.bind_gbuffer(k, v)
    return t


def _halves(w, h, seed, alb):
    """Two positive half renders around one mean, with differing alphas."""
    rng = np.random.default_rng(seed)
    mean = alb[..., :3] * rng.uniform(0.2, 4.0, (h, w, 3)) + rng.uniform(0.01, 0.2, (h, w, 3))
    a = np.concatenate([mean * rng.uniform(0.5, 1.5, (h, w, 3)), rng.choice([0.0, 1.0, 7.5], size=(h, w, 1))], -1).astype(np.float32)
    b = np.concatenate([mean * rng.uniform(0.5, 1.5, (h, w, 3)), rng.choice([0.0, 2.0], size=(h, w, 1))], -1).astype(np.float32)
    return a, b


# ---- the estimate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(37, 21), (64, 48)])
def test_estimate_identities_and_definition(srt, w, h):
    _, obj, nd, pos, alb = synthetic(w, h, seed=w + 1)
    hit = obj >= 0
    assert hit.any() and (~hit).any()
    a, b = _halves(w, h, 5, alb)
    pt = srt.PathTracer(w, h)
    assert _code(srt, lambda: pt.variance(gbuffer=False)) == srt.capi.ERR_STATE  # no guide
    keep = _bind(pt, obj, nd, pos, alb)
    assert _code(srt, lambda: pt.variance(gbuffer=False)) == srt.capi.ERR_STATE  # no half buffer bound or fetched
    assert _code(srt, pt.variance_map) == srt.capi.ERR_STATE
    worst = 0.0

    def run(a_, b_, albedo, merge):
        tb = _cuda(b_)
        pt.bind_half(tb)
        pt.write_accumulator(a_)
        pt.variance(albedo=albedo, merge=merge, gbuffer=False)
        v, acc = pt.variance_map(), pt.accumulator()
        assert _same_bits(tb.cpu().numpy(), b_), "half B was written"
        return v, acc

    for albedo in (False, True):
        # equal halves: +0 everywhere, the merged accumulator is A
        v, acc = run(a, a.copy(), albedo, True)
        assert not _bits(v).any() and _same_bits(acc, a)
        # no MERGE: the accumulator is untouched
        v0, acc = run(a, b, albedo, False)
        assert _same_bits(acc, a)
        # MERGE: the plain mean on every pixel, misses included; alpha never written; the variance is the same
        v1, acc = run(a, b, albedo, True)
        mean32 = np.float32(0.5) * a[..., :3] + np.float32(0.5) * b[..., :3]
        assert _same_bits(acc[..., :3], mean32) and _same_bits(acc[..., 3], a[..., 3]) and _same_bits(v0, v1)
        # swap: the same variance bits and the same merged bits (the alpha is the accumulator's own)
        v2, acc2 = run(b, a, albedo, True)
        assert _same_bits(v2, v1) and _same_bits(acc2[..., :3], acc[..., :3]) and _same_bits(acc2[..., 3], b[..., 3])
        # misses are +0, hits are not all 0
        assert not _bits(v1[~hit]).any() and (v1[hit] > 0).any()
        # the float64 definition
        ref, mean = vr.variance(a, b, obj, alb, albedo)
        m = vr.demod(alb, albedo)
        s = 0.5 * vr.lum(a[..., :3].astype(np.float64) / m) + 0.5 * vr.lum(b[..., :3].astype(np.float64) / m)
        err = np.abs(v1.astype(np.float64) - ref) / (s * s)
        worst = max(worst, float(err[hit].max()))
        assert err[hit].max() <= 2 * EST_ROUNDINGS * U, (albedo, err[hit].max())
        assert np.max(np.abs(acc[..., :3] - mean) / mean) <= U
    print("estimate: max |v - v_ref| / S^2 = %.3g (bound %.3g)" % (worst, 2 * EST_ROUNDINGS * U))
    pt.bind_half(None)
    pt.close()
    del keep


# ---- real first-hit buffers -----------------------------------------------------------------------------------------------------
_GUIDES = {}


def _mesh_scene(oracle):
    """Scene1 with its big ball tessellated, as tests/test_gpu_antialias.py builds its small mesh scene."""
    objs = oracle.load_scene_json_py(scene_path("Scene1"))
    big = objs[64]
    objs[64] = dict(type=oracle.OBJ_MESH, position=big["position"], mesh=0, base=big["base"], emissive=big["emissive"],
                    smoothness=big["smoothness"], specular_amount=big["specular_amount"], specular=big["specular"])
    return objs, [oracle.uv_sphere(1.0, 8, 12)]


def _scene_tracer(srt, oracle, case, w, h):
    keep = []
    pt = srt.PathTracer(w, h)
    if case == "mesh":
        objs, meshes = _mesh_scene(oracle)
        marr, mn, mkeep = oracle.make_meshes(meshes)
        keep += [marr, mkeep]
        pt.set_meshes(C.cast(marr, C.POINTER(srt.Mesh)), mn)
    else:
        objs = oracle.load_scene_json_py(scene_path(case))
    oarr, n = oracle.make_objects(objs)
    keep.append(oarr)
    pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
    pt.set_camera(srt.default_camera())
    return pt, keep


SHAPES = {"Scene1": (37, 21), "mesh": (64, 48)}


def _guides(srt, oracle, case):
    """The four first-hit buffers of a scene at its test shape with synthetic colour and variance on top; made once, shared,
    read-only."""
    if case not in _GUIDES:
        w, h = SHAPES[case]
        pt, keep = _scene_tracer(srt, oracle, case, w, h)
        pt.render_gbuffer()
        g = [pt.gbuffer(k) for k in NAMES]
        pt.close()
        obj, alb = g[0], g[3]
        assert (obj >= 0).any() and (obj < 0).any() and len(np.unique(obj)) > 3
        rng = np.random.default_rng(len(case))
        acc = np.concatenate([alb[..., :3] * rng.uniform(0.2, 4.0, (h, w, 3)) + rng.uniform(0.01, 0.2, (h, w, 3)),
                              rng.choice(np.array([0.0, 1.0], np.float32), size=(h, w, 1))], -1).astype(np.float32)
        var = rng.uniform(0.02, 0.5, (h, w)).astype(np.float32)
        arrs = (acc, var) + tuple(g)
        for a in arrs:
            a.setflags(write=False)
        _GUIDES[case] = arrs
    return _GUIDES[case]


def _bound_tracer(srt, oracle, case):
    acc, var, obj, nd, pos, alb = _guides(srt, oracle, case)
    w, h = SHAPES[case]
    pt = srt.PathTracer(w, h)
    keep = _bind(pt, obj, nd, pos, alb)
    keep["variance"] = _cuda(var)
    pt.bind_variance(keep["variance"])
    pt.write_accumulator(acc)
    return pt, keep


@pytest.mark.parametrize("case", ["Scene1", "mesh"])
def test_filter_matches_the_definition(srt, oracle, case):
    acc, var, obj, nd, pos, alb = _guides(srt, oracle, case)
    hit = obj >= 0
    pt, keep = _bound_tracer(srt, oracle, case)
    worst = {}
    for levels in (1, 3, 5):
        for albedo in (False, True):
            for sl in (0.0, 4.0, float("inf")):
                pt.denoise_variance(iterations=levels, sigma_luminance=sl, sigma_normal=32.0, sigma_plane=0.02, albedo=albedo, gbuffer=False)
                got = pt.denoised()
                ref = vr.denoise_variance(acc, var, obj, nd, pos, alb, levels, sl, 32.0, 0.02, albedo)
                err = _rel_err(got, ref, hit)
                worst[levels] = max(worst.get(levels, 0.0), err)
                assert _same_bits(got[..., 3], acc[..., 3]), "alpha is not the input's"
                assert _same_bits(got[~hit], acc[~hit]), "miss pixels are not the input"
                assert _same_bits(keep["variance"].cpu().numpy(), var), "the variance buffer was written"
    for levels, err in sorted(worst.items()):
        print("variance_error " + json.dumps({"test": "test_filter_matches_the_definition", "case": case, "width": SHAPES[case][0],
                                              "height": SHAPES[case][1], "iterations": levels, "max_rel_err": err, "bound": REL_TOL}))
    assert max(worst.values()) <= REL_TOL, worst
    pt.close()
    del keep


@pytest.mark.parametrize("albedo", [False, True])
@pytest.mark.parametrize("case", ["Scene1", "mesh"])
def test_sigma_luminance_zero_is_srt_denoise_bit_for_bit(srt, oracle, case, albedo):
    acc, var, obj, nd, pos, alb = _guides(srt, oracle, case)
    pt, keep = _bound_tracer(srt, oracle, case)
    for levels in (1, 2, 4, 5):
        for sn, sx in ((32.0, 0.02), (0.0, 0.05), (128.0, 0.0), (0.0, 0.0)):
            pt.denoise(iterations=levels, sigma_color=0.0, sigma_normal=sn, sigma_plane=sx, albedo=albedo, gbuffer=False)
            want = pt.denoised()
            pt.denoise_variance(iterations=levels, sigma_luminance=0.0, sigma_normal=sn, sigma_plane=sx, albedo=albedo, gbuffer=False)
            assert _same_bits(pt.denoised(), want), (levels, sn, sx)
    assert not _same_bits(want, acc)
    pt.close()
    del keep


def test_real_frame_links_to_srt_denoise_and_repeats(srt, oracle):
    """One real frame of Scene1 at 96 x 64: two rendered halves, their variance and mean, the filter at its defaults."""
    w, h = 96, 64
    pt, keep = _scene_tracer(srt, oracle, "Scene1", w, h)
    pt.render(spp=4, bounces=4, seed=3)
    pt.bind_output(None, pt.half_ptr())
    pt.render(spp=4, bounces=4, seed=3 ^ 0x9E3779B9)
    pt.bind_output()
    a = pt.accumulator()
    pt.render_gbuffer()
    pt.variance(gbuffer=False)
    merged, var, obj = pt.accumulator(), pt.variance_map(), pt.gbuffer("object")
    hit = obj >= 0
    assert not _same_bits(merged, a) and (var[hit] > 0).any() and not var[~hit].any()
    pt.denoise_variance(gbuffer=False)
    one = pt.denoised()
    pt.denoise_variance(gbuffer=False)
    assert _same_bits(pt.denoised(), one), "a repeated call differs"
    assert _same_bits(pt.variance_map(), var) and _same_bits(pt.accumulator(), merged)
    assert _same_bits(one[~hit], merged[~hit]) and _same_bits(one[..., 3], merged[..., 3])
    assert not _same_bits(one, merged)
    for albedo in (True, False):
        if not albedo:
            assert _code(srt, lambda: pt.denoise_variance(sigma_luminance=0.0, albedo=False, gbuffer=False)) == srt.capi.ERR_STATE
            pt.write_accumulator(a)
            pt.variance(albedo=False, gbuffer=False)
        pt.denoise(sigma_color=0.0, albedo=albedo, gbuffer=False)
        want = pt.denoised()
        pt.denoise_variance(sigma_luminance=0.0, albedo=albedo, gbuffer=False)
        assert _same_bits(pt.denoised(), want), albedo
    # against the definition too
    g = [pt.gbuffer(k) for k in NAMES]
    acc, var = pt.accumulator(), pt.variance_map()
    pt.denoise_variance(albedo=False, gbuffer=False)
    d = srt.capi.DENOISE_VARIANCE_DEFAULTS
    ref = vr.denoise_variance(acc, var, *g, d["iterations"], d["sigma_luminance"], d["sigma_normal"], d["sigma_plane"], False)
    err = _rel_err(pt.denoised(), ref, hit)
    print("variance_error " + json.dumps({"test": "test_real_frame_links_to_srt_denoise_and_repeats", "case": "Scene1 rendered", "width": w,
                                          "height": h, "iterations": d["iterations"], "max_rel_err": err, "bound": REL_TOL}))
    assert err <= REL_TOL
    pt.close()


def test_isolation(srt, oracle):
    """NaN or inf colour and variance on one object change no bit on any pixel of another object."""
    acc, var, obj, nd, pos, alb = _guides(srt, oracle, "mesh")
    pt, keep = _bound_tracer(srt, oracle, "mesh")
    params = dict(iterations=5, sigma_luminance=4.0, gbuffer=False)
    pt.denoise_variance(**params)
    base = pt.denoised()
    ids, counts = np.unique(obj[obj >= 0], return_counts=True)
    rng = np.random.default_rng(4)
    for k in ids[np.argsort(-counts)][:3]:
        bad_c, bad_v = acc.copy(), var.copy()
        on = obj == k
        bad_c[on] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -3.0], np.float32), size=bad_c.shape)[on]
        bad_v[on] = rng.choice(np.array([np.nan, np.inf, -1.0, 1e38], np.float32), size=bad_v.shape)[on]
        pt.write_accumulator(bad_c)
        tv = _cuda(bad_v)
        pt.bind_variance(tv)
        pt.denoise_variance(**params)
        got = pt.denoised()
        other = ~on
        assert _same_bits(got[other], base[other]), int(k)
        assert _same_bits(tv.cpu().numpy(), bad_v)
    pt.close()
    del keep


def test_zero_and_huge_variance_and_iteration_limits(srt, oracle):
    acc, var, obj, nd, pos, alb = _guides(srt, oracle, "Scene1")
    hit = obj >= 0
    pt, keep = _bound_tracer(srt, oracle, "Scene1")
    # zero variance: the edge-stop closes on the distinct luminances of neighbouring pixels, the output is the input
    lum = vr.lum(acc[..., :3].astype(np.float64))
    assert np.min(np.abs(np.diff(lum, axis=1))) > 1e-6 and np.min(np.abs(np.diff(lum, axis=0))) > 1e-6
    zero = _cuda(np.zeros_like(var))
    pt.bind_variance(zero)
    for sl in (4.0, float("inf")):
        for albedo in (False, True):
            pt.denoise_variance(iterations=5, sigma_luminance=sl, albedo=albedo, gbuffer=False)
            assert _rel_err(pt.denoised(), acc.astype(np.float64), hit) <= REL_TOL, (sl, albedo)
    # a huge variance opens it: the result of sigma_luminance = 0
    huge = _cuda(np.full_like(var, 1e30))
    pt.bind_variance(huge)
    for albedo in (False, True):
        pt.denoise_variance(iterations=5, sigma_luminance=0.0, albedo=albedo, gbuffer=False)
        off = pt.denoised()
        pt.denoise_variance(iterations=5, sigma_luminance=4.0, albedo=albedo, gbuffer=False)
        got = pt.denoised()
        assert np.isfinite(got[hit][:, :3]).all()
        assert _rel_err(got, off.astype(np.float64), hit) <= REL_TOL, albedo
    # iterations: 8 is accepted, 0 and 9 are refused
    pt.denoise_variance(iterations=8, gbuffer=False)
    assert pt.denoised().shape == acc.shape
    for it in (0, 9, -1):
        assert _code(srt, lambda: pt.denoise_variance(iterations=it, gbuffer=False)) == srt.capi.ERR_INVALID_ARG
    pt.close()
    del keep, zero, huge


# ---- state, errors and layers -----------------------------------------------------------------------------------------------------
def test_errors_and_state(srt):
    import torch

    w, h = 40, 24
    STATE, ARG = srt.capi.ERR_STATE, srt.capi.ERR_INVALID_ARG
    acc, obj, nd, pos, alb = synthetic(w, h, seed=1)
    pt = srt.PathTracer(w, h)
    pt.write_accumulator(acc)
    assert _code(srt, lambda: pt.denoise_variance(gbuffer=False)) == STATE  # no guide
    keep = _bind(pt, obj, nd, pos, alb)
    assert _code(srt, lambda: pt.denoise_variance(gbuffer=False)) == STATE  # no variance bound or written
    assert _code(srt, lambda: pt.variance(gbuffer=False)) == STATE          # no half bound or fetched
    assert _code(srt, pt.variance_map) == STATE
    for flags in (4, 8, 7):
        assert pt.L.srt_variance(pt._h, C.byref(srt.capi.VarianceParams(flags))) == ARG
    half = pt.half_ptr()
    assert half and pt.half_ptr() == half
    pt.bind_gbuffer("albedo", None)  # never rendered: needed with ALBEDO only
    assert _code(srt, lambda: pt.variance(albedo=True, gbuffer=False)) == STATE
    assert _code(srt, lambda: pt.denoise_variance(gbuffer=False)) == STATE  # (still no variance)
    pt.variance(albedo=False, merge=False, gbuffer=False)
    assert pt.variance_map().shape == (h, w)
    assert _code(srt, lambda: pt.denoise_variance(albedo=True, gbuffer=False)) == STATE  # ALBEDO guide missing
    pt.denoise_variance(albedo=False, gbuffer=False)
    pt.bind_gbuffer("albedo", keep["albedo"])
    # the own variance buffer was estimated without ALBEDO: a call with it is refused, and the other way round
    assert _code(srt, lambda: pt.denoise_variance(albedo=True, gbuffer=False)) == STATE
    pt.variance(albedo=True, merge=False, gbuffer=False)
    pt.denoise_variance(albedo=True, gbuffer=False)
    assert _code(srt, lambda: pt.denoise_variance(albedo=False, gbuffer=False)) == STATE
    # a bound buffer is the caller's responsibility: no such check
    tv = torch.full((h, w), 0.1, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    pt.bind_variance(tv)
    pt.denoise_variance(albedo=False, gbuffer=False)
    pt.denoise_variance(albedo=True, gbuffer=False)
    pt.bind_variance(None)
    assert _code(srt, lambda: pt.denoise_variance(albedo=False, gbuffer=False)) == STATE  # the own one is the ALBEDO estimate still
    bad = [dict(iterations=0), dict(iterations=9), dict(sigma_luminance=-1.0), dict(sigma_normal=-0.5), dict(sigma_plane=-1e-9),
           dict(sigma_luminance=float("nan")), dict(sigma_normal=float("nan")), dict(sigma_plane=float("nan"))]
    for kw in bad:
        assert _code(srt, lambda: pt.denoise_variance(gbuffer=False, **kw)) == ARG, kw
    p = srt.capi.denoise_variance_params()
    p.flags = 4
    assert pt.L.srt_denoise_variance(pt._h, C.byref(p)) == ARG
    # tensors of the wrong kind are refused before any native call
    for t in (torch.empty((h, w), dtype=torch.float64, device="cuda:0"), torch.empty((h, w, 1), device="cuda:0"), torch.empty((h, w)),
              torch.empty((h, 2 * w), device="cuda:0")[:, ::2], np.zeros((h, w), np.float32)):
        with pytest.raises((TypeError, ValueError)):
            pt.bind_variance(t)
    for t in (torch.empty((h, w, 4), dtype=torch.float64, device="cuda:0"), torch.empty((h, w, 3), device="cuda:0"), torch.empty((h, w, 4))):
        with pytest.raises((TypeError, ValueError)):
            pt.bind_half(t)
    pt.close()
    del keep, tv


def test_torch_bound_half_variance_and_denoised(srt, oracle):
    import torch

    w, h = 61, 35
    pt, keep = _scene_tracer(srt, oracle, "Scene1", w, h)

    def frame(half_ptr):
        pt.render(spp=2, bounces=4, seed=3)
        pt.bind_output(None, half_ptr)
        pt.render(spp=2, bounces=4, seed=4)
        pt.bind_output()
        pt.variance()
        pt.denoise_variance()

    frame(pt.half_ptr())
    own_v, own_d, own_acc = pt.variance_map(), pt.denoised(), pt.accumulator()
    stream = torch.cuda.Stream(device=0)
    pt.set_stream(stream.cuda_stream)
    half = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    var = torch.full((h, w), -5.0, dtype=torch.float32, device="cuda:0")
    out = torch.full((h, w, 4), -5.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    pt.bind_half(half)
    pt.bind_variance(var)
    pt.bind_denoised(out)
    frame(half.data_ptr())
    stream.synchronize()
    assert _same_bits(var.cpu().numpy(), own_v) and _same_bits(out.cpu().numpy(), own_d)
    assert _same_bits(pt.variance_map(), own_v) and _same_bits(pt.denoised(), own_d) and _same_bits(pt.accumulator(), own_acc)
    assert (half.cpu().numpy()[..., :3] > 0).any()
    pt.bind_half(None)
    pt.bind_variance(None)
    pt.bind_denoised(None)
    pt.set_stream(0)
    assert _same_bits(pt.variance_map(), own_v) and _same_bits(pt.denoised(), own_d)  # the own buffers still hold the first results
    pt.close()


def test_antialias_takes_the_result_as_its_denoised_source(srt, oracle):
    from antialias_reference import resolve

    w, h, k = 64, 40, 2
    pt, keep = _scene_tracer(srt, oracle, "Scene1", w, h)
    pt.render_gbuffer()
    pt.render_subsamples(k)
    assert _code(srt, lambda: pt.antialias(k, denoised=True, guides=False)) == srt.capi.ERR_STATE
    pt.render(spp=2, bounces=4, seed=1)
    pt.bind_output(None, pt.half_ptr())
    pt.render(spp=2, bounces=4, seed=2)
    pt.bind_output()
    pt.variance(gbuffer=False)
    pt.denoise_variance(gbuffer=False)
    dv = pt.denoised()
    pt.antialias(k, denoised=True, guides=False)
    got = pt.antialiased()
    ref, foreign, changed = resolve(dv, pt.gbuffer("object"), pt.subsamples())
    assert changed.any() and _rel_err(got, ref, changed) <= 1e-5  # tests/test_gpu_antialias.py's derived bound
    assert _same_bits(got[~changed], dv[~changed]) and _same_bits(pt.denoised(), dv)
    pt.close()


def test_non_interference(srt, oracle):
    w, h = 64, 40
    fields = ("rays", "sample_chunks", "tile_rows", "chunk_samples", "shape_source", "path_samples")
    runs = []
    for with_passes in (False, True):
        pt, keep = _scene_tracer(srt, oracle, "Scene1", w, h)
        half = pt.half_ptr()
        pt.bind_output(None, half)
        pt.render(spp=4, bounces=4, seed=6)
        pt.bind_output()
        pt.render(spp=4, bounces=4, seed=5, count_rays=True, count_work=True)
        pt.render_gbuffer()
        pt.temporal(samples=4, gbuffer=False)
        pt.denoise(gbuffer=False)
        if with_passes:
            first, wc = pt.stats(), pt.work_counts().as_dict()
            acc, g, hist, dn, fb = pt.accumulator(), {k: pt.gbuffer(k) for k in NAMES}, pt.history_length(), pt.denoised(), pt.framebuffer()
            pt.variance(albedo=True, merge=False, gbuffer=False)
            assert _same_bits(pt.denoised(), dn) and _same_bits(pt.accumulator(), acc)
            pt.denoise_variance(gbuffer=False)
            assert np.array_equal(pt.framebuffer(), fb), "the framebuffer was written without SRT_DENOISE_FRAMEBUFFER"
            dv = pt.denoised()
            pt.denoise_variance(gbuffer=False, framebuffer=True)
            assert _same_bits(pt.denoised(), dv) and np.array_equal(pt.framebuffer(), tone_map(dv)[::-1])
            assert _same_bits(pt.accumulator(), acc) and _same_bits(pt.history_length(), hist)
            for k in NAMES:
                assert np.array_equal(_bits(pt.gbuffer(k)) if k != "object" else pt.gbuffer(k), _bits(g[k]) if k != "object" else g[k]), k
            after = pt.stats()
            assert bytes(after) == bytes(first) and pt.work_counts().as_dict() == wc
        pt.render(spp=4, first_sample=5, reset=False, bounces=4, seed=5, count_rays=True, count_work=True)
        st = pt.stats()
        pt.render_gbuffer()
        pt.temporal(samples=8, gbuffer=False)  # the history of the first call is read here
        runs.append(([getattr(st, f) for f in fields], pt.work_counts().as_dict(), pt.framebuffer(), pt.accumulator(), pt.history_length()))
        pt.close()
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1]
    assert np.array_equal(a[2], b[2]) and _same_bits(a[3], b[3]) and _same_bits(a[4], b[4])


def _rgb(fb):
    return np.stack([(fb >> 16) & 255, (fb >> 8) & 255, fb & 255], -1).astype(np.uint8)


def _ppm_rgb(path, w, h):
    data = open(path, "rb").read()
    head = b"P6\n%d %d\n255\n" % (w, h)
    assert data.startswith(head)
    return np.frombuffer(data[len(head):], np.uint8).reshape(h, w, 3)


def _library_frame(srt, w, h, spp, bounces, seed):
    """What PathTraceRenderer::denoiseVariance is documented to do, through the C calls."""
    objs, n = srt.host.Scene(scene_path("Scene1")).objects_copy()
    pt = srt.PathTracer(w, h)
    pt.set_scene(objs, n)
    pt.set_camera(srt.default_camera())
    pt.render(spp=spp // 2, bounces=bounces, seed=seed)
    pt.bind_output(None, pt.half_ptr())
    pt.render(spp=spp // 2, bounces=bounces, seed=seed ^ 0x9E3779B9)
    pt.bind_output()
    pt.render_gbuffer()
    pt.variance(albedo=True, merge=True, gbuffer=False)
    pt.denoise_variance(gbuffer=False, framebuffer=True)
    res = dict(denoised=pt.denoised(), variance=pt.variance_map(), acc=pt.accumulator(), fb=pt.framebuffer())
    pt.close()
    return res


def test_host_renderer_and_cli_equal_the_library_path(srt, tmp_path):
    w, h = 96, 64
    want = _library_frame(srt, w, h, 8, 2, 0)
    r = srt.host.Renderer(w, h)
    r.set_scene(srt.host.Scene(scene_path("Scene1")))
    r.settings(fov=55, max_bounces=2, seed=0)
    for spp in (0, 1, 3):
        with pytest.raises(RuntimeError):
            r.denoise_variance(spp)
    r.denoise_variance(8, framebuffer=True)
    assert _same_bits(r.denoised(), want["denoised"]) and _same_bits(r.variance_map(), want["variance"])
    assert _same_bits(r.accumulator(), want["acc"]) and np.array_equal(r.framebuffer(), want["fb"])
    r.render_samples(2)  # a later render starts afresh, into the accumulator (the binding was restored)
    assert not _same_bits(r.accumulator(), want["acc"])
    r.close()
    base = [CLI, "--scene", scene_path("Scene1"), "--width", str(w), "--height", str(h), "--spp", "8", "--bounces", "2"]
    r1 = subprocess.run(base + ["--out", str(tmp_path / "a.ppm")], capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr[-2000:]
    r2 = subprocess.run(base + ["--out", str(tmp_path / "b.ppm"), "--denoise-variance", str(tmp_path / "v.ppm")], capture_output=True,
                        text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr[-2000:]
    assert (tmp_path / "a.ppm").read_bytes() == (tmp_path / "b.ppm").read_bytes()
    assert np.array_equal(_ppm_rgb(tmp_path / "v.ppm", w, h), _rgb(want["fb"]))
    assert not np.array_equal(_ppm_rgb(tmp_path / "v.ppm", w, h), _ppm_rgb(tmp_path / "a.ppm", w, h))


def test_scripted_viewer_key(srt, tmp_path):
    if not os.path.exists(VIEWER):
        pytest.fail("srt_viewer not built (make -C software-raytracer_amd/host)")
    w, h = 96, 64
    outs = [str(tmp_path / ("%s.ppm" % n)) for n in "abc"]
    script = tmp_path / "session.txt"
    script.write_text("frames 1\nsave %s\npress V\nframes 2\nsave %s\npress V\nframes 1\nsave %s\n" % tuple(outs))
    r = subprocess.run([VIEWER, "--scene", scene_path("Scene1"), "--width", str(w), "--height", str(h), "--script", str(script)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [_ppm_rgb(p, w, h) for p in outs]
    rr = srt.host.Renderer(w, h)
    rr.set_scene(srt.host.Scene(scene_path("Scene1")))
    rr.render_frame()
    want = [_rgb(rr.framebuffer())]
    rr.denoise_variance(2, framebuffer=True)
    rr.denoise_variance(2, framebuffer=True)
    want.append(_rgb(rr.framebuffer()))
    rr.invalidate()
    rr.render_frame()
    want.append(_rgb(rr.framebuffer()))
    rr.close()
    for i in range(3):
        assert np.array_equal(got[i], want[i]), i
    assert not np.array_equal(got[0], got[1])


# ---- quality ------------------------------------------------------------------------------------------------------------------------
def test_it_denoises_a_real_frame(srt):
    """tools/variance_time.py's procedure: Scene1 at 96 x 64, 8 bounces, two halves of 4 spp against 2048 spp of the same library;
    MSE of the tone-mapped values over hit pixels.  The condition: srt_denoise_variance at its defaults is below the unfiltered
    merged mean.  srt_denoise's figure on the same merged mean is computed and printed next to it; no ratio against it is
    asserted.  The three figures on the MI355X have NOT been recorded yet (the test prints them; `tools/variance_time.py quality`
writes the line that belongs in profiles/denoise/variance_quality.jsonl)."""
    spec = importlib.util.spec_from_file_location("variance_time", os.path.join(ROOT, "tools", "variance_time.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    q = tool.quality_figures(srt)
    print("variance_quality " + json.dumps(q))
    assert q["hit_pixels"] > 1000 and q["mean_variance"] > 0
    assert np.isfinite([q["mse_merged"], q["mse_denoise_variance"], q["mse_denoise"]]).all()
    assert q["mse_denoise_variance"] < q["mse_merged"]
