"""Variance estimate and variance-guided denoiser (srt_variance_params_default, srt_device_half, srt_bind_half, srt_variance,
srt_bind_variance, srt_read_variance, srt_denoise_variance_params_default, srt_denoise_variance; ABI 7 additions): the C-ABI
declares and exports them, the ctypes mirrors match the header, the ABI number stays, both defaults are readable without a
device, the Python layers have the methods and the host library its delegates.  The float64 definition the GPU test compares
with (tests/variance_reference.py) is checked against hand-worked cases.  No compute: runs without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import variance_reference as vr
from conftest import ROOT

NEW = ["srt_variance_params_default", "srt_device_half", "srt_bind_half", "srt_variance", "srt_bind_variance", "srt_read_variance",
       "srt_denoise_variance_params_default", "srt_denoise_variance"]


def _header():
    return open(os.path.join(ROOT, "include", "srt_pathtrace.h")).read()


def test_header_declares_and_library_exports_the_variance_entries(srt):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
        assert n in srt.capi.EXPORTS
    syms = subprocess.run(["nm", "-D", srt.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (srt_[a-z_0-9]+)", syms))
    assert set(NEW) <= exported
    declared = set(re.findall(r"\b(srt_[a-z_0-9]+)\s*\(", text)) - {"srt_context"}
    assert declared == set(srt.capi.EXPORTS) == exported
    assert len(srt.capi.EXPORTS) == len(set(srt.capi.EXPORTS))
    # below the anti-aliasing block, above the buffers the worker writes
    assert _header().index("srt_read_antialiased(") < _header().index("srt_variance_params_default(") < _header().index("srt_read_framebuffer(")


def test_abi_number_and_parameter_layouts(srt):
    assert C.CDLL(srt.lib_path()).srt_abi_version() == 7 == srt.capi.ABI_VERSION
    assert re.search(r"#define SRT_ABI_VERSION 7\b", _header())
    V, D = srt.capi.VarianceParams, srt.capi.DenoiseVarianceParams
    assert srt.VarianceParams is V and srt.DenoiseVarianceParams is D
    assert C.sizeof(V) == 4 and C.sizeof(D) == 20
    assert [(n, getattr(V, n).offset) for n, _ in V._fields_] == [("flags", 0)]
    assert [(n, getattr(D, n).offset) for n, _ in D._fields_] == [("iterations", 0), ("sigma_luminance", 4), ("sigma_normal", 8),
                                                                  ("sigma_plane", 12), ("flags", 16)]
    for name, cls in (("srt_variance_params", V), ("srt_denoise_variance_params", D)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), re.S)
        assert re.findall(r"(?:u?int32_t|float) (\w+);", m.group(1)) == [n for n, _ in cls._fields_]
    defs = dict(re.findall(r"#define (SRT_VARIANCE_\w+) (\d+)u?\b", _header()))
    assert defs == {"SRT_VARIANCE_ALBEDO": "1", "SRT_VARIANCE_MERGE": "2"}
    assert (srt.capi.VARIANCE_ALBEDO, srt.capi.VARIANCE_MERGE) == (1, 2)
    # the earlier passes' parameter blocks keep their sizes
    assert C.sizeof(srt.capi.DenoiseParams) == 20 and C.sizeof(srt.capi.AntialiasParams) == 12


def test_defaults_are_readable_without_a_device(srt):
    v = srt.capi.variance_defaults()
    assert v == srt.capi.VARIANCE_DEFAULTS == {"flags": srt.capi.VARIANCE_ALBEDO | srt.capi.VARIANCE_MERGE}
    d, dn = srt.capi.denoise_variance_defaults(), srt.capi.denoise_defaults()
    assert d == srt.capi.DENOISE_VARIANCE_DEFAULTS
    assert d["sigma_luminance"] == 4.0
    assert all(d[k] == dn[k] for k in ("iterations", "sigma_normal", "sigma_plane", "flags"))
    p = srt.capi.denoise_variance_params(iterations=3, sigma_luminance=1.5, albedo=False, framebuffer=True)
    assert (p.iterations, p.sigma_luminance, p.sigma_normal, p.sigma_plane, p.flags) == (3, 1.5, dn["sigma_normal"], dn["sigma_plane"], 2)
    assert srt.capi.variance_params().flags == 3 and srt.capi.variance_params(albedo=False).flags == 2
    assert srt.capi.variance_params(albedo=True, merge=False).flags == 1


def test_null_arguments_are_invalid_arg_without_a_gpu(srt):
    L = srt.load_library()
    bad = srt.capi.ERR_INVALID_ARG
    v, d, p = srt.capi.VarianceParams(), srt.capi.DenoiseVarianceParams(), C.c_void_p()
    assert L.srt_variance_params_default(None) == bad and L.srt_denoise_variance_params_default(None) == bad
    assert L.srt_device_half(None, C.byref(p)) == bad and L.srt_bind_half(None, None) == bad
    assert L.srt_variance(None, C.byref(v)) == bad and L.srt_variance(None, None) == bad
    assert L.srt_bind_variance(None, None) == bad and L.srt_read_variance(None, (C.c_float * 4)()) == bad
    assert L.srt_denoise_variance(None, C.byref(d)) == bad and L.srt_denoise_variance(None, None) == bad


def test_python_layers_and_host_library_have_the_new_entries(srt):
    for n in ("half_ptr", "bind_half", "variance", "variance_map", "bind_variance", "denoise_variance"):
        assert callable(getattr(srt.PathTracer, n)), n
    for n in ("denoise_variance", "variance_map"):
        assert callable(getattr(srt.host.Renderer, n)), n
    L = C.CDLL(os.path.join(os.path.dirname(srt.lib_path()), "libsrt_host.so"))
    for n in ("srt_host_renderer_denoise_variance", "srt_host_renderer_read_variance"):
        assert n in srt.host.EXPORTS and hasattr(L, n), n


def test_cli_refuses_bad_denoise_variance_arguments_before_touching_a_device(tmp_path):
    cli = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
    scene = os.path.join(ROOT, "software-raytracer_amd", "scenes", "Scene1.json")
    base = [cli, "--scene", scene, "--width", "16", "--height", "8", "--out", str(tmp_path / "x.ppm")]
    for extra in (["--spp", "1"], ["--spp", "3"], ["--spp", "4", "--denoise", str(tmp_path / "d.ppm")], ["--spp", "4", "--temporal", "2"]):
        r = subprocess.run(base + extra + ["--denoise-variance", str(tmp_path / "v.ppm")], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--denoise-variance" in r.stderr, (extra, r.stderr)
        assert not (tmp_path / "x.ppm").exists()


# ---- the float64 definition against cases worked by hand ----------------------------------------------------------------------
def _f32(*v):
    return np.array(v, np.float32)


def test_reference_estimate_by_hand():
    a = np.zeros((1, 3, 4), np.float32)
    b = np.zeros((1, 3, 4), np.float32)
    a[0, :, :3] = [1.0, 2.0, 4.0]
    b[0, :, :3] = [3.0, 2.0, 0.0]
    obj = np.array([[0, 0, -1]], np.int32)
    alb = np.zeros((1, 3, 4), np.float32)
    alb[0, :, :3] = [0.5, 0.25, 5e-4]  # the last channel is below 1e-3: not divided
    v, mean = vr.variance(a, b, obj, alb, albedo=False)
    l = [float(np.float32(x)) for x in (0.2126, 0.7152, 0.0722)]
    d = 0.5 * (l[0] * 1 + l[1] * 2 + l[2] * 4) - 0.5 * (l[0] * 3 + l[1] * 2)
    assert np.allclose(v[0, :2], d * d, rtol=1e-14) and v[0, 2] == 0.0
    assert np.array_equal(mean[0, 2], [2.0, 2.0, 2.0])  # misses are merged too
    v, _ = vr.variance(a, b, obj, alb, albedo=True)
    d = 0.5 * (l[0] * 1 / 0.5 + l[1] * 2 / 0.25 + l[2] * 4) - 0.5 * (l[0] * 3 / 0.5 + l[1] * 2 / 0.25)
    assert np.allclose(v[0, :2], d * d, rtol=1e-14)
    # equal halves: +0; swapped halves: the same value
    assert np.array_equal(vr.variance(a, a, obj, alb, True)[0], np.zeros((1, 3)))
    assert np.array_equal(vr.variance(b, a, obj, alb, True)[0], v)


def test_reference_prefilter_by_hand():
    obj = np.array([[0, 0, 1], [0, 1, 1], [-1, 0, 0]], np.int32)
    v = np.arange(1.0, 10.0).reshape(3, 3)
    g = vr.prefilter(v, obj)
    # centre (1, 1), object 1: itself (4/16), right (1, 2) (2/16), up-right (0, 2) (1/16)
    assert np.isclose(g[1, 1], (4 * 5 + 2 * 6 + 1 * 3) / 7, rtol=1e-15)
    # corner (0, 0), object 0: itself 4, right 2, below 2; the diagonal is object 1
    assert np.isclose(g[0, 0], (4 * 1 + 2 * 2 + 2 * 4) / 8, rtol=1e-15)
    # a pixel alone in its object keeps its value, NaN on another object does not reach it
    v2 = v.copy()
    v2[obj != 1] = np.nan
    assert np.isclose(vr.prefilter(v2, obj)[1, 1], g[1, 1], rtol=1e-15)


def _flat(h, w):
    obj = np.zeros((h, w), np.int32)
    nd = np.zeros((h, w, 4), np.float32)
    nd[..., 2], nd[..., 3] = -1.0, 2.0
    pos = np.zeros((h, w, 4), np.float32)
    alb = np.full((h, w, 4), 0.5, np.float32)
    return obj, nd, pos, alb


def test_reference_filter_by_hand():
    h, w = 5, 5
    obj, nd, pos, alb = _flat(h, w)
    rng = np.random.default_rng(2)
    acc = rng.uniform(0.2, 3.0, (h, w, 4)).astype(np.float32)
    var = rng.uniform(0.1, 1.0, (h, w)).astype(np.float32)
    # all terms off: the plain 5 x 5 binomial mean, and the variance by the squared weights
    lv = []
    out = vr.denoise_variance(acc, var, obj, nd, pos, alb, 1, 0.0, 0.0, 0.0, False, levels_out=lv)
    k = np.outer(vr.H5, vr.H5)
    assert np.allclose(out[2, 2, :3], np.tensordot(k, acc[..., :3].astype(np.float64), 2), rtol=1e-14)
    assert np.isclose(lv[0][2, 2], np.sum(k * k * var), rtol=1e-14)
    assert out[2, 2, 3] == acc[2, 2, 3]
    # corner: the taps outside are skipped and the rest renormalised
    kc = k[2:, 2:]
    assert np.allclose(out[0, 0, :3], np.tensordot(kc, acc[:3, :3, :3].astype(np.float64), 2) / kc.sum(), rtol=1e-14)
    assert np.isclose(lv[0][0, 0], np.sum(kc * kc * var[:3, :3]) / kc.sum() ** 2, rtol=1e-14)
    # zero variance closes the stop at every sigma, +inf included: the output is the input
    zero = np.zeros_like(var)
    for sl in (4.0, np.inf):
        out = vr.denoise_variance(acc, zero, obj, nd, pos, alb, 3, sl, 0.0, 0.0, True)
        assert np.allclose(out[..., :3], acc[..., :3], rtol=1e-12)
    # a huge variance, or +inf sigma on a positive one, opens it: the result of sigma_luminance = 0
    off = vr.denoise_variance(acc, var, obj, nd, pos, alb, 2, 0.0, 0.0, 0.0, True)
    assert np.allclose(vr.denoise_variance(acc, np.full_like(var, 1e30), obj, nd, pos, alb, 2, 4.0, 0.0, 0.0, True), off, rtol=1e-12)
    assert np.allclose(vr.denoise_variance(acc, var, obj, nd, pos, alb, 2, np.inf, 0.0, 0.0, True), off, rtol=1e-12)
    # one tap by hand: a 1 x 2 frame, luminance term only
    obj2, nd2, pos2, alb2 = _flat(1, 2)
    acc2 = np.zeros((1, 2, 4), np.float32)
    acc2[0, 0, :3], acc2[0, 1, :3] = 1.0, 2.0
    var2 = _f32([0.25, 0.25])
    out = vr.denoise_variance(acc2, var2, obj2, nd2, pos2, alb2, 1, 2.0, 0.0, 0.0, False)
    dl = float(np.float32(0.2126)) + float(np.float32(0.7152)) + float(np.float32(0.0722))
    wq = (4 / 16 * 6 / 16) * np.exp(-dl / (2.0 * 0.5 + float(np.float32(1e-10))))
    wc = 36 / 256
    assert np.isclose(out[0, 0, 0], (wc * 1 + wq * 2) / (wc + wq), rtol=1e-14)
    # a miss passes through and is no tap
    obj2[0, 1] = -1
    out = vr.denoise_variance(acc2, var2, obj2, nd2, pos2, alb2, 2, 2.0, 0.0, 0.0, False)
    assert np.array_equal(out, acc2.astype(np.float64))
