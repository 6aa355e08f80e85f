"""Anti-aliasing (srt_render_subsamples, srt_bind_subsamples, srt_read_subsamples, srt_antialias_params_default, srt_antialias,
srt_bind_antialiased, srt_read_antialiased; ABI 7 additions): the C-ABI declares and exports them, the ctypes mirrors match the
header, the ABI number stays, the argument checks that need no device are made, the Python layers have the methods and the host
library its delegates.  The float64 definition the GPU test compares with (tests/antialias_reference.py) is checked against
hand-worked cases.  No compute: runs without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from antialias_reference import offsets, resolve
from conftest import ROOT

NEW = ["srt_render_subsamples", "srt_bind_subsamples", "srt_read_subsamples", "srt_antialias_params_default", "srt_antialias",
       "srt_bind_antialiased", "srt_read_antialiased"]


def _header():
    return open(os.path.join(ROOT, "include", "srt_pathtrace.h")).read()


def test_header_declares_and_library_exports_the_antialias_entries(srt):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
        assert n in srt.capi.EXPORTS
    # the eighth entry of the feature is a parameter block's default; both blocks are declared
    assert "srt_subsample_params" in text and "srt_antialias_params" in text
    syms = subprocess.run(["nm", "-D", srt.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (srt_[a-z_0-9]+)", syms))
    assert set(NEW) <= exported
    declared = set(re.findall(r"\b(srt_[a-z_0-9]+)\s*\(", text)) - {"srt_context"}
    assert declared == set(srt.capi.EXPORTS)
    assert len(srt.capi.EXPORTS) == len(set(srt.capi.EXPORTS))


def test_abi_number_and_parameter_layouts(srt):
    assert C.CDLL(srt.lib_path()).srt_abi_version() == 7 == srt.capi.ABI_VERSION
    assert re.search(r"#define SRT_ABI_VERSION 7\b", _header())
    S, A = srt.capi.SubsampleParams, srt.capi.AntialiasParams
    assert srt.SubsampleParams is S and srt.AntialiasParams is A
    assert C.sizeof(S) == 16 and C.sizeof(A) == 12
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("row_begin", 0), ("row_end", 4), ("k", 8), ("flags", 12)]
    assert [(n, getattr(A, n).offset) for n, _ in A._fields_] == [("k", 0), ("source", 4), ("flags", 8)]
    for name, cls in (("srt_subsample_params", S), ("srt_antialias_params", A)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), re.S)
        assert re.findall(r"(?:u?int32_t|float) (\w+);", m.group(1)) == [n for n, _ in cls._fields_]
    defs = dict(re.findall(r"#define (SRT_AA_\w+) (\d+)u?\b", _header()))
    assert defs == {"SRT_AA_FRAMEBUFFER": "2", "SRT_AA_SOURCE_ACCUMULATOR": "0", "SRT_AA_SOURCE_DENOISED": "1"}
    assert (srt.capi.AA_FRAMEBUFFER, srt.capi.AA_SOURCE_ACCUMULATOR, srt.capi.AA_SOURCE_DENOISED) == (2, 0, 1)
    # the earlier passes' parameter blocks keep their sizes
    assert C.sizeof(srt.capi.DenoiseParams) == 20 and C.sizeof(srt.capi.TemporalParams) == 20 and C.sizeof(srt.capi.UpsampleParams) == 20


def test_null_arguments_are_invalid_arg_without_a_gpu(srt):
    L = srt.load_library()
    s, a = srt.capi.SubsampleParams(0, 1, 2, 0), srt.capi.AntialiasParams()
    bad = srt.capi.ERR_INVALID_ARG
    assert L.srt_antialias_params_default(None) == bad
    assert L.srt_render_subsamples(None, C.byref(s)) == bad and L.srt_render_subsamples(None, None) == bad
    assert L.srt_antialias(None, C.byref(a)) == bad and L.srt_antialias(None, None) == bad
    assert L.srt_bind_subsamples(None, None) == bad and L.srt_bind_antialiased(None, None) == bad
    assert L.srt_read_subsamples(None, (C.c_int32 * 4)()) == bad
    assert L.srt_read_antialiased(None, (C.c_float * 4)()) == bad


def test_defaults_are_readable_without_a_device(srt):
    d = srt.capi.antialias_defaults()
    assert d == srt.capi.ANTIALIAS_DEFAULTS == {"k": 2, "source": srt.capi.AA_SOURCE_ACCUMULATOR, "flags": 0}
    p = srt.capi.antialias_params(k=3, denoised=True, framebuffer=True)
    assert (p.k, p.source, p.flags) == (3, 1, 2)
    p = srt.capi.antialias_params()
    assert (p.k, p.source, p.flags) == (2, 0, 0)


def test_python_layers_have_the_new_methods(srt):
    for n in ("render_subsamples", "bind_subsamples", "subsamples", "antialias", "bind_antialiased", "antialiased"):
        assert callable(getattr(srt.PathTracer, n)), n
    for n in ("antialias", "antialiased", "set_antialias"):
        assert callable(getattr(srt.host.Renderer, n)), n


def test_host_library_exports_the_antialias_delegates(srt):
    L = C.CDLL(os.path.join(os.path.dirname(srt.lib_path()), "libsrt_host.so"))
    for n in ("srt_host_renderer_antialias", "srt_host_renderer_read_antialiased", "srt_host_renderer_set_antialias"):
        assert n in srt.host.EXPORTS
        assert hasattr(L, n), n


# ---- the float64 definition against cases worked by hand --------------------------------------------------------------------
def test_offsets_are_exact():
    assert offsets(1).tolist() == [0.0]
    assert offsets(2).tolist() == [-0.25, 0.25]
    assert offsets(4).tolist() == [-0.375, -0.125, 0.125, 0.375]
    o3 = offsets(3)
    assert o3[1] == 0.0 and o3[2] == np.float32(2) / np.float32(6) and o3[0] == -o3[2]


def _colours(h, w, seed=3):
    c = np.random.default_rng(seed).uniform(0.05, 4.0, (h, w, 4)).astype(np.float32)
    return c


def test_vertical_edge_with_two_of_four_foreign():
    h, w = 3, 4
    obj = np.zeros((h, w), np.int32)
    obj[:, 2:] = 1
    sub = np.broadcast_to(obj, (4, h, w)).copy()
    sub[1, 1, 1] = sub[3, 1, 1] = 1  # pixel (1, 1): its two right-hand sub-samples (i = 1) see the neighbour's object
    c = _colours(h, w)
    c[:, :2, :3] = [1.0, 2.0, 0.5]   # one colour per object
    c[:, 2:, :3] = [3.0, 0.25, 1.5]
    out, foreign, changed = resolve(c, obj, sub)
    assert foreign.sum() == 1 and foreign[1, 1] and changed[1, 1] and changed.sum() == 1
    want = (2 * c[1, 1, :3].astype(np.float64) + 2 * c[1, 2, :3].astype(np.float64)) / 4
    assert np.allclose(out[1, 1, :3], want, rtol=1e-15)
    assert out[1, 1, 3] == c[1, 1, 3]
    keep = np.ones((h, w), bool)
    keep[1, 1] = False
    assert np.array_equal(out[keep], c[keep].astype(np.float64))
    # with a colour per pixel: sub-sample (i, j) = (1, 0) sits at (+0.25, -0.25), its footprint is columns x, x + 1 and rows
    # y - 1, y; of those only column x + 1 holds object 1: weights 0.25 * 0.25 and 0.25 * 0.75 -> (c[0, 2] + 3 c[1, 2]) / 4;
    # sub-sample (1, 1) at (+0.25, +0.25) alike with row y + 1
    c = _colours(h, w, seed=8)
    out, _, _ = resolve(c, obj, sub)
    d = c[..., :3].astype(np.float64)
    want = (2 * d[1, 1] + (d[0, 2] + 3 * d[1, 2]) / 4 + (3 * d[1, 2] + d[2, 2]) / 4) / 4
    assert np.allclose(out[1, 1, :3], want, rtol=1e-15)


def test_frame_corner_and_fallback():
    h, w = 3, 3
    obj = np.zeros((h, w), np.int32)
    obj[1, 1] = 2
    obj[0, 1] = 5
    c = _colours(h, w, seed=4)
    d = c[..., :3].astype(np.float64)
    sub = np.zeros((4, h, w), np.int32)
    sub[1:, 1, 1] = 2  # (keep the centre pixel interior apart from the plane below)
    sub[:, 0, 1] = 5
    # corner pixel (0, 0): sub-sample 0 points out of the frame at (-0.25, -0.25) and holds object 5, which pixel (1, 0) has,
    # but its footprint is columns -1, 0 and rows -1, 0: the taps outside are skipped, the one inside is the pixel itself -> fallback.
    # sub-sample 3 at (+0.25, +0.25) holds object 2: of its footprint (0..1, 0..1) only pixel (1, 1) has it -> C = c[1, 1]
    sub[0, 0, 0] = 5
    sub[3, 0, 0] = 2
    sub[0, 1, 1] = 77  # an object no pixel has: fallback, the pixel keeps its bits
    out, foreign, changed = resolve(c, obj, sub)
    assert foreign[0, 0] and foreign[1, 1] and foreign.sum() == 2
    assert changed[0, 0] and not changed[1, 1] and changed.sum() == 1
    assert np.allclose(out[0, 0, :3], (3 * d[0, 0] + d[1, 1]) / 4, rtol=1e-15)
    assert np.array_equal(out[1, 1], c[1, 1].astype(np.float64))
    # k = 1 is the identity whatever the plane holds that no neighbour has; an own plane is the identity too
    out, _, changed = resolve(c, obj, obj[None].copy())
    assert not changed.any() and np.array_equal(out, c.astype(np.float64))
    # a non-finite colour on another object does not reach a pixel none of whose sub-samples holds that object
    c2 = c.copy()
    c2[0, 1, :3] = np.nan
    out2, _, _ = resolve(c2, obj, sub)
    assert np.allclose(out2[0, 0, :3], (3 * d[0, 0] + d[1, 1]) / 4, rtol=1e-15)
