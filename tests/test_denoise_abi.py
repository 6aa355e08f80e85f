"""Denoiser (srt_denoise, ABI 7 addition): the C-ABI declares and exports srt_denoise_params_default / srt_denoise /
srt_bind_denoised / srt_read_denoised, the ctypes mirror matches the header, the defaults come from the library, and the
host library exports its delegates.  No compute: runs without a GPU."""
import ctypes as C
import math
import os
import re
import subprocess

from conftest import ROOT

NEW = ["srt_denoise_params_default", "srt_denoise", "srt_bind_denoised", "srt_read_denoised"]


def _header():
    return open(os.path.join(ROOT, "include", "srt_pathtrace.h")).read()


def test_header_declares_and_library_exports_the_denoise_entries(srt):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
        assert n in srt.capi.EXPORTS
    syms = subprocess.run(["nm", "-D", srt.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (srt_[a-z_0-9]+)", syms))
    assert set(NEW) <= exported
    # backward-compatible additions: the ABI number stays
    assert C.CDLL(srt.lib_path()).srt_abi_version() == 7 == srt.capi.ABI_VERSION
    bits = dict(re.findall(r"#define (SRT_DENOISE_\w+) (\d+)u", _header()))
    assert bits == {"SRT_DENOISE_ALBEDO": "1", "SRT_DENOISE_FRAMEBUFFER": "2"}
    assert (srt.capi.DENOISE_ALBEDO, srt.capi.DENOISE_FRAMEBUFFER) == (1, 2)


def test_denoise_params_layout_matches_the_header(srt):
    D = srt.capi.DenoiseParams
    assert D is srt.DenoiseParams
    assert C.sizeof(D) == 20
    m = re.search(r"typedef struct srt_denoise_params \{(.*?)\} srt_denoise_params;", _header(), re.S)
    fields = re.findall(r"(?:u?int32_t|float) (\w+);", m.group(1))
    assert fields == [n for n, _ in D._fields_] == ["iterations", "sigma_color", "sigma_normal", "sigma_plane", "flags"]
    assert [getattr(D, f).offset for f in fields] == [0, 4, 8, 12, 16]


def test_defaults_come_from_the_library_without_a_gpu(srt):
    L = srt.load_library()
    p = srt.capi.DenoiseParams(-1, -1.0, -1.0, -1.0, 99)
    assert L.srt_denoise_params_default(C.byref(p)) == srt.capi.OK
    assert L.srt_denoise_params_default(None) == srt.capi.ERR_INVALID_ARG
    got = {n: getattr(p, n) for n, _ in srt.capi.DenoiseParams._fields_}
    # the documented defaults
    assert got["iterations"] == 4 and got["flags"] == srt.capi.DENOISE_ALBEDO
    assert got["sigma_color"] == 0.0 and got["sigma_normal"] == 32.0
    assert math.isclose(got["sigma_plane"], 0.02, rel_tol=1e-6)
    assert srt.capi.DENOISE_DEFAULTS == got
    q = srt.capi.denoise_params(iterations=3, albedo=False, framebuffer=True)
    assert (q.iterations, q.sigma_normal, q.flags) == (3, 32.0, srt.capi.DENOISE_FRAMEBUFFER)


def test_null_context_or_params_is_invalid_arg_without_a_gpu(srt):
    L = srt.load_library()
    p = srt.capi.DenoiseParams(5, 0.0, 128.0, 0.02, 1)
    assert L.srt_denoise(None, C.byref(p)) == srt.capi.ERR_INVALID_ARG
    assert L.srt_denoise(None, None) == srt.capi.ERR_INVALID_ARG
    assert L.srt_bind_denoised(None, None) == srt.capi.ERR_INVALID_ARG
    buf = (C.c_float * 4)()
    assert L.srt_read_denoised(None, buf) == srt.capi.ERR_INVALID_ARG


def test_host_library_exports_the_denoise_delegates(srt):
    L = C.CDLL(os.path.join(os.path.dirname(srt.lib_path()), "libsrt_host.so"))
    for n in ("srt_host_renderer_denoise", "srt_host_renderer_read_denoised"):
        assert n in srt.host.EXPORTS
        assert hasattr(L, n), n
