"""Guided upsampler (srt_upsample_params_default, srt_upsample, srt_bind_upsampled, srt_read_upsampled; ABI 7 additions): the
C-ABI declares and exports them, the ctypes mirror matches the header, the ABI number stays, the Python layers have the
methods, the host library exports its delegates and the defaults are readable without a device.  No compute: runs without a
GPU."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

NEW = ["srt_upsample_params_default", "srt_upsample", "srt_bind_upsampled", "srt_read_upsampled"]


def _header():
    return open(os.path.join(ROOT, "include", "srt_pathtrace.h")).read()


def test_header_declares_and_library_exports_the_upsample_entries(srt):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
        assert n in srt.capi.EXPORTS
    syms = subprocess.run(["nm", "-D", srt.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (srt_[a-z_0-9]+)", syms))
    assert set(NEW) <= exported
    # capi.EXPORTS is exactly what the header declares
    declared = set(re.findall(r"\b(srt_[a-z_0-9]+)\s*\(", text)) - {"srt_context"}
    assert declared == set(srt.capi.EXPORTS)
    assert len(srt.capi.EXPORTS) == len(set(srt.capi.EXPORTS))


def test_abi_number_and_parameter_layout(srt):
    assert C.CDLL(srt.lib_path()).srt_abi_version() == 7 == srt.capi.ABI_VERSION
    assert re.search(r"#define SRT_ABI_VERSION 7\b", _header())
    assert C.sizeof(srt.capi.UpsampleParams) == 20
    assert srt.UpsampleParams is srt.capi.UpsampleParams
    # the ctypes mirror lists the header's fields in the header's order
    m = re.search(r"typedef struct srt_upsample_params \{(.*?)\} srt_upsample_params;", _header(), re.S)
    assert re.findall(r"(?:u?int32_t|float) (\w+);", m.group(1)) == [n for n, _ in srt.capi.UpsampleParams._fields_]
    bits = dict(re.findall(r"#define (SRT_UPSAMPLE_\w+) (\d+)u", _header()))
    assert bits == {"SRT_UPSAMPLE_IN_PLACE": "1", "SRT_UPSAMPLE_FRAMEBUFFER": "2"}
    assert (srt.capi.UPSAMPLE_IN_PLACE, srt.capi.UPSAMPLE_FRAMEBUFFER) == (1, 2)
    # the earlier passes' parameter blocks keep their sizes
    assert C.sizeof(srt.capi.DenoiseParams) == 20 and C.sizeof(srt.capi.TemporalParams) == 20


def test_null_arguments_are_invalid_arg_without_a_gpu(srt):
    L = srt.load_library()
    p = srt.capi.UpsampleParams()
    assert L.srt_upsample_params_default(None) == srt.capi.ERR_INVALID_ARG
    assert L.srt_upsample(None, C.byref(p)) == srt.capi.ERR_INVALID_ARG
    assert L.srt_upsample(None, None) == srt.capi.ERR_INVALID_ARG
    assert L.srt_bind_upsampled(None, None) == srt.capi.ERR_INVALID_ARG
    buf = (C.c_float * 4)()
    assert L.srt_read_upsampled(None, buf) == srt.capi.ERR_INVALID_ARG


def test_defaults_are_readable_without_a_device(srt):
    d = srt.capi.upsample_defaults()
    assert d == srt.capi.UPSAMPLE_DEFAULTS
    assert d["steps"] == 2 and d["stripe_width"] == 0 and d["flags"] == 0
    # the denoiser's normal and plane sigmas
    dn = srt.capi.denoise_defaults()
    assert d["sigma_normal"] == dn["sigma_normal"] == 32.0
    assert abs(d["sigma_plane"] - 0.02) < 1e-9 and d["sigma_plane"] == dn["sigma_plane"]
    p = srt.capi.upsample_params(steps=8, stripe_width=17, sigma_plane=0.0, in_place=True, framebuffer=True)
    assert (p.steps, p.stripe_width, p.sigma_normal, p.sigma_plane, p.flags) == (8, 17, 32.0, 0.0, 3)


def test_python_layers_have_the_new_methods(srt):
    for n in ("upsample", "bind_upsampled", "upsampled"):
        assert callable(getattr(srt.PathTracer, n)), n
    for n in ("upsample", "upsampled", "guided_upsample"):
        assert callable(getattr(srt.host.Renderer, n)), n
    assert callable(srt.capi.upsample_defaults)


def test_host_library_exports_the_upsample_delegates(srt):
    L = C.CDLL(os.path.join(os.path.dirname(srt.lib_path()), "libsrt_host.so"))
    for n in ("srt_host_renderer_upsample", "srt_host_renderer_read_upsampled", "srt_host_renderer_guided_upsample"):
        assert n in srt.host.EXPORTS
        assert hasattr(L, n), n
