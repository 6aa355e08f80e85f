"""Temporal reprojection (srt_temporal_accumulate, ABI 7 addition): the C-ABI declares and exports
srt_temporal_params_default / srt_temporal_accumulate / srt_read_history_length, the ctypes mirror matches the header, the
defaults come from the library, and the host library exports its delegates.  No compute: runs without a GPU."""
import ctypes as C
import math
import os
import re
import subprocess

from conftest import ROOT

NEW = ["srt_temporal_params_default", "srt_temporal_accumulate", "srt_read_history_length"]


def _header():
    return open(os.path.join(ROOT, "include", "srt_pathtrace.h")).read()


def test_header_declares_and_library_exports_the_temporal_entries(srt):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NEW:
        assert re.fullmatch(r"srt_[a-z_]+", n), n
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
        assert n in srt.capi.EXPORTS
    syms = subprocess.run(["nm", "-D", srt.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (srt_[a-z_0-9]+)", syms))
    assert set(NEW) <= exported
    # capi.EXPORTS is exactly what the header declares
    declared = set(re.findall(r"\b(srt_[a-z_0-9]+)\s*\(", text)) - {"srt_context"}
    assert declared == set(srt.capi.EXPORTS)
    # backward-compatible additions: the ABI number stays
    assert C.CDLL(srt.lib_path()).srt_abi_version() == 7 == srt.capi.ABI_VERSION
    bits = dict(re.findall(r"#define (SRT_TEMPORAL_\w+) (\d+)u", _header()))
    assert bits == {"SRT_TEMPORAL_RESET": "1", "SRT_TEMPORAL_FRAMEBUFFER": "2"}
    assert (srt.capi.TEMPORAL_RESET, srt.capi.TEMPORAL_FRAMEBUFFER) == (1, 2)


def test_temporal_params_layout_matches_the_header(srt):
    T = srt.capi.TemporalParams
    assert T is srt.TemporalParams
    assert C.sizeof(T) == 20
    m = re.search(r"typedef struct srt_temporal_params \{(.*?)\} srt_temporal_params;", _header(), re.S)
    fields = re.findall(r"(?:u?int32_t|float) (\w+);", m.group(1))
    assert fields == [n for n, _ in T._fields_] == ["samples", "max_samples", "plane_tolerance", "normal_threshold", "flags"]
    assert [getattr(T, f).offset for f in fields] == [0, 4, 8, 12, 16]


def test_defaults_come_from_the_library_without_a_gpu(srt):
    L = srt.load_library()
    p = srt.capi.TemporalParams(0, -1.0, -1.0, -5.0, 99)
    assert L.srt_temporal_params_default(C.byref(p)) == srt.capi.OK
    assert L.srt_temporal_params_default(None) == srt.capi.ERR_INVALID_ARG
    got = {n: getattr(p, n) for n, _ in srt.capi.TemporalParams._fields_}
    # the documented defaults
    assert got["samples"] == 1 and got["flags"] == 0
    assert got["max_samples"] == 32.0
    assert math.isclose(got["plane_tolerance"], 0.02, rel_tol=1e-6)
    assert math.isclose(got["normal_threshold"], 0.9, rel_tol=1e-6)
    assert srt.capi.TEMPORAL_DEFAULTS == got
    q = srt.capi.temporal_params(samples=4, max_samples=64.0, reset=True, framebuffer=True)
    assert (q.samples, q.max_samples, q.flags) == (4, 64.0, srt.capi.TEMPORAL_RESET | srt.capi.TEMPORAL_FRAMEBUFFER)
    assert math.isclose(q.plane_tolerance, 0.02, rel_tol=1e-6)


def test_null_context_or_params_is_invalid_arg_without_a_gpu(srt):
    L = srt.load_library()
    p = srt.capi.temporal_params()
    assert L.srt_temporal_accumulate(None, C.byref(p)) == srt.capi.ERR_INVALID_ARG
    assert L.srt_temporal_accumulate(None, None) == srt.capi.ERR_INVALID_ARG
    buf = (C.c_float * 4)()
    assert L.srt_read_history_length(None, buf) == srt.capi.ERR_INVALID_ARG


def test_host_library_exports_the_temporal_delegates(srt):
    L = C.CDLL(os.path.join(os.path.dirname(srt.lib_path()), "libsrt_host.so"))
    for n in ("srt_host_renderer_temporal", "srt_host_renderer_read_history_length", "srt_host_renderer_render_temporal_frame",
              "srt_host_renderer_move_camera"):
        assert n in srt.host.EXPORTS
        assert hasattr(L, n), n
