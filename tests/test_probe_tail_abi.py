"""The probe tail (srt_probe_tail, srt_probe_tail_params_default, srt_get_probe_tail_work; ABI 7 additions): the C-ABI declares and
exports the entries, srt_probe_tail_params (32 bytes) and srt_probe_tail_work (56 bytes) have the same layout in ctypes and in C,
the constants agree, the ABI number stays, the defaults are readable without a device, NULL arguments are refused before a device
is touched, and the Python layers and the host library have their entries.  No compute: runs without a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

NEW = ["srt_probe_tail_params_default", "srt_probe_tail", "srt_get_probe_tail_work"]


def _header():
    return open(os.path.join(ROOT, "include", "srt_pathtrace.h")).read()


def test_header_declares_and_library_exports_the_entries(srt):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    syms = subprocess.run(["nm", "-D", srt.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (srt_[a-z_0-9]+)", syms))
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
        assert n in srt.capi.EXPORTS and n in exported, n
    assert C.CDLL(srt.lib_path()).srt_abi_version() == 7 == srt.capi.ABI_VERSION
    m = re.search(r"/\* ---- probe tail.*?\*/", _header(), re.S)
    assert m and "(ABI 7, backward compatible)" in m.group(0) and "SRT_ABI_VERSION stays 7" in m.group(0)
    for rule in ("T1.", "T2.", "T3.", "T4.", "T5.", "T6.", "g = 1.0f - (Smoothness * spec)", "k_l = (T_l * 0.8f) * g", "x + n * .00001f", "wave_lookups"):
        assert rule in m.group(0), rule
    assert dict(re.findall(r"#define (SRT_PROBE_TAIL_\w+) +(\d+)u\b", _header())) == {
        "SRT_PROBE_TAIL_NORMAL_WEIGHT": "1", "SRT_PROBE_TAIL_DEPTH": "2", "SRT_PROBE_TAIL_STATES": "4", "SRT_PROBE_TAIL_COUNT_WORK": "8"}


def test_struct_sizes_layouts_and_constants(srt):
    c = srt.capi
    P, W = c.ProbeTailParams, c.ProbeTailWork
    assert srt.ProbeTailParams is P and srt.ProbeTailWork is W
    assert (C.sizeof(P), C.sizeof(W)) == (32, 56)
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("enabled", 0), ("flags", 4), ("band_weight", 8), ("bias", 20), ("min_variance", 24),
                                                                  ("reserved", 28)]
    assert [(n, getattr(W, n).offset) for n, _ in W._fields_] == [("valid", 0), ("reserved", 4), ("tails", 8), ("corners", 16), ("open", 24), ("dark", 32),
                                                                  ("mirror_ends", 40), ("wave_lookups", 48)]
    for name, mirror in (("srt_probe_tail_params", P), ("srt_probe_tail_work", W)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), re.S)
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        names = [re.sub(r"\[\d+\]", "", x.strip()) for decl in re.findall(r"(?:u?int(?:32|64)_t|float) ([\w, \[\]]+);", body) for x in decl.split(",")]
        assert names == [n for n, _ in mirror._fields_], name
    assert (c.PROBE_TAIL_NORMAL_WEIGHT, c.PROBE_TAIL_DEPTH, c.PROBE_TAIL_STATES, c.PROBE_TAIL_COUNT_WORK) == (1, 2, 4, 8)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_layout_in_c(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "srt_pathtrace.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(srt_probe_tail_params), '
                   'offsetof(srt_probe_tail_params, flags), offsetof(srt_probe_tail_params, band_weight), offsetof(srt_probe_tail_params, bias), '
                   'offsetof(srt_probe_tail_params, min_variance), offsetof(srt_probe_tail_params, reserved), sizeof(srt_probe_tail_work), '
                   'offsetof(srt_probe_tail_work, tails), offsetof(srt_probe_tail_work, dark), offsetof(srt_probe_tail_work, mirror_ends), '
                   'offsetof(srt_probe_tail_work, wave_lookups)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["32", "4", "8", "20", "24", "28", "56", "8", "32", "40", "48"]


def test_defaults_and_null_arguments_without_a_gpu(srt):
    L = srt.load_library()
    c = srt.capi
    p = c.ProbeTailParams(7, 0xFFFFFFFF, (9.0, 9.0, 9.0), -1.0, -1.0, 5)
    assert L.srt_probe_tail_params_default(C.byref(p)) == c.OK
    assert (p.enabled, p.flags, list(p.band_weight), p.bias, p.min_variance, p.reserved) == (1, 0, [1.0, 0.5, 0.0], 0.0, C.c_float(1e-4).value, 0)
    bad = c.ERR_INVALID_ARG
    assert L.srt_probe_tail_params_default(None) == bad
    assert L.srt_probe_tail(None, C.byref(p)) == bad and L.srt_probe_tail(None, None) == bad
    w = c.ProbeTailWork()
    assert L.srt_get_probe_tail_work(None, C.byref(w)) == bad


def test_python_layers_and_host_library_have_the_new_entries(srt):
    for n in ("probe_tail", "probe_tail_work"):
        assert callable(getattr(srt.PathTracer, n)) and callable(getattr(srt.host.Renderer, n)), n
    L = C.CDLL(os.path.join(os.path.dirname(srt.lib_path()), "libsrt_host.so"))
    for n in ("srt_host_renderer_probe_tail", "srt_host_renderer_probe_tail_work"):
        assert n in srt.host.EXPORTS and hasattr(L, n), n
