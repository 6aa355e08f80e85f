"""Probe classification and relocation and the shading that obeys the records (srt_probe_classify_params_default ...
srt_shade_probe_grid_states; ABI 7 additions): the C-ABI declares and exports them inside their own two blocks, the two structs have
the same layout in ctypes and in a compiled C program, the constants agree, the header sections promise ABI 7 and state the rules,
the defaults work without a device, NULL or impossible arguments are refused before a device is touched, and the upper layers have
the entries.  No compute: runs without a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import probe_states_reference as PS
from conftest import ROOT

CLASSIFY = ["srt_probe_classify_params_default", "srt_classify_probes", "srt_bind_probe_states_output", "srt_read_probe_states_output",
            "srt_get_probe_classify_work"]
SHADE = ["srt_write_probe_grid_states", "srt_bind_probe_grid_states", "srt_shade_probe_grid_states"]
HEAD_CLASSIFY = "/* ---- probe classification and relocation:"
HEAD_SHADE = "/* ---- probe-grid shading that obeys the probe states"
NEXT = "/* ---- probe depth moments:"
DEFINES = {"SRT_PROBE_STATE_RECORDS": "1", "SRT_PROBE_STATE_POSITIONS": "2", "SRT_PROBE_CLASSIFY_RELOCATE": "1", "SRT_PROBE_CLASSIFY_NORMALIZE": "2",
           "SRT_PROBE_CLASSIFY_COUNT_WORK": "4", "SRT_PROBE_CLEAR": "0", "SRT_PROBE_MOVED": "1", "SRT_PROBE_BURIED": "2", "SRT_PROBE_INSIDE": "4", "SRT_PROBE_IDLE": "8"}


def _header():
    return open(os.path.join(ROOT, "include", "srt_pathtrace.h")).read()


def test_header_declares_and_library_exports_the_entries_in_their_blocks(srt):
    h = _header()
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    text = strip(h)
    syms = subprocess.run(["nm", "-D", srt.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (srt_[a-z_0-9]+)", syms))
    for n in CLASSIFY + SHADE:
        assert len(re.findall(r"\bint\s+%s\s*\(" % n, text)) == 1, n
        assert srt.capi.EXPORTS.count(n) == 1 and n in exported, n
    a, b, c = h.index(HEAD_CLASSIFY), h.index(HEAD_SHADE), h.index(NEXT)
    assert h.index("/* ---- diagnostics") < a < b < c
    assert set(re.findall(r"\b(srt_[a-z_]+)\s*\(", strip(h[a:b]))) == set(CLASSIFY)
    assert set(re.findall(r"\b(srt_[a-z_]+)\s*\(", strip(h[b:c]))) == set(SHADE)


def test_the_header_sections_promise_abi_7_and_state_the_rules(srt):
    h = _header()
    assert C.CDLL(srt.lib_path()).srt_abi_version() == 7 == srt.capi.ABI_VERSION and re.search(r"#define SRT_ABI_VERSION 7\b", h)
    sec = re.search(re.escape(HEAD_CLASSIFY) + r".*?\*/", h, re.S).group(0)
    assert "(ABI 7, backward compatible)" in sec and "SRT_ABI_VERSION stays 7" in sec
    assert all(("\n * S%d. " % k) in sec for k in range(1, 10))
    for words in ("S = sd < S ? sd : S", "D = sqrtf((e.x*e.x + e.y*e.y) + e.z*e.z)", "sd = D - fabsf(radius)", "q_a = fabsf(x_a - c_a) - h_a", "m_a = q_a > 0 ? q_a : 0",
                  "sqrtf((m.x*m.x + m.y*m.y) + m.z*m.z) + min0(max(max(q.x, q.y), q.z))", "mesh objects contribute no", "margin = clearance * smin",
                  "reach = sqrtf((sx*sx + sy*sy) + sz*sz)", "dt = max_offset / (float)steps", "s0 > 1.0625f * reach", "t = (float)m * dt",
                  "o_a = (d_k.a * t) * spacing_a", "x_a = g_a + o_a", "S(x) >= margin", "the lowest", "BURIED|INSIDE", "No atomics reach an output",
                  "One vector atomic per wave", "srt_bind_light_probes", "steps outside 1 .. 64"):
        assert words in sec, words
    sec = re.search(re.escape(HEAD_SHADE) + r".*?\*/", h, re.S).group(0)
    assert "(ABI 7, backward compatible)" in sec and "3s." in sec and "4s." in sec
    for words in ("rec = states[k]", "SRT_PROBE_BURIED is skipped before rule 5", "enters no counter", "p_a = (origin_a + (float)(i_a + c_a) * spacing_a) + rec.o_a",
                  "SRT_PROBE_GRID_VISIBILITY is SRT_ERR_INVALID_ARG", "nx*ny*nz", "Finite offsets are pinned"):
        assert words in sec, words
    block = h[h.index(HEAD_CLASSIFY):h.index(NEXT)]
    assert dict(re.findall(r"#define (\w+) +(\d+)u\b", block)) == DEFINES and len(re.findall(r"#define ", block)) == len(DEFINES)


def test_struct_sizes_layouts_and_constants(srt):
    c = srt.capi
    P, W = c.ProbeClassifyParams, c.ProbeClassifyWork
    assert srt.ProbeClassifyParams is P and srt.ProbeClassifyWork is W
    assert (C.sizeof(P), C.sizeof(W)) == (24, 64)
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("clearance", 0), ("max_offset", 4), ("steps", 8), ("flags", 12), ("outputs", 16), ("reserved", 20)]
    assert [(n, getattr(W, n).offset) for n, _ in W._fields_] == [("valid", 0), ("reserved", 4), ("probes", 8), ("inside", 16), ("moved", 24), ("buried", 32),
                                                                  ("idle", 40), ("candidates", 48), ("waves", 56)]
    for name, mirror in (("srt_probe_classify_params", P), ("srt_probe_classify_work", W)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), re.S)
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        names = [x.strip() for decl in re.findall(r"(?:u?int(?:32|64)_t|float) ([\w, ]+);", body) for x in decl.split(",")]
        assert names == [n for n, _ in mirror._fields_], name
    assert (c.PROBE_STATE_RECORDS, c.PROBE_STATE_POSITIONS) == (PS.RECORDS, PS.POSITIONS) == (1, 2)
    assert (c.PROBE_CLASSIFY_RELOCATE, c.PROBE_CLASSIFY_NORMALIZE, c.PROBE_CLASSIFY_COUNT_WORK) == (PS.RELOCATE, PS.NORMALIZE, PS.COUNT_WORK) == (1, 2, 4)
    assert (c.PROBE_CLEAR, c.PROBE_MOVED, c.PROBE_BURIED, c.PROBE_INSIDE, c.PROBE_IDLE) == (PS.CLEAR, PS.MOVED, PS.BURIED, PS.INSIDE, PS.IDLE) == (0, 1, 2, 4, 8)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_layout_in_c(tmp_path):
    src = tmp_path / "layout.c"
    fields = (["sizeof(srt_probe_classify_params)"] + ["offsetof(srt_probe_classify_params, %s)" % f for f in ("clearance", "max_offset", "steps", "flags", "outputs", "reserved")] +
              ["sizeof(srt_probe_classify_work)"] + ["offsetof(srt_probe_classify_work, %s)" % f for f in ("valid", "reserved", "probes", "inside", "moved", "buried", "idle",
                                                                                                               "candidates", "waves")])
    consts = sorted(DEFINES)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "srt_pathtrace.h"\nint main(void) { printf("%s%s\\n", %s, %s); return 0; }\n' %
                   ("%zu " * len(fields), "%u " * len(consts), ", ".join(fields), ", ".join(consts)))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert got == ["24", "0", "4", "8", "12", "16", "20", "64", "0", "4", "8", "16", "24", "32", "40", "48", "56"] + [DEFINES[k] for k in consts]


def test_defaults_and_refusals_without_a_gpu(srt):
    import numpy as np

    L = srt.load_library()
    c = srt.capi
    bad = c.ERR_INVALID_ARG
    p = c.ProbeClassifyParams(9.0, 9.0, 99, 0xFFFFFFFF, 0xFFFFFFFF, 7)
    assert L.srt_probe_classify_params_default(C.byref(p)) == c.OK
    assert (np.float32(p.clearance), np.float32(p.max_offset), p.steps, p.flags, p.outputs, p.reserved) == (np.float32(0.2), np.float32(0.45), 8, 0, c.PROBE_STATE_RECORDS, 0)
    assert L.srt_probe_classify_params_default(None) == bad
    w, g, d = c.ProbeClassifyWork(), c.ProbeGridParams(), c.ProbeGridDepthParams()
    buf = np.zeros((4, 4), np.float32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    assert L.srt_classify_probes(None, C.byref(p)) == bad and L.srt_bind_probe_states_output(None, 1, None) == bad
    assert L.srt_read_probe_states_output(None, 1, fp) == bad and L.srt_get_probe_classify_work(None, C.byref(w)) == bad
    assert L.srt_write_probe_grid_states(None, fp, 4) == bad and L.srt_bind_probe_grid_states(None, None, 0) == bad
    assert L.srt_shade_probe_grid_states(None, C.byref(g), C.byref(d)) == bad and L.srt_shade_probe_grid_states(None, C.byref(g), None) == bad


def test_python_layers_have_the_new_entries(srt):
    for n in ("classify_probes", "bind_probe_states_output", "probe_states_output", "probe_states_work", "bind_probe_grid_states", "shade_probe_grid_states"):
        assert callable(getattr(srt.PathTracer, n)), n
    for n in ("classify_probes", "probe_states_work", "shade_probe_grid_states"):
        assert callable(getattr(srt.host.Renderer, n)), n
    L = C.CDLL(os.path.join(os.path.dirname(srt.lib_path()), "libsrt_host.so"))
    for n in ("srt_host_renderer_classify_probes", "srt_host_renderer_read_probe_states_output", "srt_host_renderer_probe_classify_work",
              "srt_host_renderer_shade_probe_grid_states"):
        assert srt.host.EXPORTS.count(n) == 1 and hasattr(L, n), n


def test_the_cli_refuses_probe_classify_options_it_cannot_run(tmp_path):
    cli = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
    scene = os.path.join(ROOT, "software-raytracer_amd", "scenes", "Scene1.json")
    out = tmp_path / "out.bin"
    base = [cli, "--scene", scene, "--probe-grid", "-4,0,0,2,2,2,5,3,6", "--probe-directions", "64", "--irradiance-out", str(out)]
    for extra in (["--probe-classify", "--probe-visibility"], ["--probe-relocate"], ["--probe-steps", "4"], ["--states-out", str(tmp_path / "s.bin")],
                  ["--probe-classify", "--probe-clearance", "0"], ["--probe-classify", "--probe-clearance", "0.6"], ["--probe-classify", "--probe-clearance", "nan"],
                  ["--probe-classify", "--probe-max-offset", "0.51"], ["--probe-classify", "--probe-max-offset", "-1"], ["--probe-classify", "--probe-steps", "0"],
                  ["--probe-classify", "--probe-steps", "65"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--probe-classify" in r.stderr and not out.exists(), (extra, r.returncode, r.stderr)
    r = subprocess.run([cli, "--scene", scene, "--probe-classify"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--probe-grid" in r.stderr
