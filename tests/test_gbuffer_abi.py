"""First-hit buffers (ABI 7): the C-ABI declares, exports and validates srt_render_gbuffer / srt_bind_gbuffer /
srt_read_gbuffer, and the host library exports its delegates.  No compute: runs without a GPU."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

NEW = ["srt_render_gbuffer", "srt_bind_gbuffer", "srt_read_gbuffer"]


def _header():
    return open(os.path.join(ROOT, "include", "srt_pathtrace.h")).read()


def test_header_declares_and_library_exports_the_gbuffer_entries(srt):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
        assert n in srt.capi.EXPORTS
    syms = subprocess.run(["nm", "-D", srt.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (srt_[a-z_0-9]+)", syms))
    assert set(NEW) <= exported
    assert C.CDLL(srt.lib_path()).srt_abi_version() == 7 == srt.capi.ABI_VERSION
    assert re.search(r"#define SRT_ABI_VERSION 7\b", _header())


def test_gbuffer_params_layout_and_bits_match_the_header(srt):
    G = srt.capi.GBufferParams
    assert C.sizeof(G) == 16
    m = re.search(r"typedef struct srt_gbuffer_params \{(.*?)\} srt_gbuffer_params;", _header(), re.S)
    fields = re.findall(r"u?int32_t (\w+);", m.group(1))
    assert fields == [n for n, _ in G._fields_] == ["row_begin", "row_end", "outputs", "flags"]
    assert [G.row_begin.offset, G.row_end.offset, G.outputs.offset, G.flags.offset] == [0, 4, 8, 12]
    bits = dict(re.findall(r"#define (SRT_GBUF_\w+) (\d+)u", _header()))
    assert bits == {"SRT_GBUF_OBJECT": "1", "SRT_GBUF_NORMAL_DEPTH": "2", "SRT_GBUF_POSITION": "4", "SRT_GBUF_ALBEDO": "8", "SRT_GBUF_ALL": "15"}
    c = srt.capi
    assert (c.GBUF_OBJECT, c.GBUF_NORMAL_DEPTH, c.GBUF_POSITION, c.GBUF_ALBEDO, c.GBUF_ALL) == (1, 2, 4, 8, 15)
    assert {n: v[0] for n, v in c.GBUFFERS.items()} == {"object": 1, "normal_depth": 2, "position": 4, "albedo": 8}
    assert c.gbuffer_outputs(["object", "albedo"]) == 9 and c.gbuffer_outputs("position") == 4 and c.gbuffer_outputs(15) == 15


def test_null_context_or_params_is_invalid_arg_without_a_gpu(srt):
    L = srt.load_library()
    p = srt.capi.GBufferParams(0, 1, 1, 0)
    assert L.srt_render_gbuffer(None, C.byref(p)) == srt.capi.ERR_INVALID_ARG
    assert L.srt_render_gbuffer(None, None) == srt.capi.ERR_INVALID_ARG
    buf = (C.c_int32 * 4)()
    assert L.srt_bind_gbuffer(None, 1, None) == srt.capi.ERR_INVALID_ARG
    assert L.srt_read_gbuffer(None, 1, buf) == srt.capi.ERR_INVALID_ARG


def test_host_library_exports_the_gbuffer_delegates(srt):
    L = C.CDLL(os.path.join(os.path.dirname(srt.lib_path()), "libsrt_host.so"))
    for n in ("srt_host_renderer_render_gbuffer", "srt_host_renderer_read_gbuffer"):
        assert n in srt.host.EXPORTS
        assert hasattr(L, n), n
