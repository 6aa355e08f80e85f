"""Moving objects and motion vectors (srt_update_scene, srt_motion_output, srt_bind_motion, srt_read_motion; ABI 7 additions):
the C-ABI declares and exports them, the ctypes mirror matches the header, nothing that existed changed its number, its size or
its bits, and the host library exports its delegates.  No compute: runs without a GPU."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

NEW = ["srt_update_scene", "srt_motion_output", "srt_bind_motion", "srt_read_motion"]


def _header():
    return open(os.path.join(ROOT, "include", "srt_pathtrace.h")).read()


def test_header_declares_and_library_exports_the_motion_entries(srt):
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


def test_nothing_that_existed_changed(srt):
    # backward-compatible additions: the ABI number, the temporal parameters and the temporal flag bits stay
    assert C.CDLL(srt.lib_path()).srt_abi_version() == 7 == srt.capi.ABI_VERSION
    assert re.search(r"#define SRT_ABI_VERSION 7\b", _header())
    assert C.sizeof(srt.capi.TemporalParams) == 20
    bits = dict(re.findall(r"#define (SRT_TEMPORAL_\w+) (\d+)u", _header()))
    assert bits == {"SRT_TEMPORAL_RESET": "1", "SRT_TEMPORAL_FRAMEBUFFER": "2"}
    assert (srt.capi.TEMPORAL_RESET, srt.capi.TEMPORAL_FRAMEBUFFER) == (1, 2)
    assert not [n for n in dir(srt.capi) if n.startswith("TEMPORAL_") and n not in
                ("TEMPORAL_RESET", "TEMPORAL_FRAMEBUFFER", "TEMPORAL_GUIDES", "TEMPORAL_DEFAULTS")]
    assert C.sizeof(srt.capi.Object) == 80  # the motion table compares whole objects: no padding to compare by accident


def test_null_arguments_are_invalid_arg_without_a_gpu(srt):
    L = srt.load_library()
    objs = (srt.capi.Object * 2)()
    assert L.srt_update_scene(None, objs, 2) == srt.capi.ERR_INVALID_ARG
    assert L.srt_update_scene(None, None, 0) == srt.capi.ERR_INVALID_ARG
    assert L.srt_motion_output(None, 1) == srt.capi.ERR_INVALID_ARG
    assert L.srt_bind_motion(None, None) == srt.capi.ERR_INVALID_ARG
    buf = (C.c_float * 4)()
    assert L.srt_read_motion(None, buf) == srt.capi.ERR_INVALID_ARG


def test_python_layers_have_the_new_methods(srt):
    for n in ("update_scene", "motion_output", "bind_motion", "motion"):
        assert callable(getattr(srt.PathTracer, n)), n
    for n in ("update_scene", "motion_output", "motion"):
        assert callable(getattr(srt.host.Renderer, n)), n
    assert callable(srt.host.Scene.set_position)


def test_host_library_exports_the_motion_delegates(srt):
    L = C.CDLL(os.path.join(os.path.dirname(srt.lib_path()), "libsrt_host.so"))
    for n in ("srt_host_renderer_update_scene", "srt_host_renderer_motion_output", "srt_host_renderer_read_motion",
              "srt_host_scene_set_position"):
        assert n in srt.host.EXPORTS
        assert hasattr(L, n), n
