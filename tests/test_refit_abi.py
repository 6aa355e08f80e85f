"""Refitting the mesh BVH (srt_update_mode, srt_get_update_info, srt_mesh_image_size, srt_read_mesh_image and the srt_update_info
struct; ABI 7 additions): the C-ABI declares and exports them, the ctypes mirror matches the header, the struct has the size
and offsets the header gives it, nothing that existed changed its number.  No compute: runs without a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

NEW = ["srt_update_mode", "srt_get_update_info", "srt_mesh_image_size", "srt_read_mesh_image"]
FIELDS = [("path", 0, 4), ("reason", 4, 4), ("levels", 8, 4), ("triangles", 12, 4), ("nodes", 16, 4), ("moved_mesh_objects", 20, 4)]


def _header():
    return open(os.path.join(ROOT, "include", "srt_pathtrace.h")).read()


def test_header_declares_and_library_exports_the_refit_entries(srt):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NEW + ["srt_update_scene"]:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), n
        assert n in srt.capi.EXPORTS
    assert re.search(r"typedef\s+struct\s+srt_update_info\s*\{", text)
    syms = subprocess.run(["nm", "-D", srt.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (srt_[a-z_0-9]+)", syms))
    assert set(NEW) | {"srt_update_scene"} <= exported
    declared = set(re.findall(r"\b(srt_[a-z_0-9]+)\s*\(", text)) - {"srt_context"}
    assert declared == set(srt.capi.EXPORTS)
    assert len(srt.capi.EXPORTS) == len(set(srt.capi.EXPORTS))


def test_constants_and_abi_number(srt):
    h = _header()
    assert re.search(r"#define SRT_UPDATE_REBUILD 0\b", h) and re.search(r"#define SRT_UPDATE_REFIT 1\b", h)
    assert (srt.capi.UPDATE_REBUILD, srt.capi.UPDATE_REFIT) == (0, 1)
    assert re.search(r"#define SRT_ABI_VERSION 7\b", h)
    assert C.CDLL(srt.lib_path()).srt_abi_version() == 7 == srt.capi.ABI_VERSION
    assert C.sizeof(srt.capi.Object) == 80 and srt.capi.Object.position.offset == 4  # the path is chosen by comparing the bytes around position


def test_update_info_layout_in_ctypes(srt):
    U = srt.capi.UpdateInfo
    assert C.sizeof(U) == 24
    assert [(n, getattr(U, n).offset, getattr(U, n).size) for n, _ in U._fields_] == FIELDS
    # the order and types the header declares
    body = re.search(r"typedef struct srt_update_info \{(.*?)\} srt_update_info;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = re.findall(r"\b(int32_t|uint32_t)\s+(\w+)\s*;", body)
    assert [n for _, n in decl] == [n for n, _, _ in FIELDS]
    assert [t for t, _ in decl] == ["int32_t"] * 3 + ["uint32_t"] * 3


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs a C compiler")
def test_update_info_layout_in_c(tmp_path):
    """The header compiles as C, and the compiler gives the struct 24 bytes and the offsets the binding assumes."""
    checks = "".join('_Static_assert(offsetof(srt_update_info, %s) == %d, "%s");\n' % (n, off, n) for n, off, _ in FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "srt_pathtrace.h"\n_Static_assert(sizeof(srt_update_info) == 24, "size");\n' + checks +
                   "_Static_assert(SRT_UPDATE_REBUILD == 0 && SRT_UPDATE_REFIT == 1, \"modes\");\nint main(void) { return 0; }\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")],
                   check=True, capture_output=True)


def test_null_arguments_are_invalid_arg_without_a_gpu(srt):
    L = srt.load_library()
    u = srt.capi.UpdateInfo()
    n = C.c_size_t(0)
    assert L.srt_update_mode(None, 1) == srt.capi.ERR_INVALID_ARG
    assert L.srt_get_update_info(None, C.byref(u)) == srt.capi.ERR_INVALID_ARG
    assert L.srt_mesh_image_size(None, C.byref(n), C.byref(n)) == srt.capi.ERR_INVALID_ARG
    assert L.srt_read_mesh_image(None, None, None) == srt.capi.ERR_INVALID_ARG


def test_python_layers_have_the_new_methods(srt):
    for n in ("update_mode", "update_info", "mesh_image"):
        assert callable(getattr(srt.PathTracer, n)), n
    assert srt.capi.UPDATE_PATHS == {0: "none", 1: "rebuilt", 2: "refitted", 3: "kept"}
