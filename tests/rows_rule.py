"""What the launch-shape rule answers for a request, for the GPU tests that must know which pathtrace_kernel instantiation a launch
reaches: the library does not report it (no ABI change), so the tests ask the rule itself — tests/native/rows_rule_check.cpp --ask
runs plan_launch_shape, finish_launch_shape, fold_from_rows and rows_six_waves of csrc/srt_launch_shape.h, and
tests/native/six_wave_rule_check.cpp --grow builds a scene's image with the library's own build_scene_image and prints the LDS bytes
of a rows workgroup.  Both are stand-alone host programs under ASan + UBSan, built once per test session."""
import collections
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "software-raytracer_amd", "csrc")
HOST = os.path.join(ROOT, "software-raytracer_amd", "host")
SANITIZE = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
_EXES = {}

Answer = collections.namedtuple("Answer", "tile_h chunks wg8 rows six rows_bytes")


def rows_rule_exe(tmp_path_factory):
    if "rows" not in _EXES:
        exe = str(tmp_path_factory.mktemp("rows_rule") / "rows_rule_check")
        subprocess.run(SANITIZE + ["-I" + CSRC, os.path.join(ROOT, "tests", "native", "rows_rule_check.cpp"), "-o", exe], check=True, capture_output=True)
        _EXES["rows"] = exe
    return _EXES["rows"]


def six_wave_rule_exe(tmp_path_factory):
    if "six" not in _EXES:
        exe = str(tmp_path_factory.mktemp("six_wave_rule") / "six_wave_rule_check")
        subprocess.run(SANITIZE + ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC, "-I" + HOST, "-I" + os.path.join(ROOT, "include"),
                                   os.path.join(ROOT, "tests", "native", "six_wave_rule_check.cpp"), os.path.join(HOST, "scene.cpp"), "-o", exe],
                       check=True, capture_output=True)
        _EXES["six"] = exe
    return _EXES["six"]


def ask(exe, requests):
    """requests: dicts of w, rows, spp, cu_count and optionally mesh, preview, steps, block_grid, scene_in_lds, lds_bytes ->
    one Answer per request"""
    lines = []
    for q in requests:
        lines.append("%d %d %d %d %d %d %d %d %d %d\n" % (q["w"], q["rows"], q["spp"], q["cu_count"], bool(q.get("mesh")), bool(q.get("preview")),
                                                         q.get("steps", 1), bool(q.get("block_grid")), bool(q.get("scene_in_lds", True)),
                                                         q.get("lds_bytes", 0)))
    r = subprocess.run([exe, "--ask"], input="".join(lines), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-2000:]
    out = [Answer(*(int(v) for v in line.split())) for line in r.stdout.splitlines()]
    assert len(out) == len(lines), r.stdout[-400:]
    return out


def grow(exe, scene_json, spheres):
    """[(k, LDS bytes of a rows workgroup, six waves?)] for the scene plus the first k of `spheres` (x, y, z, radius), k = 0 .. len"""
    text = "".join("%r %r %r %r\n" % tuple(float(v) for v in s) for s in spheres)
    r = subprocess.run([exe, "--grow", scene_json], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-2000:]
    out = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert [k for k, _, _ in out] == list(range(len(spheres) + 1)), r.stdout[-400:]
    return out
