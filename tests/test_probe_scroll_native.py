"""The host-side rules of the scrolling probe grid (software-raytracer_amd/csrc/srt_probe_scroll_host.h: the index rule swept over
every shift around three small grids and the int32 extremes, the moved origin, the follow shift, the order of the checks, what a
scroll makes stale), run by tests/native/probe_scroll_check.cpp as a stand-alone program under ASan + UBSan.  CPU build only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SAN = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_host_rules_of_the_scroll(tmp_path):
    exe = str(tmp_path / "probe_scroll_check")
    subprocess.run(["g++"] + SAN + ["-I" + os.path.join(ROOT, "software-raytracer_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                                    os.path.join(HERE, "native", "probe_scroll_check.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-600:] + r.stderr[-2000:]
