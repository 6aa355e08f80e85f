"""The host-side rules every image and ray pass shares (software-raytracer_amd/csrc/srt_outputs_host.h: the output slot behind
srt_bind_* / srt_read_*, the grid of persistent workgroups), run by tests/native/outputs_check.cpp as a stand-alone program under
ASan + UBSan.  CPU build only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_host_rules_of_the_output_slots(tmp_path):
    exe = str(tmp_path / "outputs_check")
    subprocess.run(["g++"] + SAN + ["-I" + os.path.join(ROOT, "software-raytracer_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                                    os.path.join(HERE, "native", "outputs_check.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-600:] + r.stderr[-2000:]
