"""The host-side rules of the probe cascade (software-raytracer_amd/csrc/srt_probe_cascade_host.h: which cascades are accepted and
what a refused one leaves, which "present" marks survive a new cascade, the capture's state checks, the order of the shading call's
errors, the grids helper and rule C2 on a table of points), run by tests/native/probe_cascade_check.cpp as a stand-alone program
under ASan + UBSan.  CPU build only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_host_rules_of_the_probe_cascade(tmp_path):
    exe = str(tmp_path / "probe_cascade_check")
    subprocess.run(["g++"] + SAN + ["-I" + os.path.join(ROOT, "software-raytracer_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                                    os.path.join(HERE, "native", "probe_cascade_check.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-600:] + r.stderr[-2000:]
