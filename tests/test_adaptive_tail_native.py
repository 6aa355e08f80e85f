"""The host-side rules of srt_render_adaptive_tail (software-raytracer_amd/csrc/srt_adaptive_tail_host.h: rule R1's order of checks,
rule R2, the two-buffer overlap test, what the call leaves in the adaptive and the probe-tail state), run by
tests/native/adaptive_tail_check.cpp as a stand-alone program under ASan + UBSan.  CPU build only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_host_rules_of_the_adaptive_tail(tmp_path):
    exe = str(tmp_path / "adaptive_tail_check")
    subprocess.run(["g++"] + SAN + ["-I" + os.path.join(ROOT, "software-raytracer_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                                    os.path.join(HERE, "native", "adaptive_tail_check.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-600:] + r.stderr[-2000:]
