"""The host-side rules of sun sampling (software-raytracer_amd/csrc/srt_sun_sampling_host.h: the flag's acceptance, the order of
the errors, rule S5's frame and its two refusals with their edges, bit 8 still refused alone and with 16), run by
tests/native/sun_sampling_check.cpp as a stand-alone program under ASan + UBSan.  CPU build only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_host_rules_of_sun_sampling(tmp_path):
    exe = str(tmp_path / "sun_sampling_check")
    subprocess.run(["g++"] + SAN + ["-I" + os.path.join(ROOT, "software-raytracer_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                                    os.path.join(HERE, "native", "sun_sampling_check.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-600:] + r.stderr[-2000:]
