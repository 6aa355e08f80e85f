"""The host-side rules of the light probes (software-raytracer_amd/csrc/srt_light_probes_host.h: validation order, the K and P*K
limits, the RESET-needs-RADIANCE rule, the record of the last trace, the partial-buffer size, the grid, the Fibonacci set and the
irradiance sum), run by tests/native/light_probe_check.cpp as a stand-alone program under ASan + UBSan.  CPU build only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_host_rules_of_the_light_probes(tmp_path):
    exe = str(tmp_path / "light_probe_check")
    subprocess.run(["g++"] + SAN + ["-I" + os.path.join(ROOT, "software-raytracer_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                                    os.path.join(HERE, "native", "light_probe_check.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-600:] + r.stderr[-2000:]
