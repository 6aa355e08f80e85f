"""The refit of the mesh image, run as a host loop over the functions the refit kernels share with the BVH build
(tests/native/refit_check.cpp), as a stand-alone program under ASan + UBSan: an identity refit reproduces the build's bytes,
a moved one keeps every child box around what lies below it and every triangle record equal to a fresh build's, the
host-derived root box is the min / max of the world vertices, and the closed-form exponent is the build's old loop.
CPU build only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"),
                                reason="needs g++ and the HIP headers")


def test_host_refit_matches_the_build(tmp_path):
    exe = str(tmp_path / "refit_check")
    subprocess.run(["g++"] + SAN + ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "software-raytracer_amd", "csrc"),
                                    "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "native", "refit_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-600:] + r.stderr[-2000:]
