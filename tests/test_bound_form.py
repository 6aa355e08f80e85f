"""closest_hit's cluster bound test about the ray's foot point (csrc/srt_kernel.hip.h; form and proof in csrc/srt_scene_image.h)
against the reference's candidate test of every member sphere, on the CPU: tests/native/bound_form_check.cpp builds the scene
images with the library's own build_scene_image, evaluates both tests in binary32 as the kernel and the reference do, and must find
no culled cluster with a candidate inside — the shipped scenes and the random families of test_gpu_fuzz.py, as they are and moved
by 1e3 and 1e5, origins on the floor, inside clusters, far out and in front of spheres behind the ray, grazing, random and
axis-parallel directions of |d|^2 = 1 +- 1e-6, and rays with a NaN or an infinity.  Here with about 1e6 (ray, cluster) pairs, under
ASan + UBSan; run the program itself for its default of 1e8."""
import os
import subprocess

from conftest import ROOT, scene_path

CSRC = os.path.join(ROOT, "software-raytracer_amd", "csrc")
HOST = os.path.join(ROOT, "software-raytracer_amd", "host")


def test_no_culled_cluster_holds_a_candidate(tmp_path):
    exe = str(tmp_path / "bound_form_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC, "-I" + HOST, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "bound_form_check.cpp"), os.path.join(HOST, "scene.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe, "--pairs", "1000000"] + [scene_path(s) for s in ("Scene1", "Scene3", "Scene_indirect")],
                       capture_output=True, text=True)
    print(r.stdout)
    last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0 and last.startswith("ok ") and last.endswith(" 0 violations"), r.stdout[-2000:] + r.stderr[-2000:]
    pairs, culled = int(last.split()[1]), int(last.split()[3])
    assert pairs >= 1000000 and culled > pairs // 10  # (a test that culls nothing would pass the check too)
    assert "first scene, 16 clusters" in r.stdout
