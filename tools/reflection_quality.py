#!/usr/bin/env python3
"""What the reflection guides do to srt_denoise on mirror pixels, on an MI355X — one JSON line per scene.

Scene1_reflection and Scene3 (--scenes) at --width x --height (default 480 x 270), the default camera, --bounces (default 8).
Each scene runs in a child process of its own under its own time limit (--limit seconds); the first failure ends the run.
The input is an --spp (default 8) sample render with seed 1, the reference a --reference (default 4096) sample srt_render with
seed 2.  The error is the relative luminance RMSE, sqrt(mean(((L - Lref) / (Lref + 0.01))^2)) with L = 0.2126 r + 0.7152 g +
0.0722 b, over the pixels whose chain follows at least one reflection and ends on an object (BOUNCES >= 1 and OBJECT != -1),
for three variants:

    noisy        the input as it is
    first_hit    srt_denoise with its defaults, guided by the first-hit buffers
    reflection   srt_denoise with its defaults, guided by the reflection guides (use_reflection_guides)

and, for orientation, the same three over all the other pixels that hit something (first-hit OBJECT != -1).

    python tools/reflection_quality.py --out profiles/reflection/reflection_quality.jsonl

The lines go to stdout, or are appended to --out FILE.  GPU box only."""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = ["Scene1_reflection", "Scene3"]


def step(a):
    import numpy as np
    import torch

    srt = importlib.import_module("software-raytracer_amd")
    scene = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", a.step + ".json"))
    assert scene.error == "", scene.error
    objs, cnt = scene.objects_copy()
    pt = srt.PathTracer(a.width, a.height)
    pt.set_scene(objs, cnt)
    pt.set_camera(srt.default_camera())

    def lum(img):
        c = img.astype(np.float64)
        return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]

    chunk = 256  # (a render call takes at most 2^20 samples; chunks keep a launch short)
    for first in range(1, a.reference + 1, chunk):
        pt.render(spp=min(chunk, a.reference + 1 - first), bounces=a.bounces, seed=2, first_sample=first, reset=(first == 1))
    ref = lum(pt.accumulator())
    pt.render_reflection_gbuffer()
    robj, J = pt.read_reflection("object"), pt.read_reflection("bounces")
    pt.render_gbuffer()
    first_obj = pt.gbuffer("object")
    mirror = (J >= 1) & (robj != -1)
    other = (first_obj != -1) & ~mirror & (J == 0)
    pt.render(spp=a.spp, bounces=a.bounces, seed=1)
    noisy = pt.accumulator()
    variants = {"noisy": noisy}
    for name, on in (("first_hit", False), ("reflection", True)):
        pt.use_reflection_guides(on)
        pt.write_accumulator(noisy)
        pt.denoise()
        variants[name] = pt.denoised()
    pt.use_reflection_guides(False)
    pt.close()

    def rmse(img, mask):
        e = (lum(img)[mask] - ref[mask]) / (ref[mask] + 0.01)
        return round(float(np.sqrt(np.mean(e * e))), 5) if mask.any() else None

    out = {"device": torch.cuda.get_device_name(0), "mirror_pixels": int(mirror.sum()), "other_pixels": int(other.sum())}
    for name, img in variants.items():
        out["mirror_rmse_" + name] = rmse(img, mirror)
        out["other_rmse_" + name] = rmse(img, other)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--reference", type=int, default=4096)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--limit", type=int, default=180, help="seconds a scene may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one scene in this process and print its JSON")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step(a)))
        return 0
    for name in a.scenes.split(","):  # each in a fresh process, under its own limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + [x for k in ("width", "height", "spp", "reference", "bounces") for x in ("--" + k, str(getattr(a, k)))]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            sys.stderr.write("reflection_quality: scene %s ran into its limit of %d s; stopping\n" % (name, a.limit))
            return 1
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            sys.stderr.write("reflection_quality: scene %s failed (exit %d); stopping\n%s\n" % (name, r.returncode, r.stderr[-2000:]))
            return 1
        line = {"tool": "reflection_quality", "scene": name, "width": a.width, "height": a.height, "spp": a.spp, "reference_spp": a.reference, "bounces": a.bounces}
        line.update(json.loads(res[-1][len("RESULT "):]))
        text = json.dumps(line) + "\n"
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(text)
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
