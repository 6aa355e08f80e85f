#!/usr/bin/env python3
"""What the mirror history does to the temporal result on mirror pixels, on an MI355X — one JSON line per scene and camera path.

The mirror-box scene (tests/mirror_history_reference.py's), Scene3 and Scene1_reflection (--scenes) at --width x --height (default
480 x 270), --bounces (default 8), --spp (default 1) samples per frame over --frames (default 16) frames of a camera that starts
at the default camera and either moves along its right axis by --step-move per frame ("translation") or turns about world up by
--step-turn degrees per frame ("rotation").  Each scene runs in a child process of its own under its own time limit (--limit
seconds); the first failure ends the run.  The reference is a --reference (default 4096) sample srt_render from the last camera.
The error is the relative luminance RMSE of the last frame, sqrt(mean(((L - Lref) / (Lref + 0.01))^2)) with L = 0.2126 r +
0.7152 g + 0.0722 b, over two sets: the mirror pixels (BOUNCES >= 1 and terminal OBJECT != -1) and all other hit pixels, for

    none         no temporal pass: the last frame's samples alone
    off          srt_temporal_accumulate with its defaults, the mirror history off
    on_r1 .. 8   the mirror history on with radius_pixels 1, 2, 4, 8

and, per `on` case, the share of the mirror pixels of the last frame that reuse history (L > n), split by the candidate that was
blended: the motion output equals the virtual point's projection (candidate 1) or it does not (candidate 2).

    python tools/mirror_history_quality.py --out profiles/mirror_history/mirror_history_quality.jsonl

The lines go to stdout, or are appended to --out FILE.  GPU box only."""
import argparse
import importlib
import json
import math
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SCENES = ["mirror_box", "Scene3", "Scene1_reflection"]
RADII = [1.0, 2.0, 4.0, 8.0]


def path_camera(srt, mh, base, kind, k, a):
    """Frame k's camera: the default camera moved along its right axis, or turned about world up."""
    pos = [float(v) for v in base.position[:]]
    basis = [[float(v) for v in axis[:]] for axis in (base.right, base.up, base.forward)]
    if kind == "translation":
        pos = [p + k * a.step_move * r for p, r in zip(pos, basis[0])]
    else:
        t = math.radians(k * a.step_turn)
        c, s = math.cos(t), math.sin(t)
        basis = [[c * v[0] + s * v[2], v[1], -s * v[0] + c * v[2]] for v in basis]
    cam = mh.camera(srt, pos, basis=basis)
    cam.fov_degrees = base.fov_degrees
    return cam


def step(a):
    import numpy as np
    import torch

    import mirror_history_reference as mh
    from mirror_history_time import scene_file

    srt = importlib.import_module("software-raytracer_amd")
    with tempfile.TemporaryDirectory() as tmp:
        scene = srt.host.Scene(scene_file(a.step, tmp))
        assert scene.error == "", scene.error
        objs, cnt = scene.objects_copy()
    pt = srt.PathTracer(a.width, a.height)
    pt.set_scene(objs, cnt)
    base = srt.default_camera()
    w, h, n = a.width, a.height, a.spp

    def lum(img):
        c = img.astype(np.float64)
        return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]

    lines = []
    for kind in ("translation", "rotation"):
        cams = [path_camera(srt, mh, base, kind, k, a) for k in range(a.frames)]
        pt.mirror_history(False)
        pt.set_camera(cams[-1])
        chunk = 256  # (chunks keep a launch short)
        for first in range(1, a.reference + 1, chunk):
            pt.render(spp=min(chunk, a.reference + 1 - first), bounces=a.bounces, seed=2, first_sample=first, reset=(first == 1))
        ref = lum(pt.accumulator())
        pt.render_reflection_gbuffer()
        pt.render_gbuffer()
        robj, J, first_obj = pt.read_reflection("object"), pt.read_reflection("bounces"), pt.gbuffer("object")
        mirror = (J >= 1) & (robj != -1)
        other = (first_obj != -1) & ~mirror & (J == 0)

        def rmse(img, mask):
            e = (lum(img)[mask] - ref[mask]) / (ref[mask] + 0.01)
            return round(float(np.sqrt(np.mean(e * e))), 5) if mask.any() else None

        out = {"path": kind, "mirror_pixels": int(mirror.sum()), "other_pixels": int(other.sum())}
        for case, radius in [("none", None), ("off", None)] + [("on_r%g" % r, r) for r in RADII]:
            pt.mirror_history(radius is not None, radius_pixels=radius)
            pt.motion_output(radius is not None)
            for k, cam in enumerate(cams):
                pt.set_camera(cam)
                pt.render(spp=n, bounces=a.bounces, seed=100 + k)
                if case != "none":
                    pt.temporal(samples=n, reset=k == 0)
            img = pt.accumulator()
            out["mirror_rmse_" + case], out["other_rmse_" + case] = rmse(img, mirror), rmse(img, other)
            if case != "none" and mirror.any():
                out["mirror_reuse_" + case] = round(float(np.mean(pt.history_length()[mirror] > n)), 4)
            if radius is not None and mirror.any():
                # which candidate: the motion output against candidate 1's projection into the previous camera
                g = {k: pt.gbuffer(k) for k in ("normal_depth", "position")}
                D = pt.read_reflection("normal_depth")[..., 3].astype(np.float64)
                C = np.array(cams[-1].position[:], np.float64)
                with np.errstate(all="ignore"):
                    y = C + (g["position"][..., :3].astype(np.float64) - C) * (D / g["normal_depth"][..., 3].astype(np.float64))[..., None]
                u1, v1, ok1, _ = mh.project(y, cams[-2], w, h)
                ys, xs = np.mgrid[0:h, 0:w]
                mv = pt.motion()
                used = mirror & (pt.history_length() > n)
                with np.errstate(all="ignore"):
                    first_c = used & ok1 & (np.abs(mv[..., 0] - (u1 - xs)) < 1e-2) & (np.abs(mv[..., 1] - (v1 - ys)) < 1e-2)
                out["mirror_reuse_candidate1_" + case] = round(float(first_c.sum()) / float(mirror.sum()), 4)
                out["mirror_reuse_candidate2_" + case] = round(float((used & ~first_c).sum()) / float(mirror.sum()), 4)
        lines.append(out)
    pt.mirror_history(False)
    pt.close()
    return {"device": torch.cuda.get_device_name(0), "paths": lines}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--spp", type=int, default=1)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reference", type=int, default=4096)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--step-move", type=float, default=0.03)
    ap.add_argument("--step-turn", type=float, default=0.3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a scene may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one scene in this process and print its JSON")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step(a)))
        return 0
    for name in a.scenes.split(","):  # each in a fresh process, under its own limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + [
            x for k in ("width", "height", "spp", "frames", "reference", "bounces", "step_move", "step_turn") for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            sys.stderr.write("mirror_history_quality: scene %s ran into its limit of %d s; stopping\n" % (name, a.limit))
            return 1
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            sys.stderr.write("mirror_history_quality: scene %s failed (exit %d); stopping\n%s\n" % (name, r.returncode, r.stderr[-2000:]))
            return 1
        got = json.loads(res[-1][len("RESULT "):])
        for per_path in got["paths"]:
            line = {"tool": "mirror_history_quality", "scene": name, "width": a.width, "height": a.height, "spp": a.spp, "frames": a.frames,
                    "reference_spp": a.reference, "bounces": a.bounces, "step_move": a.step_move, "step_turn_degrees": a.step_turn, "device": got["device"]}
            line.update(per_path)
            text = json.dumps(line) + "\n"
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(text)
            sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
