#!/usr/bin/env python3
"""Time of srt_temporal_accumulate with the mirror history off and on, on an MI355X — one JSON line per scene.

Scene1, Scene3 and the mirror-box scene (--scenes; "mirror_box" is tests/mirror_history_reference.py's: a mirror box with two
diffuse spheres behind the camera) at --width x --height (default 1920 x 1080), the default camera, a 1-spp accumulator.  Each
scene runs in a child process of its own under its own time limit (--limit seconds); the first failure ends the run.  Per scene:

    off / on    --launches calls of srt_temporal_accumulate after --warmup, the two modes alternating on ONE context, each call
                bracketed by two events on the tracer's stream; median / min / max.  Switching the mode drops the history, so
                every timed call follows an untimed call in the same mode that stores the history it then reads (a still
                camera: every pixel finds its taps, the steady state of a slowly moving one)
    pixels      mirror pixels (BOUNCES >= 1 and the chain ends on an object), reflected sky, all hit pixels; the share of the
                mirror pixels whose history length grew in the timed call

The mode off launches the kernel it always launched: its column is the plain pass's time (0.046 ms).  Scene1 has
no mirror in view: its `on` column shows what the tag test and the extra loads cost on nothing.  The guide renders (first hits,
reflection outputs) are outside the brackets.

    python tools/mirror_history_time.py --out profiles/mirror_history/mirror_history_time.jsonl

The lines go to stdout, or are appended to --out FILE.  GPU box only."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCENES = ["Scene1", "Scene3", "mirror_box"]


def scene_file(name, tmp):
    if name == "mirror_box":
        import mirror_history_reference as mh

        return mh.mirror_box_scene(os.path.join(tmp, "mirror_box.json"))
    return os.path.join(ROOT, "software-raytracer_amd", "scenes", name + ".json")


def step(a):
    import numpy as np
    import torch

    srt = importlib.import_module("software-raytracer_amd")
    with tempfile.TemporaryDirectory() as tmp:
        scene = srt.host.Scene(scene_file(a.step, tmp))
        assert scene.error == "", scene.error
        objs, cnt = scene.objects_copy()
    pt = srt.PathTracer(a.width, a.height)
    pt.set_scene(objs, cnt)
    pt.set_camera(srt.default_camera())
    pt.render(spp=1, bounces=4, seed=1)
    pt.render_gbuffer(outputs=srt.capi.TEMPORAL_GUIDES)
    pt.render_reflection_gbuffer(outputs=srt.capi.MIRROR_HISTORY_GUIDES)
    robj, J, first = pt.read_reflection("object"), pt.read_reflection("bounces"), pt.gbuffer("object")
    mirror = (J >= 1) & (robj >= 0)
    stream = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    pt.set_stream(stream.cuda_stream)
    ms = {False: [], True: []}
    reuse = None
    for i in range(a.warmup + a.launches):
        for on in (False, True):
            pt.mirror_history(on)
            pt.temporal(samples=1, gbuffer=False)  # stores the history of this mode
            b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b.record(stream)
            pt.temporal(samples=1, gbuffer=False)
            e.record(stream)
            if i >= a.warmup:
                ms[on].append((b, e))
    stream.synchronize()
    reuse = float(np.mean(pt.history_length()[mirror] > 1)) if mirror.any() else None  # (the last call ran with the mode on)
    pt.set_stream(0)
    pt.close()
    out = {"device": torch.cuda.get_device_name(0), "objects": int(cnt), "mirror_pixels": int(mirror.sum()),
           "sky_pixels": int(((J >= 1) & (robj < 0)).sum()), "hit_pixels": int((first >= 0).sum()),
           "mirror_reuse_share": None if reuse is None else round(reuse, 4)}
    for on, name in ((False, "off"), (True, "on")):
        t = [b.elapsed_time(e) for b, e in ms[on]]
        out.update({name + "_median_ms": round(statistics.median(t), 4), name + "_min_ms": round(min(t), 4), name + "_max_ms": round(max(t), 4)})
    out["on_to_off"] = round(out["on_median_ms"] / out["off_median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds a scene may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one scene in this process and print its JSON")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step(a)))
        return 0
    for name in a.scenes.split(","):  # each in a fresh process, under its own limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + [x for k in ("width", "height", "launches", "warmup") for x in ("--" + k, str(getattr(a, k)))]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            sys.stderr.write("mirror_history_time: scene %s ran into its limit of %d s; stopping\n" % (name, a.limit))
            return 1
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            sys.stderr.write("mirror_history_time: scene %s failed (exit %d); stopping\n%s\n" % (name, r.returncode, r.stderr[-2000:]))
            return 1
        line = {"tool": "mirror_history_time", "scene": name, "width": a.width, "height": a.height, "launches": a.launches, "warmup": a.warmup}
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
