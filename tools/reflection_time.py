#!/usr/bin/env python3
"""Time of srt_render_reflection_gbuffer on an MI355X next to srt_render_gbuffer on the same context — one JSON line per scene.

Scene1, Scene1_reflection and Scene3 (--scenes) at --width x --height (default 1920 x 1080), the default camera, all five
outputs, the library's defaults (8 reflections, mirrors only).  Each scene runs in a child process of its own under its own
time limit (--limit seconds); the first failure ends the run.  Per scene:

    gbuffer / reflection   --launches launches of srt_render_gbuffer(ALL) and of srt_render_reflection_gbuffer after --warmup, the
                           two alternating, each bracketed by two events on the tracer's stream; median / min / max
    work                   one counting launch: pixels, reflections, wave_calls, waves, and the mean number of occupied lanes
                           per wave-level closest-hit call, (pixels + reflections) / (64 * wave_calls)

Scene1 has no mirror in view: it shows what the lane pool costs when it has nothing to pack.

    python tools/reflection_time.py --out profiles/reflection/reflection_time.jsonl

The lines go to stdout, or are appended to --out FILE.  GPU box only."""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SCENES = ["Scene1", "Scene1_reflection", "Scene3"]


def step(a):
    import torch

    import rays_time as R

    srt = importlib.import_module("software-raytracer_amd")
    scene = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", a.step + ".json"))
    assert scene.error == "", scene.error
    objs, cnt = scene.objects_copy()
    pt = srt.PathTracer(a.width, a.height)
    pt.set_scene(objs, cnt)
    pt.set_camera(srt.default_camera())
    stream = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    pt.set_stream(stream.cuda_stream)
    t = R.timed(torch, stream, a.launches, a.warmup, {"gbuffer": lambda: pt.render_gbuffer(), "reflection": lambda: pt.render_reflection_gbuffer()})
    pt.render_reflection_gbuffer(count_work=True)
    work = pt.reflection_work()
    pt.wait()
    pt.set_stream(0)
    pt.close()
    out = {"device": torch.cuda.get_device_name(0), "objects": int(cnt)}
    for k in ("gbuffer", "reflection"):
        out.update({"%s_median_ms" % k: t[k]["median_ms"], "%s_min_ms" % k: t[k]["min_ms"], "%s_max_ms" % k: t[k]["max_ms"]})
    out["reflection_to_gbuffer"] = round(t["reflection"]["median_ms"] / t["gbuffer"]["median_ms"], 3)
    out.update({k: work[k] for k in ("pixels", "reflections", "wave_calls", "waves")})
    out["occupied_lanes_per_call"] = round((work["pixels"] + work["reflections"]) / float(work["wave_calls"]), 2)
    out["occupancy"] = round((work["pixels"] + work["reflections"]) / (64.0 * work["wave_calls"]), 4)
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
            sys.stderr.write("reflection_time: scene %s ran into its limit of %d s; stopping\n" % (name, a.limit))
            return 1
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            sys.stderr.write("reflection_time: scene %s failed (exit %d); stopping\n%s\n" % (name, r.returncode, r.stderr[-2000:]))
            return 1
        line = {"tool": "reflection_time", "scene": name, "width": a.width, "height": a.height, "launches": a.launches, "warmup": a.warmup}
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
