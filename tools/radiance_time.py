#!/usr/bin/env python3
"""Time of srt_trace_radiance on an MI355X next to srt_render doing the same work — one JSON line.

Scene1 at --width x --height (default 1920 x 1080), the default camera and environment, --samples (default 32) samples of
--bounces (default 8) bounces, seed 0.  Two steps, each in a child process of its own under its own time limit (--limit
seconds); the first failure ends the run and nothing is written:

    render     srt_render of the frame: srt_stats.kernel_ms of --launches launches after --warmup (the cost-ordered dispatch
               settles in the warm-up); median / min / max
    radiance   the frame's camera rays (tools/rays_time.py: camera_rays, GetRayDirection's arithmetic in torch) bound as a
               batch of width * height rays, srt_trace_radiance with id_base 0: --launches launches after --warmup, each
               bracketed by two events on the tracer's stream; median / min / max; then one counting launch for wave_calls and
               closest_calls, and how many of its elements equal srt_render's accumulator bit for bit (the directions come from
               torch, so a few pixels may differ in the last bit of a direction)

    python tools/radiance_time.py --out profiles/radiance/radiance_time.jsonl

The line goes to stdout, or is appended to --out FILE.  GPU box only."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def tracer(a):
    import rays_time as R

    srt = importlib.import_module("software-raytracer_amd")
    scene = R.load_scene(srt, None)
    objs, cnt = scene.objects_copy()
    pt = srt.PathTracer(a.width, a.height)
    pt.set_scene(objs, cnt)
    pt.set_camera(srt.default_camera())
    return srt, R, pt


def step_render(a):
    import torch

    srt, R, pt = tracer(a)
    ms = []
    for i in range(a.warmup + a.launches):
        pt.render(spp=a.samples, bounces=a.bounces, seed=0)
        pt.wait()
        if i >= a.warmup:
            ms.append(float(pt.stats().kernel_ms))
    st = pt.stats()
    out = {"device": torch.cuda.get_device_name(0), "render_kernel_median_ms": round(statistics.median(ms), 4), "render_kernel_min_ms": round(min(ms), 4),
           "render_kernel_max_ms": round(max(ms), 4), "render_sample_chunks": int(st.sample_chunks), "render_tile_rows": int(st.tile_rows)}
    pt.close()
    return out


def step_radiance(a):
    import numpy as np
    import torch

    srt, R, pt = tracer(a)
    stream = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    pt.set_stream(stream.cuda_stream)
    o, d = R.camera_rays(torch, a.width, a.height)
    torch.cuda.synchronize()
    pt.bind_rays(o, d)
    t = R.timed(torch, stream, a.launches, a.warmup, {"radiance": lambda: pt.trace_radiance(samples=a.samples, bounces=a.bounces, seed=0)})["radiance"]
    pt.trace_radiance(samples=a.samples, bounces=a.bounces, seed=0, count_work=True)
    rad, work = pt.radiance(), pt.radiance_work()
    pt.render(spp=a.samples, bounces=a.bounces, seed=0)
    acc = pt.accumulator().reshape(-1, 4)
    equal = int((rad.view(np.uint32) == acc.view(np.uint32)).all(axis=1).sum())
    pt.wait()
    pt.set_stream(0)
    pt.close()
    return {"radiance_median_ms": t["median_ms"], "radiance_min_ms": t["min_ms"], "radiance_max_ms": t["max_ms"], "rays": work["rays"],
            "wave_calls": work["wave_calls"], "closest_calls": work["closest_calls"], "elements_equal_to_render": equal}


STEPS = {"render": step_render, "radiance": step_radiance}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds a step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="(internal) run one step in this process and print its JSON")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(STEPS[a.step](a)))
        return 0
    line = {"tool": "radiance_time", "scene": "Scene1", "width": a.width, "height": a.height, "samples": a.samples, "bounces": a.bounces,
            "launches": a.launches, "warmup": a.warmup}
    for step in ("render", "radiance"):  # each in a fresh process, under its own limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + [x for k in ("width", "height", "samples", "bounces", "launches", "warmup")
                                                                            for x in ("--" + k, str(getattr(a, k)))]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            sys.stderr.write("radiance_time: step %s ran into its limit of %d s; stopping\n" % (step, a.limit))
            return 1
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            sys.stderr.write("radiance_time: step %s failed (exit %d); stopping\n%s\n" % (step, r.returncode, r.stderr[-2000:]))
            return 1
        line.update(json.loads(res[-1][len("RESULT "):]))
    line["radiance_to_render"] = round(line["radiance_median_ms"] / line["render_kernel_median_ms"], 3)
    text = json.dumps(line) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
