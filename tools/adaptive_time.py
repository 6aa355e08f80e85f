#!/usr/bin/env python3
"""Time of srt_render_adaptive on an MI355X next to srt_render and srt_trace_radiance doing the same work — one JSON line.

Scene1 at --width x --height (default 1920 x 1080), the default camera and environment, --bounces (default 8) bounces, seed 0.
Four steps, each in a child process of its own under its own time limit (--limit seconds); the first failure ends the run and
nothing is written:

    render     srt_render of the frame at --samples (default 32) samples: srt_stats.kernel_ms of --launches launches after
               --warmup; median / min / max
    radiance   the frame's camera rays as a batch, srt_trace_radiance at --samples samples (tools/radiance_time.py's step)
    uniform    (a) srt_render_adaptive with a uniform budget of --samples from n = 0 (SRT_ADAPTIVE_KEEP_COUNTS, so every launch
               does the same work): --launches launches after --warmup, each bracketed by two events on the tracer's stream
               (the ticket's memset included); then one counting launch, and how many accumulator elements equal srt_render's
    map        (b) the map srt_sample_budget (the library's defaults) makes after a seed of --seed-samples (default 8) samples
               in each of two halves: the time of srt_render_adaptive on half A with that map (KEEP_COUNTS: the same frames
               every launch), the sum of e_p, path-samples per second, and srt_render's kernel time for the same total spread
               uniformly (rounded up to whole samples per pixel, continuing the half)

    python tools/adaptive_time.py --out profiles/adaptive/adaptive_time.jsonl

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

import radiance_time as RT  # noqa: E402


def on_stream(a):
    import torch

    srt, R, pt = RT.tracer(a)
    stream = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    pt.set_stream(stream.cuda_stream)
    return torch, srt, R, pt, stream


def render_ms(pt, a, **kw):
    ms = []
    for i in range(a.warmup + a.launches):
        pt.render(bounces=a.bounces, **kw)
        pt.wait()
        if i >= a.warmup:
            ms.append(float(pt.stats().kernel_ms))
    return ms


def step_uniform(a):
    import numpy as np

    torch, srt, R, pt, stream = on_stream(a)
    pt.set_sample_counts(0)
    pt.write_sample_budget(np.full((a.height, a.width), a.samples, np.uint32))
    t = R.timed(torch, stream, a.launches, a.warmup, {"x": lambda: pt.render_adaptive(bounces=a.bounces, seed=0, keep_counts=True)})["x"]
    pt.render_adaptive(bounces=a.bounces, seed=0, keep_counts=True, count_work=True)
    acc, work = pt.accumulator(), pt.adaptive_work()
    pt.render(spp=a.samples, bounces=a.bounces, seed=0)
    equal = int((acc.view(np.uint32) == pt.accumulator().view(np.uint32)).all(axis=2).sum())
    pt.wait()
    pt.set_stream(0)
    pt.close()
    return {"uniform_median_ms": t["median_ms"], "uniform_min_ms": t["min_ms"], "uniform_max_ms": t["max_ms"], "uniform_wave_calls": work["wave_calls"],
            "uniform_closest_calls": work["closest_calls"], "uniform_elements_equal_to_render": equal}


def step_map(a):
    import numpy as np

    torch, srt, R, pt, stream = on_stream(a)
    n, seed_b = a.seed_samples, 0x9E3779B9
    pt.render(spp=n, bounces=a.bounces, seed=0)
    pt.bind_output(None, pt.half_ptr())
    pt.render(spp=n, bounces=a.bounces, seed=seed_b)
    pt.bind_output()
    pt.set_sample_counts(n)
    pt.variance(merge=False)
    pt.sample_budget()
    total = pt.budget_total()
    budget = pt.sample_budget_map()
    t = R.timed(torch, stream, a.launches, a.warmup, {"x": lambda: pt.render_adaptive(bounces=a.bounces, seed=0, keep_counts=True)})["x"]
    pt.render_adaptive(bounces=a.bounces, seed=0, keep_counts=True, count_work=True)
    work = pt.adaptive_work()
    assert work["samples"] == total, (work, total)
    px = a.width * a.height
    spread = -(-total // px)
    ms = render_ms(pt, a, spp=spread, seed=0, first_sample=n + 1, reset=False) if spread else [0.0]
    pt.set_stream(0)
    pt.close()
    return {"seed_samples_per_half": n, "map_median_ms": t["median_ms"], "map_min_ms": t["min_ms"], "map_max_ms": t["max_ms"], "map_samples": total,
            "map_pixels": work["pixels"], "map_pixels_at_max": int((budget == budget.max()).sum()) if total else 0, "map_wave_calls": work["wave_calls"],
            "map_closest_calls": work["closest_calls"], "map_path_samples_per_s": round(total / (t["median_ms"] * 1e-3), 1) if t["median_ms"] else 0.0,
            "spread_samples_per_pixel": spread, "spread_render_kernel_median_ms": round(statistics.median(ms), 4),
            "spread_render_kernel_min_ms": round(min(ms), 4), "spread_render_kernel_max_ms": round(max(ms), 4)}


STEPS = {"render": RT.step_render, "radiance": RT.step_radiance, "uniform": step_uniform, "map": step_map}
ARGS = ("width", "height", "samples", "bounces", "launches", "warmup", "seed_samples")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--seed-samples", dest="seed_samples", type=int, default=8)
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
    line = {"tool": "adaptive_time", "scene": "Scene1", "width": a.width, "height": a.height, "samples": a.samples, "bounces": a.bounces,
            "launches": a.launches, "warmup": a.warmup}
    for step in ("render", "radiance", "uniform", "map"):  # each in a fresh process, under its own limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + [x for k in ARGS for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            sys.stderr.write("adaptive_time: step %s ran into its limit of %d s; stopping\n" % (step, a.limit))
            return 1
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            sys.stderr.write("adaptive_time: step %s failed (exit %d); stopping\n%s\n" % (step, r.returncode, r.stderr[-2000:]))
            return 1
        line.update(json.loads(res[-1][len("RESULT "):]))
    line["uniform_to_render"] = round(line["uniform_median_ms"] / line["render_kernel_median_ms"], 3)
    line["uniform_to_radiance"] = round(line["uniform_median_ms"] / line["radiance_median_ms"], 3)
    if line["spread_render_kernel_median_ms"]:
        line["map_to_spread_render"] = round(line["map_median_ms"] / line["spread_render_kernel_median_ms"], 3)
    text = json.dumps(line) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
