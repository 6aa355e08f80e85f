#!/usr/bin/env python3
"""What sun sampling buys a PICTURE in error (SRT_ADAPTIVE_SUN_SAMPLING in srt_render_adaptive and srt_render_adaptive_tail) — JSON
lines, one run.

Reference: srt_render at --reference (4096) samples and 8 bounces, which has no flag.  Error: the relative luminance RMSE
|L - ref| / (ref + 0.01) of the accumulator over the hit pixels.  Every frame is a uniform budget from n = 0.

adaptive (per scene of --scenes, default Scene1,Scene2): srt_render_adaptive at --samples (16) samples and 8 bounces, flag off and
flag on, with the median time of 5 event-timed launches (SRT_ADAPTIVE_KEEP_COUNTS on counts of 0: every launch runs the same
samples); then the flag OFF at the sample count that takes the flagged time (samples * t_on / t_off, at least 1) with its own
measured time: the equal-time comparison.

tail (--tail-scene, default Scene1): srt_render_adaptive_tail at 1 bounce and --tail-samples (64) with DEPTH | STATES, flag off and
flag on, and the same equal-time row.  Grid, depth maps and records are tools/probe_tail_frame_quality.py's (spacing --spacing,
0.5); the coefficients come from probes traced at 8 bounces WITH SRT_LIGHT_PROBE_SUN_SAMPLING (256 directions, 16 samples).

    python tools/adaptive_sun_quality.py --out profiles/adaptive_sun/adaptive_sun_quality.jsonl

The lines go to stdout, or are appended to --out FILE.  GPU box only."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import probe_tail_frame_quality as PTF  # noqa: E402
import probe_tail_quality as Q  # noqa: E402

TAIL_FLAGS = {"depth": True, "states": True}


def _uniform(pt, w, h, samples):
    pt.set_sample_counts(0)
    pt.write_sample_budget(np.full((h, w), samples, np.uint32))


def frame_setup(srt, name, w, h, reference, bounces=8):
    """(tracer, rmse(samples, sun), info): the error over the hit pixels of one uniform srt_render_adaptive frame from n = 0."""
    objs, cnt = Q.load(srt, name)
    pt = srt.PathTracer(w, h)
    pt.set_scene(objs, cnt)
    pt.set_camera(srt.default_camera())
    for first in range(1, reference + 1, 256):
        pt.render(spp=min(256, reference + 1 - first), bounces=bounces, seed=2, first_sample=first, reset=(first == 1))
    ref = Q.lum(pt.accumulator()).reshape(-1)
    pt.render_gbuffer()
    mask = pt.gbuffer("object").reshape(-1) != -1

    def render(samples, sun, seed=11, keep_counts=False):
        pt.render_adaptive(bounces=bounces, seed=seed, sun_sampling=sun, keep_counts=keep_counts)

    def rmse(samples, sun, seed=11):
        _uniform(pt, w, h, samples)
        render(samples, sun, seed)
        e = (Q.lum(pt.accumulator()).reshape(-1) - ref)[mask] / (ref[mask] + 0.01)
        return float(np.sqrt(np.mean(e * e)))

    pt._frame_render = render
    return pt, rmse, dict(pixels=int(mask.sum()))


def tail_setup(srt, name, w, h, reference, spacing, bounces=1):
    """(tracer, rmse(samples, sun), info): the error over the hit pixels of one uniform srt_render_adaptive_tail frame at `bounces`
    under DEPTH | STATES, the coefficients from probes traced at 8 bounces with the flag."""
    pt, _, info = PTF.frame_setup(srt, name, w, h, reference, spacing)
    ref = Q.lum(pt.accumulator()).reshape(-1)  # (the reference render still stands in the accumulator)
    mask = pt.gbuffer("object").reshape(-1) != -1
    # the grid as the set-up made it (the same guides and spacing), then the flagged probe trace
    from probe_grid_time import bounds_grid

    grid = bounds_grid(pt.gbuffer("object"), pt.gbuffer("position"), spacing)
    assert grid.probes == info["probes"]
    pt.probe_tail(enabled=False)
    pt.trace_light_probes(srt.probe_grid_positions(grid.origin, grid.spacing, grid.counts), 256, samples=16, bounces=8, seed=3, sun_sampling=True)
    Q.write_inputs(pt, grid, pt.light_probe_coefficients(), None, None)
    pt.probe_tail(enabled=True, **TAIL_FLAGS)

    def render(samples, sun, seed=11, keep_counts=False):
        pt.render_adaptive_tail(bounces=bounces, seed=seed, sun_sampling=sun, keep_counts=keep_counts)

    def rmse(samples, sun, seed=11):
        _uniform(pt, w, h, samples)
        render(samples, sun, seed)
        e = (Q.lum(pt.accumulator()).reshape(-1) - ref)[mask] / (ref[mask] + 0.01)
        return float(np.sqrt(np.mean(e * e)))

    pt._frame_render = render
    return pt, rmse, dict(probes=grid.probes, pixels=int(mask.sum()))


def measure(part, setup, a, name, samples, **extra):
    import rays_time as RT
    import torch

    pt, rmse, info = setup()
    stream = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    pt.set_stream(stream.cuda_stream)
    out = dict(tool="adaptive_sun_quality", part=part, scene=name, width=a.width, height=a.height, samples=samples, reference=a.reference, runs="one run",
               **extra, **info)

    def ms(n, sun):
        _uniform(pt, a.width, a.height, n)
        return RT.timed(torch, stream, 5, 2, {"x": lambda: pt._frame_render(n, sun, keep_counts=True)})["x"]["median_ms"]

    for k, sun in (("off", False), ("on", True)):
        out[k] = {"rmse": round(rmse(samples, sun), 4), "ms": ms(samples, sun)}
    n = max(1, int(round(samples * out["on"]["ms"] / out["off"]["ms"])))
    out["off_equal_time"] = {"samples": n, "rmse": round(rmse(n, False), 4), "ms": ms(n, False)}
    out["ratio_off_over_on"] = round(out["off"]["rmse"] / out["on"]["rmse"], 3)
    out["ratio_off_equal_time_over_on"] = round(out["off_equal_time"]["rmse"] / out["on"]["rmse"], 3)
    pt.wait()
    pt.set_stream(0)
    pt.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="Scene1,Scene2")
    ap.add_argument("--tail-scene", default="Scene1")
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--tail-samples", type=int, default=64)
    ap.add_argument("--spacing", type=float, default=0.5)
    ap.add_argument("--reference", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    srt = importlib.import_module("software-raytracer_amd")
    lines = []
    for name in [n for n in a.scenes.split(",") if n]:
        lines.append(measure("adaptive", lambda: frame_setup(srt, name, a.width, a.height, a.reference), a, name, a.samples, bounces=8))
    if a.tail_scene:
        lines.append(measure("tail", lambda: tail_setup(srt, a.tail_scene, a.width, a.height, a.reference, a.spacing), a, a.tail_scene, a.tail_samples,
                             bounces=1, spacing=a.spacing, tail_flags="DEPTH | STATES"))
    text = "".join(json.dumps(line) + "\n" for line in lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
