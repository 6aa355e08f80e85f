#!/usr/bin/env python3
"""What the probe tail buys a PICTURE in error — JSON lines, one run.

tools/probe_tail_quality.py's frame protocol (its frame_setup is reused: the scene, the 4096-sample B = 8 srt_render reference,
the grid over the frame's hit points at --spacing (0.5) with coefficients from probes traced at 8 bounces, classified, R = 16 depth
maps) with the frame made by the per-pixel renders instead of srt_trace_radiance on camera rays: a uniform budget from n = 0 through
srt_render_adaptive (no tail) or srt_render_adaptive_tail.  Error: the relative luminance RMSE |L - ref| / (ref + 0.01) of the
accumulator over the DIFFUSE hit pixels.  Per size of --sizes (default 480x270,96x54), in Scene_indirect, each at --samples (64):

    B8, B1                          srt_render_adaptive at 8 bounces and at 1
    B1_tail, B1_tail_depth_states   srt_render_adaptive_tail at 1 bounce, flags none and DEPTH | STATES
    B8_equal_time                   srt_render_adaptive at 8 bounces at the sample count that takes the measured time of
                                    B1_tail_depth_states (samples * t_tail / t_B8, at least 1), and its own measured time

with the median time of 5 event-timed launches (SRT_ADAPTIVE_KEEP_COUNTS on counts of 0: every launch runs the same samples).

    python tools/probe_tail_frame_quality.py --out profiles/probe_tail_frame/probe_tail_frame_quality.jsonl

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

import probe_tail_quality as Q  # noqa: E402


def frame_setup(srt, name, w, h, reference, spacing):
    """probe_tail_quality.frame_setup, with the error of a FRAME: (tracer, rmse(samples, bounces, tail, seed), info).  `tail`: None
    renders with srt_render_adaptive, a dict of probe_tail() flags with srt_render_adaptive_tail; both from n = 0."""
    pt, _, info = Q.frame_setup(srt, name, w, h, reference, spacing)
    pt.bind_rays(None, None)
    # the reference render still stands in the accumulator: the set-up traced probes, guides and rays, none of which write it
    ref = Q.lum(pt.accumulator()).reshape(-1)
    objs, cnt = Q.load(srt, name)
    diffuse = np.array([objs[i].material.specular_amount == 0.0 for i in range(cnt)])
    obj = pt.gbuffer("object").reshape(-1)
    mask = (obj != -1) & diffuse[np.maximum(obj, 0)]
    diffuse_pixels = int(mask.sum())
    if not mask.any():
        mask = obj != -1
    assert int(mask.sum()) == info["pixels"]

    def render(bounces, tail, seed=11, keep_counts=False):
        if tail is None:
            pt.probe_tail(enabled=False)
            pt.render_adaptive(bounces=bounces, seed=seed, keep_counts=keep_counts)
        else:
            pt.probe_tail(enabled=True, **tail)
            pt.render_adaptive_tail(bounces=bounces, seed=seed, keep_counts=keep_counts)

    def rmse(samples, bounces, tail, seed=11):
        pt.set_sample_counts(0)
        pt.write_sample_budget(np.full((h, w), samples, np.uint32))
        render(bounces, tail, seed)
        e = (Q.lum(pt.accumulator()).reshape(-1) - ref)[mask] / (ref[mask] + 0.01)
        return float(np.sqrt(np.mean(e * e)))

    pt._frame_render = render
    return pt, rmse, dict(info, diffuse_pixels=diffuse_pixels)


def frame(srt, a, name, w, h):
    import rays_time as RT
    import torch

    pt, rmse, info = frame_setup(srt, name, w, h, a.reference, a.spacing)
    stream = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    pt.set_stream(stream.cuda_stream)
    rows = {"B8": (8, None), "B1": (1, None), "B1_tail": (1, {}), "B1_tail_depth_states": (1, {"depth": True, "states": True})}
    out = dict(tool="probe_tail_frame_quality", scene=name, width=w, height=h, samples=a.samples, spacing=a.spacing, reference=a.reference, runs="one run", **info)

    def ms(samples, bounces, tail):
        pt.set_sample_counts(0)
        pt.write_sample_budget(np.full((h, w), samples, np.uint32))
        return RT.timed(torch, stream, 5, 2, {"x": lambda: pt._frame_render(bounces, tail, keep_counts=True)})["x"]["median_ms"]

    for k, (b, tail) in rows.items():
        out[k] = {"rmse": round(rmse(a.samples, b, tail), 4), "ms": ms(a.samples, b, tail)}
    n8 = max(1, int(round(a.samples * out["B1_tail_depth_states"]["ms"] / out["B8"]["ms"])))
    out["B8_equal_time"] = {"samples": n8, "rmse": round(rmse(n8, 8, None), 4), "ms": ms(n8, 8, None)}
    for k in ("B1_tail", "B1_tail_depth_states"):
        out["ratio_B1_over_" + k] = round(out["B1"]["rmse"] / out[k]["rmse"], 3)
    out["ratio_B8_equal_time_over_B1_tail_depth_states"] = round(out["B8_equal_time"]["rmse"] / out["B1_tail_depth_states"]["rmse"], 3)
    pt.wait()
    pt.set_stream(0)
    pt.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="Scene_indirect")
    ap.add_argument("--sizes", default="480x270,96x54")
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--spacing", type=float, default=0.5)
    ap.add_argument("--reference", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    srt = importlib.import_module("software-raytracer_amd")
    lines = [frame(srt, a, a.scene, *[int(v) for v in size.split("x")]) for size in a.sizes.split(",") if size]
    text = "".join(json.dumps(line) + "\n" for line in lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
