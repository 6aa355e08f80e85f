#!/usr/bin/env python3
"""Time of probe classification (srt_classify_probes) and of the shading that obeys the records (srt_shade_probe_grid_states) on an
MI355X, the shading next to its parent calls measured in the same run — JSON lines.

Scene_indirect at --width x --height (default 1920 x 1080), tools/probe_grid_time.py's grids over the frame's hit points.  Every time
is the median of --launches event-bracketed launches after --warmup, the calls of a part alternating launch by launch
(tools/rays_time.py: timed).

    classify  per spacing (--spacings, default 1, 0.5, 0.25: 210, 1287 and 8925 probes in Scene_indirect) srt_classify_probes with --directions (256)
              directions, without and with SRT_PROBE_CLASSIFY_RELOCATE (the default parameters), RECORDS only, and the work counts of
              one counting call each.
    shade     at --spacing (default 1.0), seeded random coefficients, depth maps of srt_trace_probe_depth and records of a
              relocating srt_classify_probes, all bound device to device: srt_shade_probe_grid and srt_shade_probe_grid_states
              without depth, srt_shade_probe_grid_depth and srt_shade_probe_grid_states with it; the ratios states / parent.

    python tools/probe_states_time.py --out profiles/probe_states/probe_states_time.jsonl

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
import rays_time as R  # noqa: E402  (timed)
from probe_depth_time import open_tracer  # noqa: E402
from probe_grid_time import bounds_grid  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="Scene_indirect")
    ap.add_argument("--parts", default="classify,shade")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spacings", default="1,0.5,0.25")
    ap.add_argument("--spacing", type=float, default=1.0)
    ap.add_argument("--directions", type=int, default=256)
    ap.add_argument("--resolution", type=int, default=16)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    srt = importlib.import_module("software-raytracer_amd")
    w, h = a.width, a.height
    dev = "cuda:0"
    pt, _ = open_tracer(srt, a.scene, w, h)
    stream = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    pt.set_stream(stream.cuda_stream)
    pt.render_gbuffer(outputs=["object", "normal_depth", "position"])
    obj, posb = pt.gbuffer("object"), pt.gbuffer("position")
    base = {"device": torch.cuda.get_device_name(0), "scene": a.scene, "launches": a.launches, "warmup": a.warmup, "directions": a.directions}
    d = srt.light_probe_sphere(a.directions)
    lines = []
    if "classify" in a.parts.split(","):
        for spacing in [float(s) for s in a.spacings.split(",")]:
            grid = bounds_grid(obj, posb, spacing)
            pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
            pt.classify_probes(directions=d, relocate=True)
            calls = {"at_rest": lambda: pt.classify_probes(), "relocate": lambda: pt.classify_probes(relocate=True)}
            t = R.timed(torch, stream, a.launches, a.warmup, calls)
            line = dict(base, tool="probe_states_time", part="classify", grid_spacing=spacing, grid_counts=list(grid.counts), probes=grid.probes)
            for case, fn in (("at_rest", lambda: pt.classify_probes(count_work=True)), ("relocate", lambda: pt.classify_probes(relocate=True, count_work=True))):
                fn()
                line[case] = dict(t[case], work=pt.probe_states_work())
            lines.append(line)
    if "shade" in a.parts.split(","):
        grid = bounds_grid(obj, posb, a.spacing)
        P, Rz = grid.probes, a.resolution
        coeff = np.random.default_rng(7).uniform(0.0, 2.0, (P, 9, 4)).astype(np.float32)
        mom_t = torch.empty((P * Rz * Rz, 4), dtype=torch.float32, device=dev)
        rec_t = torch.zeros((P, 4), dtype=torch.float32, device=dev)
        pos_t = torch.zeros((P, 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        pt.bind_probe_states_output("records", rec_t)
        pt.bind_probe_states_output("positions", pos_t)
        pt.classify_probes(directions=d, relocate=True, count_work=True, positions=True)
        states = pt.probe_states_work()
        pt.bind_probe_depth_output("moments", mom_t)
        pt.trace_probe_depth(pos_t, d, resolution=Rz, sharpness=5, max_distance=1.5 * float(np.sqrt(3.0) * a.spacing))
        pt.shade_probe_grid(coefficients=coeff)
        pt.shade_probe_grid_depth(moments=mom_t, resolution=Rz)
        pt.shade_probe_grid_states(states=rec_t)
        calls = {"none": lambda: pt.shade_probe_grid(), "none_states": lambda: pt.shade_probe_grid_states(), "depth": lambda: pt.shade_probe_grid_depth(),
                 "depth_states": lambda: pt.shade_probe_grid_states(depth=True)}
        t = R.timed(torch, stream, a.launches, a.warmup, calls)
        line = dict(base, tool="probe_states_time", part="shade", width=w, height=h, hit_pixels=int((obj != -1).sum()), grid_spacing=a.spacing,
                    grid_counts=list(grid.counts), probes=P, resolution=Rz, states=states)
        for case, fn in (("none", lambda: pt.shade_probe_grid(count_work=True)), ("none_states", lambda: pt.shade_probe_grid_states(count_work=True)),
                         ("depth", lambda: pt.shade_probe_grid_depth(count_work=True)), ("depth_states", lambda: pt.shade_probe_grid_states(depth=True, count_work=True))):
            fn()
            line[case] = dict(t[case], work=pt.probe_grid_work())
        line["none_states_to_none"] = round(t["none_states"]["median_ms"] / t["none"]["median_ms"], 3)
        line["depth_states_to_depth"] = round(t["depth_states"]["median_ms"] / t["depth"]["median_ms"], 3)
        line["depth_to_none"] = round(t["depth"]["median_ms"] / t["none"]["median_ms"], 3)
        lines.append(line)
        pt.wait()
        pt.bind_probe_depth_output("moments", None)
        pt.bind_probe_states_output("records", None)
        pt.bind_probe_states_output("positions", None)
        pt.bind_probe_grid_depth(None)
        pt.bind_probe_grid_states(None)
        pt.L.srt_bind_light_probes(pt._h, None, 0)
    pt.wait()
    pt.set_stream(0)
    pt.close()
    text = "".join(json.dumps(line) + "\n" for line in lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
