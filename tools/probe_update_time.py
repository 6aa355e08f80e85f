#!/usr/bin/env python3
"""Time of the per-frame probe updates on an MI355X: the listed traces next to their unlisted parents measured in the same run, the
list (srt_list_probes) and the blend (srt_blend_probes) — JSON lines.

Scene_indirect at --width x --height (default 1920 x 1080), tools/probe_grid_time.py's grids over the frame's hit points, per spacing
(--spacings, default 1, 0.5, 0.25: 210, 1287 and 8925 probes), a relocating classification, --directions (256) directions,
--samples (16) samples of 8 bounces, depth maps of --resolution (16).  Every time is the median of --launches event-bracketed launches
after --warmup, the calls of a group alternating launch by launch (tools/rays_time.py: timed).  Per spacing:

    light     srt_trace_light_probes, the same call again (the parents' own run-to-run spread), srt_trace_light_probes_listed with every
              probe listed, and with the real list (skip BURIED | IDLE)
    depth     the same four for srt_trace_probe_depth
    list      srt_list_probes
    blend     srt_blend_probes without and with the moments, all probes; the achieved share of the HBM floor of 3 x 16 bytes per
              float4 moved (--hbm-gbs, default 8000)

    python tools/probe_update_time.py --out profiles/probe_update/probe_update_time.jsonl

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
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spacings", default="1,0.5,0.25")
    ap.add_argument("--directions", type=int, default=256)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--resolution", type=int, default=16)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
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
    base = {"tool": "probe_update_time", "device": torch.cuda.get_device_name(0), "scene": a.scene, "launches": a.launches, "warmup": a.warmup,
            "directions": a.directions, "samples": a.samples, "bounces": a.bounces, "resolution": a.resolution}
    d = srt.light_probe_sphere(a.directions)
    Rz = a.resolution
    lines = []
    for spacing in [float(s) for s in a.spacings.split(",")]:
        grid = bounds_grid(obj, posb, spacing)
        P = grid.probes
        rec_t = torch.zeros((P, 4), dtype=torch.float32, device=dev)
        pos_t = torch.zeros((P, 4), dtype=torch.float32, device=dev)
        real_t = torch.zeros((4 + P,), dtype=torch.int32, device=dev)
        all_t = torch.zeros((4 + P,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        pt.bind_probe_states_output("records", rec_t)
        pt.bind_probe_states_output("positions", pos_t)
        pt.classify_probes(directions=d, relocate=True, count_work=True, positions=True)
        states = pt.probe_states_work()
        pt.bind_probe_grid_states(rec_t)
        pt.list_probes(skip_mask=0, output=all_t)
        pt.list_probes(output=real_t, count_work=True)
        listed = pt.probe_list_work()["listed"]
        md = 1.5 * float(np.sqrt(3.0) * spacing)
        lkw = dict(samples=a.samples, bounces=a.bounces, seed=1)
        dkw = dict(resolution=Rz, sharpness=5, max_distance=md)
        pt.trace_light_probes(pos_t, d, **lkw)
        pt.trace_probe_depth(**dkw)

        def listed_call(words, fn, **kw):
            def call():
                pt.L.srt_bind_probe_list(pt._h, words.data_ptr(), 4 + P)
                fn(listed=True, **kw)
            return call

        line = dict(base, grid_spacing=spacing, grid_counts=list(grid.counts), probes=P, listed=int(listed), listed_share=round(listed / P, 4), states=states)
        for part, fn, kw in (("light", pt.trace_light_probes, lkw), ("depth", pt.trace_probe_depth, dkw)):
            calls = {"parent": lambda fn=fn, kw=kw: fn(**kw), "parent_again": lambda fn=fn, kw=kw: fn(**kw), "listed_all": listed_call(all_t, fn, **kw),
                     "listed": listed_call(real_t, fn, **kw)}
            t = R.timed(torch, stream, a.launches, a.warmup, calls)
            t["listed_all_to_parent"] = round(t["listed_all"]["median_ms"] / t["parent"]["median_ms"], 3)
            t["parent_again_to_parent"] = round(t["parent_again"]["median_ms"] / t["parent"]["median_ms"], 3)
            t["listed_to_parent"] = round(t["listed"]["median_ms"] / t["parent"]["median_ms"], 3)
            line[part] = t
        line["list"] = R.timed(torch, stream, a.launches, a.warmup, {"list": lambda: pt.list_probes()})["list"]
        # the blend: all probes, histories filled by a first blend so that nothing restarts
        pt.trace_light_probes(**lkw)
        pt.trace_probe_depth(**dkw)
        pt.reset_probe_history(P, Rz)
        pt.blend_probes(moments=True)
        t = R.timed(torch, stream, a.launches, a.warmup, {"coefficients": lambda: pt.blend_probes(), "with_moments": lambda: pt.blend_probes(moments=True)})
        pt.blend_probes(moments=True, count_work=True)
        t["work"] = pt.probe_blend_work()
        for case, elems in (("coefficients", P * 9), ("with_moments", P * (9 + Rz * Rz))):
            floor_ms = elems * 48 / (a.hbm_gbs * 1e9) * 1e3
            t[case]["float4_moved"] = elems
            t[case]["hbm_floor_ms"] = round(floor_ms, 5)
            t[case]["share_of_floor"] = round(floor_ms / t[case]["median_ms"], 4) if t[case]["median_ms"] > 0 else None
        line["blend"] = t
        lines.append(line)
        pt.wait()
        pt.bind_probe_states_output("records", None)
        pt.bind_probe_states_output("positions", None)
        pt.bind_probe_list_output(None)
        pt.bind_probe_list(None)
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
