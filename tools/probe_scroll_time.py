#!/usr/bin/env python3
"""Time of srt_scroll_probes on an MI355X next to what there was before it — JSON lines.

Scene_indirect at --width x --height (default 1920 x 1080), tools/probe_grid_time.py's grids over the frame's hit points, per spacing
(--spacings, default 1, 0.5, 0.25: 210, 1287 and 8925 probes), the handle's own histories, moments at --resolution (16).  Every time
is the median of --launches (20) event-bracketed calls after --warmup, the calls of a group alternating call by call
(tools/rays_time.py: timed).  ONE run: no spread between runs has been measured.  Per spacing:

    scroll         srt_scroll_probes by --shift (1, 0, 0) with COEFFICIENTS, and with COEFFICIENTS | MOMENTS; next to each time the
                   bytes the call moves (a retained float4 is read and written, an exposed one written) and the time those bytes take
                   at the HBM peak (--hbm-gbs, default 8000), and the share of that floor the call reaches
    reset_retrace  the route without it: srt_reset_probe_history and a full unlisted srt_trace_light_probes of --samples (16)
                   samples, --directions (64) directions and --bounces (8) bounces; with the moments also srt_trace_probe_depth

    python tools/probe_scroll_time.py --out profiles/probe_scroll/probe_scroll_time.jsonl

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
import probe_scroll_reference as SC  # noqa: E402
import rays_time as R  # noqa: E402  (timed)
from probe_depth_time import open_tracer  # noqa: E402
from probe_grid_time import bounds_grid  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="Scene_indirect")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spacings", default="1,0.5,0.25")
    ap.add_argument("--shift", default="1,0,0")
    ap.add_argument("--directions", type=int, default=64)
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
    pt, _ = open_tracer(srt, a.scene, a.width, a.height)
    stream = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    pt.set_stream(stream.cuda_stream)
    pt.render_gbuffer(outputs=["object", "normal_depth", "position"])
    obj, posb = pt.gbuffer("object"), pt.gbuffer("position")
    shift = tuple(int(v) for v in a.shift.split(","))
    d = srt.light_probe_sphere(a.directions)
    Rz = a.resolution
    base = {"tool": "probe_scroll_time", "device": torch.cuda.get_device_name(0), "scene": a.scene, "launches": a.launches, "warmup": a.warmup, "runs": 1,
            "shift": list(shift), "directions": a.directions, "samples": a.samples, "bounces": a.bounces, "resolution": Rz, "hbm_gbs": a.hbm_gbs}
    lines = []
    for spacing in [float(s) for s in a.spacings.split(",")]:
        grid = bounds_grid(obj, posb, spacing)
        P = grid.probes
        pos = srt.probe_grid_positions(grid.origin, grid.spacing, grid.counts)
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        pt.reset_probe_history(P, Rz)
        lkw = dict(samples=a.samples, bounces=a.bounces, seed=1)
        dkw = dict(resolution=Rz, sharpness=5, max_distance=1.5 * float(np.sqrt(3.0) * spacing))
        pt.trace_light_probes(pos, d, **lkw)
        pt.trace_probe_depth(**dkw)
        work = SC.work(grid.counts, shift)

        def retrace(moments):
            def call():
                pt.reset_probe_history(P, Rz if moments else 0)
                pt.trace_light_probes(**lkw)
                if moments:
                    pt.trace_probe_depth(**dkw)
            return call

        line = dict(base, grid_spacing=spacing, grid_counts=[int(v) for v in grid.counts], probes=int(P), retained=work["retained"], exposed=work["exposed"])
        t = R.timed(torch, stream, a.launches, a.warmup, {"coefficients": lambda: pt.scroll_probes(shift, which="coefficients"),
                                                           "with_moments": lambda: pt.scroll_probes(shift, which="both")})
        alt = R.timed(torch, stream, a.launches, a.warmup, {"coefficients": retrace(False), "with_moments": retrace(True)})
        for case, elems in (("coefficients", 9), ("with_moments", 9 + Rz * Rz)):
            moved = 16 * elems * (2 * work["retained"] + work["exposed"])
            floor_ms = moved / (a.hbm_gbs * 1e9) * 1e3
            t[case]["bytes_moved"] = moved
            t[case]["hbm_floor_ms"] = round(floor_ms, 6)
            t[case]["share_of_floor"] = round(floor_ms / t[case]["median_ms"], 4) if t[case]["median_ms"] > 0 else None
            t[case]["reset_retrace_ms"] = alt[case]["median_ms"]
            t[case]["reset_retrace_to_scroll"] = round(alt[case]["median_ms"] / t[case]["median_ms"], 1) if t[case]["median_ms"] > 0 else None
        line["scroll"] = t
        line["reset_retrace"] = alt
        pt.scroll_probes(shift, which="both", count_work=True)
        line["work"] = pt.probe_scroll_work()
        lines.append(line)
        pt.wait()
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
