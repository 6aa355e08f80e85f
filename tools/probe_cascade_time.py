#!/usr/bin/env python3
"""Time of the probe-cascade shading (srt_shade_probe_cascade) on an MI355X next to the single-grid calls it replaces, measured in
the same run — one JSON line per scene and part.

--scenes (default Scene1, Scene_indirect) at --width x --height (default 1920 x 1080), the default camera.  Every time is the median
of --launches event-bracketed launches after --warmup, the calls of a part alternating launch by launch (tools/rays_time.py: timed).
Coefficients are seeded random numbers; records come from a relocating srt_classify_probes and depth maps from srt_trace_probe_depth
on each grid; every array stays on the device and is bound, not copied.

    one    L = 1 against srt_shade_probe_grid_states on the same grid (tools/probe_grid_time.py's grid over the frame's hit points at
           --spacing), without and with the depth maps: the cost of the scan, the level table and the larger LDS footprint.
    three  L = 3 levels of --counts probes nested around the camera position (srt_probe_cascade_grids, finest spacing --base), with
           records and depth maps, against the SUM of three srt_shade_probe_grid_states calls, one per level's grid — the cheapest
           route there was, before any blend on the host — and the work counts of one counting cascade call.

    python tools/probe_cascade_time.py --out profiles/probe_cascade/probe_cascade_time.jsonl

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
import probe_grid_reference as PG  # noqa: E402
import rays_time as R  # noqa: E402  (timed)
from probe_depth_time import open_tracer  # noqa: E402
from probe_grid_time import bounds_grid  # noqa: E402


def level_arrays(torch, pt, grid, d, Rz, seed, dev):
    """Random coefficients, classified records and traced depth maps of one grid as device tensors."""
    P = grid.probes
    co = torch.from_numpy(np.random.default_rng(seed).uniform(0.0, 2.0, (P * 9, 4)).astype(np.float32)).to(dev)
    mom = torch.empty((P * Rz * Rz, 4), dtype=torch.float32, device=dev)
    rec = torch.zeros((P, 4), dtype=torch.float32, device=dev)
    pos = torch.zeros((P, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
    pt.bind_probe_states_output("records", rec)
    pt.bind_probe_states_output("positions", pos)
    pt.classify_probes(directions=d, relocate=True, positions=True)
    pt.bind_probe_depth_output("moments", mom)
    pt.trace_probe_depth(pos, d, resolution=Rz, sharpness=5, max_distance=1.5 * float(np.sqrt(3.0) * max(grid.spacing)))
    pt.wait()
    pt.bind_probe_depth_output("moments", None)
    pt.bind_probe_states_output("records", None)
    pt.bind_probe_states_output("positions", None)
    return co, mom, rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="Scene1,Scene_indirect")
    ap.add_argument("--parts", default="one,three")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spacing", type=float, default=1.0)
    ap.add_argument("--base", type=float, default=0.5)
    ap.add_argument("--counts", default="9,9,9")
    ap.add_argument("--directions", type=int, default=256)
    ap.add_argument("--resolution", type=int, default=16)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    srt = importlib.import_module("software-raytracer_amd")
    w, h, Rz, dev = a.width, a.height, a.resolution, "cuda:0"
    counts = [int(v) for v in a.counts.split(",")]
    d = srt.light_probe_sphere(a.directions)
    lines = []
    for name in a.scenes.split(","):
        pt, _ = open_tracer(srt, name, w, h)
        stream = torch.cuda.Stream(device=0)
        torch.cuda.synchronize()
        pt.set_stream(stream.cuda_stream)
        pt.render_gbuffer(outputs=["object", "normal_depth", "position"])
        obj, posb = pt.gbuffer("object"), pt.gbuffer("position")
        base = {"tool": "probe_cascade_time", "device": torch.cuda.get_device_name(0), "scene": name, "width": w, "height": h, "hit_pixels": int((obj != -1).sum()),
                "launches": a.launches, "warmup": a.warmup, "runs": 1, "directions": a.directions, "resolution": Rz}

        def single(grid, arrays, depth):
            co, mom, rec = arrays
            pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
            pt.shade_probe_grid_states(coefficients=co, states=rec, moments=mom if depth else None, resolution=Rz, depth=depth)

        if "one" in a.parts.split(","):
            grid = bounds_grid(obj, posb, a.spacing)
            arrays = level_arrays(torch, pt, grid, d, Rz, 7, dev)
            pt.set_probe_cascade([(grid.origin, grid.spacing, grid.counts)], Rz, 1.0)
            for which, t in zip(("coefficients", "moments", "records"), arrays):
                pt.bind_probe_cascade_level(0, which, t, probes=grid.probes)
            single(grid, arrays, True)  # (the single grid's bindings: the timed calls write nothing)
            calls = {"states": lambda: pt.shade_probe_grid_states(), "cascade": lambda: pt.shade_probe_cascade(states=True),
                     "states_depth": lambda: pt.shade_probe_grid_states(depth=True), "cascade_depth": lambda: pt.shade_probe_cascade(states=True, depth=True)}
            t = R.timed(torch, stream, a.launches, a.warmup, calls)
            pt.shade_probe_cascade(states=True, depth=True, count_work=True)
            line = dict(base, part="one", grid_spacing=a.spacing, grid_counts=list(grid.counts), probes=grid.probes, work=pt.probe_cascade_work(), **t)
            line["cascade_to_states"] = round(t["cascade"]["median_ms"] / t["states"]["median_ms"], 3)
            line["cascade_depth_to_states_depth"] = round(t["cascade_depth"]["median_ms"] / t["states_depth"]["median_ms"], 3)
            lines.append(line)
        if "three" in a.parts.split(","):
            cam = srt.default_camera()
            k = srt.probe_cascade_grids([float(v) for v in cam.position], (a.base,) * 3, counts, 3)
            grids = [PG.Grid(k.grid[l].origin[:], k.grid[l].spacing[:], k.grid[l].counts[:]) for l in range(3)]
            arrays = [level_arrays(torch, pt, g, d, Rz, 11 + l, dev) for l, g in enumerate(grids)]
            pt.set_probe_cascade([(g.origin, g.spacing, g.counts) for g in grids], Rz, 1.0)
            for l, g in enumerate(grids):
                for which, t in zip(("coefficients", "moments", "records"), arrays[l]):
                    pt.bind_probe_cascade_level(l, which, t, probes=g.probes)

            def three_single():
                for l, g in enumerate(grids):
                    single(g, arrays[l], True)

            calls = {"three_single_grid_calls": three_single, "cascade": lambda: pt.shade_probe_cascade(states=True, depth=True)}
            t = R.timed(torch, stream, a.launches, a.warmup, calls)
            pt.shade_probe_cascade(states=True, depth=True, count_work=True)
            line = dict(base, part="three", base_spacing=a.base, level_counts=counts, probes_per_level=grids[0].probes, work=pt.probe_cascade_work(), **t)
            line["cascade_to_three_calls"] = round(t["cascade"]["median_ms"] / t["three_single_grid_calls"]["median_ms"], 3)
            lines.append(line)
        pt.wait()
        pt.bind_probe_grid_depth(None)
        pt.bind_probe_grid_states(None)
        pt.L.srt_bind_probe_grid_coefficients(pt._h, None, 0)
        pt.L.srt_bind_light_probes(pt._h, None, 0)
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
