#!/usr/bin/env python3
"""Time of probe-grid shading (srt_shade_probe_grid) on an MI355X next to two yardsticks measured in the same run — JSON lines.

Scene1 and Scene_indirect (--scenes) at --width x --height (default 1920 x 1080), the default camera.  The grid has spacing
--spacing (default 1.0) over the bounding box of the frame's hit points, clipped to [-16, 16] x [-2, 10] x [0, 32] (Scene1's
ground reaches the horizon); the coefficients are seeded random floats — the time does not depend on their values.  Per scene:

    shade        srt_shade_probe_grid for flags none, NORMAL_WEIGHT, VISIBILITY and both, from the G-buffer that is already on the
                 device: --launches launches after --warmup, each bracketed by two events on the tracer's stream, the four cases
                 and the yardstick alternating launch by launch; median / min / max, and the work counts of one further counting call
    ao           the yardstick with the same number of any-hit segments per hit pixel: srt_render_visibility with AO only,
                 ao_samples = 8, ao_radius = +inf; its times by the same events and its work counts
    host         what a caller had to do before, without the visibility test: read the three guides back, interpolate and evaluate
                 in numpy (tests/probe_grid_reference.py, in bands of 40 rows), upload the W x H float4; one run on the host clock,
                 and its result compared with the device's bit for bit

    python tools/probe_grid_time.py --out profiles/probe_grid/probe_grid_time.jsonl

The lines go to stdout, or are appended to --out FILE.  GPU box only."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import probe_grid_reference as PG  # noqa: E402  (the rule in numpy binary32)
import rays_time as R  # noqa: E402  (timed)

CLIP = np.array([[-16.0, -2.0, 0.0], [16.0, 10.0, 32.0]])
CASES = [("none", 0), ("normal_weight", PG.NORMAL_WEIGHT), ("visibility", PG.VISIBILITY), ("both", PG.VISIBILITY | PG.NORMAL_WEIGHT)]


def bounds_grid(obj, pos, spacing):
    p = pos[obj != -1][:, :3].astype(np.float64)
    lo = np.floor(np.clip(p.min(axis=0), CLIP[0], CLIP[1]))
    hi = np.ceil(np.clip(p.max(axis=0), CLIP[0], CLIP[1]))
    counts = [int(round((hi[a] - lo[a]) / spacing)) + 1 for a in range(3)]
    return PG.Grid(lo, (spacing,) * 3, counts)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="Scene1,Scene_indirect")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spacing", type=float, default=1.0)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    srt = importlib.import_module("software-raytracer_amd")
    w, h = a.width, a.height
    lines = []
    for name in a.scenes.split(","):
        scene = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", name + ".json"))
        assert scene.error == "", scene.error
        objs, cnt = scene.objects_copy()
        pt = srt.PathTracer(w, h)
        pt.set_scene(objs, cnt)
        pt.set_camera(srt.default_camera())
        stream = torch.cuda.Stream(device=0)
        torch.cuda.synchronize()
        pt.set_stream(stream.cuda_stream)
        pt.render_gbuffer(outputs=["object", "normal_depth", "position"])
        obj, pos = pt.gbuffer("object"), pt.gbuffer("position")
        grid = bounds_grid(obj, pos, a.spacing)
        coeff = np.random.default_rng(7).uniform(0.0, 2.0, (grid.probes, 9, 4)).astype(np.float32)
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        pt.shade_probe_grid(coefficients=coeff)
        calls = {case: (lambda f=flags: pt.shade_probe_grid(visibility=bool(f & PG.VISIBILITY), normal_weight=bool(f & PG.NORMAL_WEIGHT))) for case, flags in CASES}
        calls["ao"] = lambda: pt.render_visibility(8, float("inf"), sun=False)
        t = R.timed(torch, stream, a.launches, a.warmup, calls)
        line = {"tool": "probe_grid_time", "device": torch.cuda.get_device_name(0), "scene": name, "width": w, "height": h, "launches": a.launches,
                "warmup": a.warmup, "hit_pixels": int((obj != -1).sum()), "grid_origin": [float(v) for v in grid.origin], "grid_spacing": a.spacing,
                "grid_counts": list(grid.counts), "probes": grid.probes}
        for case, flags in CASES:
            pt.shade_probe_grid(visibility=bool(flags & PG.VISIBILITY), normal_weight=bool(flags & PG.NORMAL_WEIGHT), count_work=True)
            line[case] = dict(t[case], work=pt.probe_grid_work())
        pt.render_visibility(8, float("inf"), sun=False, count_work=True)
        line["ao"] = dict(t["ao"], work=pt.visibility_work())
        for case in ("visibility", "both"):
            line[case + "_to_ao"] = round(t[case]["median_ms"] / t["ao"]["median_ms"], 3)
        if not a.no_host:
            pt.shade_probe_grid()
            device = pt.probe_grid_output()
            t0 = time.perf_counter()
            g = [pt.gbuffer(k) for k in ("object", "normal_depth", "position")]
            host = np.empty((h, w, 4), np.float32)
            for y in range(0, h, 40):
                host[y:y + 40] = PG.shade(grid, coeff, g[0][y:y + 40], g[1][y:y + 40], g[2][y:y + 40])
            up = torch.from_numpy(host).to("cuda:0")
            torch.cuda.synchronize()
            line["host_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            line["host_equals_device"] = bool(np.array_equal(host.view(np.uint32), device.view(np.uint32)))
            del up
        lines.append(line)
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
