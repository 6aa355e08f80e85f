#!/usr/bin/env python3
"""How close probe-grid shading comes to the path tracer's diffuse indirect light, and what the visibility test buys, on an MI355X
— one JSON line per scene and grid spacing.

Scene_indirect and the closed room (Scene_indirect with a wall behind the camera, as tests/test_gpu_visibility.py closes it) at
--width x --height (default 480 x 270), the default camera.  Per spacing (--spacings, default 2, 1, 0.5) the grid covers the
bounding box of the frame's hit points, clipped to [-16, 16] x [-2, 10] x [0, 32]; its probes are traced with
srt_trace_light_probes (--directions spherical Fibonacci directions, --samples samples of --bounces bounces) and stay on the
device.  The preview is srt_shade_probe_grid with the hemisphere band weights (1, 0.5, 0) and SRT_PROBE_GRID_ALBEDO, plus the
emissive colour of the pixel's object added on the host by OBJECT id.  The reference is a --reference (default 4096) sample
srt_render of the same camera and bounces.  The error is the relative luminance RMSE sqrt(mean(((L - Lref) / (Lref + 0.01))^2)),
L = 0.2126 r + 0.7152 g + 0.0722 b, over the hit pixels whose material has SpecularAmount == 0, for the flags

    none, normal_weight, visibility, both

with, per case, the share of those pixels that end with a = 0 (no usable probe); they count with L = emissive alone.

    python tools/probe_grid_quality.py --out profiles/probe_grid/probe_grid_quality.jsonl

The lines go to stdout, or are appended to --out FILE.  GPU box only."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import probe_grid_reference as PG  # noqa: E402
from probe_grid_time import CASES, bounds_grid  # noqa: E402


def lum(img):
    c = img.astype(np.float64)
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="Scene_indirect,closed_room")
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--spacings", default="2,1,0.5")
    ap.add_argument("--directions", type=int, default=256)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--reference", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    srt = importlib.import_module("software-raytracer_amd")
    w, h = a.width, a.height
    lines = []
    for name in a.scenes.split(","):
        scene = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", "Scene_indirect.json"))
        assert scene.error == "", scene.error
        if name == "closed_room":
            wall = srt.Object()
            wall.type, wall.position[:], wall.half_size[:] = 2, (0.0, 0.0, -0.3), (6.0, 6.0, 0.2)
            wall.material.base_color[:] = (0.5, 0.5, 0.5)
            scene.add(wall, "wall behind the camera")
        objs, cnt = scene.objects_copy()
        diffuse = np.array([objs[i].material.specular_amount == 0.0 for i in range(cnt)])
        emissive = np.array([list(objs[i].material.emissive_color) for i in range(cnt)], np.float64)
        pt = srt.PathTracer(w, h)
        pt.set_scene(objs, cnt)
        pt.set_camera(srt.default_camera())
        for first in range(1, a.reference + 1, 256):  # (chunks keep a launch short)
            pt.render(spp=min(256, a.reference + 1 - first), bounces=a.bounces, seed=2, first_sample=first, reset=(first == 1))
        ref = lum(pt.accumulator())
        pt.render_gbuffer()
        obj, pos = pt.gbuffer("object"), pt.gbuffer("position")
        mask = (obj != -1) & diffuse[np.maximum(obj, 0)]
        glow = lum(emissive[np.maximum(obj, 0)])
        for spacing in [float(s) for s in a.spacings.split(",")]:
            grid = bounds_grid(obj, pos, spacing)
            positions = srt.probe_grid_positions(grid.origin, grid.spacing, grid.counts)
            t = torch.zeros((grid.probes * 9, 4), dtype=torch.float32, device="cuda:0")
            pt.bind_light_probe_output("coefficients", t)
            pt.trace_light_probes(positions, a.directions, samples=a.samples, bounces=a.bounces, seed=3)
            pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
            line = {"tool": "probe_grid_quality", "device": torch.cuda.get_device_name(0), "scene": name, "width": w, "height": h, "spacing": spacing,
                    "grid_counts": list(grid.counts), "probes": grid.probes, "directions": a.directions, "probe_samples": a.samples, "bounces": a.bounces,
                    "reference_spp": a.reference, "diffuse_pixels": int(mask.sum()), "band_weight": [1.0, 0.5, 0.0]}
            for case, flags in CASES:
                pt.shade_probe_grid(coefficients=t, visibility=bool(flags & PG.VISIBILITY), normal_weight=bool(flags & PG.NORMAL_WEIGHT), albedo=True,
                                    band_weight=PG.HEMISPHERE)
                out = pt.probe_grid_output()
                e = (lum(out)[mask] + glow[mask] - ref[mask]) / (ref[mask] + 0.01)
                line[case] = {"rmse": round(float(np.sqrt(np.mean(e * e))), 4), "mean_relative_error": round(float(np.mean(e)), 4),
                              "no_probe_share": round(float(np.mean(out[..., 3][mask] == 0)), 4)}
            pt.wait()
            pt.bind_light_probe_output("coefficients", None)
            pt.L.srt_bind_probe_grid_coefficients(pt._h, None, 0)
            lines.append(line)
        pt.close()
    text = "".join(json.dumps(line) + "\n" for line in lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
