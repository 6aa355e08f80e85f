#!/usr/bin/env python3
"""What a probe cascade buys over the two single grids a following grid has to choose between, on an MI355X — one JSON line per
scene and finest spacing.

Scene_indirect at --width x --height (default 480 x 270), the default camera.  Per finest spacing (--bases, default 0.25, 0.5)
three routes, each with --counts probes per grid (default 5 x 5 x 5) around --centre: "diffuse" (default), the centroid of the hit
points of the diffuse pixels, which are the ones the error is taken over, or "camera", the camera position (in Scene_indirect no
diffuse pixel lies within two units of the camera, so there the finest levels hold none of them).  The grids come from
srt_probe_cascade_grids.  Every grid is classified with relocation (srt_classify_probes, the defaults), traced at the positions that
gives with srt_trace_light_probes (--directions spherical Fibonacci directions, --samples samples of --bounces bounces) and
srt_trace_probe_depth (R = --resolution), and shaded with the records, the depth maps, the normal weight, the hemisphere band weights
(1, 0.5, 0) and albedo — without the records a fine grid leaks through the probes inside objects, README's probe-depth row — plus the
emissive colour of the pixel's object added on the host by OBJECT id:

    fine     srt_shade_probe_grid_states on the finest level's grid alone (spacing base): a point outside it is clamped to its outer layer
    coarse   srt_shade_probe_grid_states on the coarsest level's grid alone (spacing base * 4)
    cascade  srt_shade_probe_cascade on the three levels, blend_cells --blend

The reference is a --reference (default 4096) sample srt_render of the same camera and bounces.  The error is
tools/probe_grid_quality.py's: the relative luminance RMSE sqrt(mean(((L - Lref) / (Lref + 0.01))^2)) over the hit pixels whose
material has SpecularAmount == 0, here also separately for the pixels inside the finest level's box and for those outside it.

    python tools/probe_cascade_quality.py --out profiles/probe_cascade/probe_cascade_quality.jsonl

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
import probe_cascade_reference as PC  # noqa: E402
import probe_grid_reference as PG  # noqa: E402
from probe_grid_quality import lum  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="Scene_indirect")
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--bases", default="0.25,0.5")
    ap.add_argument("--centre", default="diffuse", choices=("diffuse", "camera"))
    ap.add_argument("--counts", default="5,5,5")
    ap.add_argument("--resolution", type=int, default=16)
    ap.add_argument("--blend", type=float, default=1.0)
    ap.add_argument("--directions", type=int, default=256)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--reference", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    srt = importlib.import_module("software-raytracer_amd")
    w, h = a.width, a.height
    counts = [int(v) for v in a.counts.split(",")]
    lines = []
    for name in a.scenes.split(","):
        scene = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", name + ".json"))
        assert scene.error == "", scene.error
        objs, cnt = scene.objects_copy()
        diffuse = np.array([objs[i].material.specular_amount == 0.0 for i in range(cnt)])
        emissive = np.array([list(objs[i].material.emissive_color) for i in range(cnt)], np.float64)
        pt = srt.PathTracer(w, h)
        pt.set_scene(objs, cnt)
        cam = srt.default_camera()
        pt.set_camera(cam)
        for first in range(1, a.reference + 1, 256):  # (chunks keep a launch short)
            pt.render(spp=min(256, a.reference + 1 - first), bounces=a.bounces, seed=2, first_sample=first, reset=(first == 1))
        ref = lum(pt.accumulator())
        pt.render_gbuffer()
        obj, pos = pt.gbuffer("object"), pt.gbuffer("position")
        mask = (obj != -1) & diffuse[np.maximum(obj, 0)]
        glow = lum(emissive[np.maximum(obj, 0)])
        centre = [float(v) for v in cam.position] if a.centre == "camera" else pos[mask][:, :3].astype(np.float64).mean(axis=0).tolist()
        for base in [float(v) for v in a.bases.split(",")]:
            k = srt.probe_cascade_grids(centre, (base,) * 3, counts, 3)
            grids = [PG.Grid(k.grid[l].origin[:], k.grid[l].spacing[:], k.grid[l].counts[:]) for l in range(3)]
            cas = PC.Cascade(grids, a.blend, 0)
            cls = PC.classes(cas, pos[..., :3].reshape(-1, 3)).reshape(h, w)
            inside = mask & (PC.level_weight(grids[0], a.blend, pos[..., :3].reshape(-1, 3)).reshape(h, w) > 0)
            coeff, rec, mom, buried = [], [], [], []
            for l, g in enumerate(grids):
                pt.set_probe_grid(g.origin, g.spacing, g.counts)
                pt.classify_probes(directions=a.directions, relocate=True, positions=True, count_work=True)
                rec.append(pt.probe_states_output("records"))
                buried.append(pt.probe_states_work()["buried"])
                pt.trace_light_probes(pt.probe_states_output("positions"), a.directions, samples=a.samples, bounces=a.bounces, seed=3 + l)
                coeff.append(pt.light_probe_coefficients())
                pt.trace_probe_depth(resolution=a.resolution, sharpness=5, max_distance=1.5 * float(np.sqrt(3.0) * max(g.spacing)))
                mom.append(pt.probe_depth_output("moments"))
            line = {"tool": "probe_cascade_quality", "device": torch.cuda.get_device_name(0), "scene": name, "width": w, "height": h, "runs": 1, "centre": a.centre, "base_spacing": base,
                    "level_counts": counts, "resolution": a.resolution, "buried_probes": buried, "blend_cells": a.blend, "directions": a.directions, "probe_samples": a.samples, "bounces": a.bounces,
                    "reference_spp": a.reference, "diffuse_pixels": int(mask.sum()), "inside_finest": int(inside.sum()), "band_weight": [1.0, 0.5, 0.0],
                    "classes": {"single_0": int((cls[mask] == PC.SINGLE).sum()), "blended": int(((cls[mask] >= PC.BLENDED) & (cls[mask] < PC.OUTSIDE)).sum()),
                                "coarsest": int((cls[mask] == PC.SINGLE + 2).sum()), "outside": int((cls[mask] == PC.OUTSIDE).sum())}}

            def errors(out):
                e = (lum(out) + glow - ref) / (ref + 0.01)
                rm = lambda m: round(float(np.sqrt(np.mean(e[m] * e[m]))), 4) if m.any() else None
                return {"rmse": rm(mask), "rmse_inside_finest": rm(inside), "rmse_outside_finest": rm(mask & ~inside),
                        "no_probe_share": round(float(np.mean(out[..., 3][mask] == 0)), 4)}

            for case, l in (("fine", 0), ("coarse", 2)):
                pt.set_probe_grid(grids[l].origin, grids[l].spacing, grids[l].counts)
                pt.shade_probe_grid_states(coefficients=coeff[l], states=rec[l], moments=mom[l], resolution=a.resolution, normal_weight=True, albedo=True,
                                           band_weight=PG.HEMISPHERE)
                line[case] = errors(pt.probe_grid_output())
            pt.set_probe_cascade([(g.origin, g.spacing, g.counts) for g in grids], a.resolution, a.blend)
            for l in range(3):
                pt.write_probe_cascade_level(l, "coefficients", coeff[l])
                pt.write_probe_cascade_level(l, "records", rec[l])
                pt.write_probe_cascade_level(l, "moments", mom[l])
            pt.shade_probe_cascade(depth=True, states=True, normal_weight=True, albedo=True, band_weight=PG.HEMISPHERE, count_work=True)
            line["cascade"] = dict(errors(pt.probe_grid_output()), work=pt.probe_cascade_work())
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
