#!/usr/bin/env python3
"""Which probes leak where the filtered visibility test fails?  A diagnostic beside tools/probe_depth_quality.py, same protocol
(Scene_indirect and the closed room, 480 x 270, 4096-sample reference, hemisphere band weights, albedo, RMSE over the diffuse
pixels), grid spacings 1 and 0.5.  The probes that lie inside a box or a sphere are found on the host from the scene's geometry.
Per scene and spacing one record: how many probes are inside; the share of their rays at max_distance and at distance 0; the RMSE
of no test, the exact test and the filtered test; the filtered test again with the inside probes' moments set to (0, 0), which
makes rule 7b distrust them at every distance; and no test with the inside probes' coefficients set to 0.

    python tools/probe_depth_leak.py [OUT.json]

Prints one JSON object; GPU box only."""
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
from probe_grid_quality import lum  # noqa: E402
from probe_grid_time import bounds_grid  # noqa: E402

srt = importlib.import_module("software-raytracer_amd")
w, h = 480, 270
res = {}
for name in ("Scene_indirect", "closed_room"):
    scene = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", "Scene_indirect.json"))
    if name == "closed_room":
        wall = srt.Object()
        wall.type, wall.position[:], wall.half_size[:] = 2, (0.0, 0.0, -0.3), (6.0, 6.0, 0.2)
        wall.material.base_color[:] = (0.5, 0.5, 0.5)
        scene.add(wall, "wall behind the camera")
    objs, cnt = scene.objects_copy()
    geo = [(int(objs[i].type), list(objs[i].position), list(objs[i].half_size), float(objs[i].radius)) for i in range(cnt)]
    diffuse = np.array([objs[i].material.specular_amount == 0.0 for i in range(cnt)])
    emissive = np.array([list(objs[i].material.emissive_color) for i in range(cnt)], np.float64)
    pt = srt.PathTracer(w, h)
    pt.set_scene(objs, cnt)
    pt.set_camera(srt.default_camera())
    for first in range(1, 4097, 256):
        pt.render(spp=256, bounces=8, seed=2, first_sample=first, reset=(first == 1))
    ref = lum(pt.accumulator())
    pt.render_gbuffer()
    obj, pos = pt.gbuffer("object"), pt.gbuffer("position")
    mask = (obj != -1) & diffuse[np.maximum(obj, 0)]
    glow = lum(emissive[np.maximum(obj, 0)])
    def score():
        out = pt.probe_grid_output()
        e = (lum(out)[mask] + glow[mask] - ref[mask]) / (ref[mask] + 0.01)
        return round(float(np.sqrt(np.mean(e * e))), 4)
    out = {"types": sorted(set(g[0] for g in geo))}
    for spacing in (1.0, 0.5):
        grid = bounds_grid(obj, pos, spacing)
        P = srt.probe_grid_positions(grid.origin, grid.spacing, grid.counts)
        inside = np.zeros(len(P), bool)
        for t, c, hs, r in geo:
            d = P[:, :3].astype(np.float64) - np.array(c)
            if any(v > 0 for v in hs):
                inside |= (np.abs(d) < np.array(hs)).all(axis=1)
            if r > 0:
                inside |= (d * d).sum(axis=1) < r * r
        pt.trace_light_probes(P, 256, samples=16, bounces=8, seed=3)
        coeff = pt.light_probe_coefficients()
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        md = 1.5 * np.sqrt(3.0) * spacing
        pt.trace_probe_depth(resolution=16, sharpness=5, max_distance=md, distances=True)
        mom, dist = pt.probe_depth_output("moments"), pt.probe_depth_output("distances")
        row = {"probes": len(P), "inside": int(inside.sum()), "far_share_inside": round(float((dist[inside] >= np.float32(md)).mean()), 3) if inside.any() else None,
               "far_share_outside": round(float((dist[~inside] >= np.float32(md)).mean()), 3), "zero_share_inside": round(float((dist[inside] == 0).mean()), 3) if inside.any() else None}
        kw = dict(albedo=True, band_weight=PG.HEMISPHERE)
        pt.shade_probe_grid(coefficients=coeff, **kw); row["none"] = score()
        pt.shade_probe_grid(visibility=True, **kw); row["visibility"] = score()
        pt.shade_probe_grid_depth(moments=mom, resolution=16, **kw); row["depth"] = score()
        m2 = mom.copy(); m2[inside, :, 0] = 0.0; m2[inside, :, 1] = 0.0
        pt.shade_probe_grid_depth(moments=m2, resolution=16, **kw); row["depth_inside_probes_distrusted"] = score()
        c2 = coeff.copy(); c2[inside] = 0.0
        pt.shade_probe_grid(coefficients=c2, **kw); row["none_inside_probes_black"] = score()
        out[str(spacing)] = row
    res[name] = out
    pt.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
print(json.dumps(res))
