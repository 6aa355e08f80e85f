#!/usr/bin/env python3
"""Time of the probe depth pass (srt_trace_probe_depth) and of the filtered probe-grid shading (srt_shade_probe_grid_depth) on an
MI355X, each next to its yardsticks measured in the same run — JSON lines, one per scene and part.

Scenes (--scenes): Scene1, Scene_indirect, and BASELINE config 4's mesh scene (Scene1 with its big ball as a 224 x 224 lat-long
sphere, 99,904 triangles: tools/rays_time.py builds it).  Every time is the median of --launches event-bracketed launches after
--warmup, the calls of a part alternating launch by launch (tools/rays_time.py: timed).

    depth    (a) srt_trace_probe_depth for --probes (default 4096) seeded random positions in [-5, 5] x [-1, 4] x [0, 10] and
             --directions (default 256) spherical Fibonacci directions, resolution --resolution (16), sharpness --sharpness (5),
             MOMENTS only; next to srt_trace_rays with NORMAL_DEPTH only on the explicit P*K rays, bound on the device.  The
             difference is what forming the rays on the device saves and the projection costs.
    shade    (b) at --width x --height (default 1920 x 1080), tools/probe_grid_time.py's grid (--spacing, default 1.0) and seeded
             random coefficients: srt_shade_probe_grid without a test and with SRT_PROBE_GRID_VISIBILITY, and
             srt_shade_probe_grid_depth with moments traced by srt_trace_probe_depth at the grid's positions (max_distance = 1.5
             cell diagonals) and bound device to device; the depth call's ratio to both, and the work counts of one counting call each.

    python tools/probe_depth_time.py --out profiles/probe_depth/probe_depth_time.jsonl

The lines go to stdout, or are appended to --out FILE.  GPU box only."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rays_time as R  # noqa: E402  (timed, load_scene)
from probe_grid_time import bounds_grid  # noqa: E402

SCENES = {"Scene1": None, "Scene_indirect": None, "config4_mesh224": (224, 224)}


def open_tracer(srt, name, w, h):
    if SCENES[name] is None:
        scene = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", name + ".json"))
        assert scene.error == "", scene.error
    else:
        scene = R.load_scene(srt, SCENES[name])
    objs, n = scene.objects_copy()
    pt = srt.PathTracer(w, h)
    if SCENES[name] is not None:
        marr, mn = scene.meshes()
        pt.set_meshes(C.cast(marr, C.POINTER(srt.Mesh)), mn)
    pt.set_scene(objs, n)
    pt.set_camera(srt.default_camera())
    return pt, scene


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--parts", default="depth,shade")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--probes", type=int, default=4096)
    ap.add_argument("--directions", type=int, default=256)
    ap.add_argument("--resolution", type=int, default=16)
    ap.add_argument("--sharpness", type=int, default=5)
    ap.add_argument("--spacing", type=float, default=1.0)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    srt = importlib.import_module("software-raytracer_amd")
    w, h = a.width, a.height
    dev = "cuda:0"
    lines = []
    for name in a.scenes.split(","):
        pt, scene = open_tracer(srt, name, w, h)
        stream = torch.cuda.Stream(device=0)
        torch.cuda.synchronize()
        pt.set_stream(stream.cuda_stream)
        base = {"device": torch.cuda.get_device_name(0), "scene": name, "launches": a.launches, "warmup": a.warmup}
        if "depth" in a.parts.split(","):
            P, K, Rz = a.probes, a.directions, a.resolution
            rng = np.random.default_rng(1)
            pos = np.zeros((P, 4), np.float32)
            pos[:, :3] = rng.uniform((-5.0, -1.0, 0.0), (5.0, 4.0, 10.0), (P, 3))
            d = srt.light_probe_sphere(K)
            o_t = torch.from_numpy(np.repeat(pos, K, axis=0)).to(dev)
            d_t = torch.from_numpy(np.tile(d, (P, 1))).to(dev)
            nd_t = torch.empty((P * K, 4), dtype=torch.float32, device=dev)
            mom_t = torch.empty((P * Rz * Rz, 4), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            pt.bind_rays(o_t, d_t)
            pt.bind_ray_output("normal_depth", nd_t)
            pt.bind_probe_depth_output("moments", mom_t)
            kw = dict(resolution=Rz, sharpness=a.sharpness, max_distance=10000.0)
            pt.trace_probe_depth(pos, d, **kw)
            calls = {"probe_depth": lambda: pt.trace_probe_depth(**kw), "trace_rays": lambda: pt.trace_rays(outputs=["normal_depth"])}
            t = R.timed(torch, stream, a.launches, a.warmup, calls)
            pt.trace_probe_depth(count_work=True, **kw)
            line = dict(base, tool="probe_depth_time", part="depth", probes=P, directions=K, resolution=Rz, sharpness=a.sharpness,
                        probe_depth=dict(t["probe_depth"], work=pt.probe_depth_work()), trace_rays=t["trace_rays"],
                        probe_depth_minus_trace_rays_ms=round(t["probe_depth"]["median_ms"] - t["trace_rays"]["median_ms"], 4),
                        probe_depth_to_trace_rays=round(t["probe_depth"]["median_ms"] / t["trace_rays"]["median_ms"], 3))
            lines.append(line)
            pt.wait()
            pt.bind_rays(None, None)
            pt.bind_ray_output("normal_depth", None)
            pt.bind_probe_depth_output("moments", None)
            del o_t, d_t, nd_t, mom_t
        if "shade" in a.parts.split(","):
            pt.render_gbuffer(outputs=["object", "normal_depth", "position"])
            obj, posb = pt.gbuffer("object"), pt.gbuffer("position")
            grid = bounds_grid(obj, posb, a.spacing)
            coeff = np.random.default_rng(7).uniform(0.0, 2.0, (grid.probes, 9, 4)).astype(np.float32)
            Rz = a.resolution
            diag = float(np.sqrt(3.0) * a.spacing)
            mom_t = torch.empty((grid.probes * Rz * Rz, 4), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            pt.bind_probe_depth_output("moments", mom_t)
            pt.trace_probe_depth(srt.probe_grid_positions(grid.origin, grid.spacing, grid.counts), a.directions, resolution=Rz, sharpness=a.sharpness,
                                 max_distance=1.5 * diag)
            pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
            pt.shade_probe_grid(coefficients=coeff)
            pt.shade_probe_grid_depth(moments=mom_t, resolution=Rz)
            calls = {"none": lambda: pt.shade_probe_grid(), "visibility": lambda: pt.shade_probe_grid(visibility=True), "depth": lambda: pt.shade_probe_grid_depth()}
            t = R.timed(torch, stream, a.launches, a.warmup, calls)
            line = dict(base, tool="probe_depth_time", part="shade", width=w, height=h, hit_pixels=int((obj != -1).sum()), grid_spacing=a.spacing,
                        grid_counts=list(grid.counts), probes=grid.probes, resolution=Rz, sharpness=a.sharpness, directions=a.directions)
            for case, fn in (("none", lambda: pt.shade_probe_grid(count_work=True)), ("visibility", lambda: pt.shade_probe_grid(visibility=True, count_work=True)),
                             ("depth", lambda: pt.shade_probe_grid_depth(count_work=True))):
                fn()
                line[case] = dict(t[case], work=pt.probe_grid_work())
            line["depth_to_none"] = round(t["depth"]["median_ms"] / t["none"]["median_ms"], 3)
            line["depth_to_visibility"] = round(t["depth"]["median_ms"] / t["visibility"]["median_ms"], 3)
            lines.append(line)
            pt.wait()
            pt.bind_probe_depth_output("moments", None)
            pt.bind_probe_grid_depth(None)
            del mom_t
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
