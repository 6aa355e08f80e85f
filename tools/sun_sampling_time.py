#!/usr/bin/env python3
"""Time of sun sampling at diffuse bounces (SRT_RADIANCE_SUN_SAMPLING, SRT_LIGHT_PROBE_SUN_SAMPLING) on an MI355X — JSON lines.

Per scene — Scene1, Scene_indirect and BASELINE config 4's mesh scene (tools/rays_time.py's) — flag off and flag on, the two
launches alternating, medians of --launches (20) event-timed launches after --warmup:

    radiance   srt_trace_radiance on the camera rays of a --width x --height (1920 x 1080) frame, 32 samples x 8 bounces
    probes     srt_trace_light_probes at --probes (4096) x --directions (256), 16 samples x 8 bounces

and, for scale, the work records of both launches: under the flag wave_calls additionally counts the wave-level any-hit
invocations (rule S9), so the difference of the two is their number; closest_calls is the same.

    python tools/sun_sampling_time.py --out profiles/sun_sampling/sun_sampling_time.jsonl

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

SCENES = {"Scene1": ("Scene1", None), "Scene_indirect": ("Scene_indirect", None), "config4_mesh224": ("Scene1", (224, 224))}


def load(srt, name):
    import rays_time as RT

    base, mesh = SCENES[name]
    if mesh is not None:
        return RT.load_scene(srt, mesh), True
    return srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", base + ".json")), False


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--probes", type=int, default=4096)
    ap.add_argument("--directions", type=int, default=256)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import rays_time as RT
    import torch

    srt = importlib.import_module("software-raytracer_amd")
    w, h = a.width, a.height
    lines = []
    for name in a.scenes.split(","):
        scene, has_mesh = load(srt, name)
        objs, n = scene.objects_copy()
        pt = srt.PathTracer(w, h)
        if has_mesh:
            marr, mn = scene.meshes()
            pt.set_meshes(C.cast(marr, C.POINTER(srt.Mesh)), mn)
        pt.set_scene(objs, n)
        pt.set_camera(srt.default_camera())
        stream = torch.cuda.Stream(device=0)
        o, d = RT.camera_rays(torch, w, h)
        rad = torch.empty((w * h, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        pt.set_stream(stream.cuda_stream)
        pt.bind_rays(o, d)
        pt.bind_radiance(rad)
        base = {"tool": "sun_sampling_time", "device": torch.cuda.get_device_name(0), "scene": name, "launches": a.launches, "warmup": a.warmup, "runs": "one run"}
        t = RT.timed(torch, stream, a.launches, a.warmup, {k: (lambda s=s: pt.trace_radiance(samples=32, bounces=8, seed=1, sun_sampling=s))
                                                           for k, s in (("off", False), ("on", True))})
        work = {}
        for k, s in (("off", False), ("on", True)):
            pt.trace_radiance(samples=32, bounces=8, seed=1, sun_sampling=s, count_work=True)
            work[k] = pt.radiance_work()
        lines.append(dict(base, part="radiance", rays=w * h, samples=32, bounces=8, off=t["off"], on=t["on"],
                          on_over_off=round(t["on"]["median_ms"] / t["off"]["median_ms"], 3), wave_calls_off=work["off"]["wave_calls"],
                          wave_calls_on=work["on"]["wave_calls"], closest_calls_off=work["off"]["closest_calls"], closest_calls_on=work["on"]["closest_calls"]))
        # probes: a grid over the scene, --probes of them
        side = int(round(a.probes ** (1.0 / 3.0)))
        pos = srt.probe_grid_positions((-4.0, -0.5, 0.5), (8.0 / side, 4.0 / side, 8.0 / side), (side, side, side))[:a.probes]
        pt.trace_light_probes(np.ascontiguousarray(pos), a.directions, samples=1, bounces=1)
        t = RT.timed(torch, stream, a.launches, a.warmup, {k: (lambda s=s: pt.trace_light_probes(samples=16, bounces=8, seed=1, sun_sampling=s))
                                                           for k, s in (("off", False), ("on", True))})
        work = {}
        for k, s in (("off", False), ("on", True)):
            pt.trace_light_probes(samples=16, bounces=8, seed=1, sun_sampling=s, count_work=True)
            work[k] = pt.light_probe_work()
        lines.append(dict(base, part="probes", probes=len(pos), directions=a.directions, samples=16, bounces=8, off=t["off"], on=t["on"],
                          on_over_off=round(t["on"]["median_ms"] / t["off"]["median_ms"], 3), wave_calls_off=work["off"]["wave_calls"],
                          wave_calls_on=work["on"]["wave_calls"], closest_calls_off=work["off"]["closest_calls"], closest_calls_on=work["on"]["closest_calls"]))
        pt.wait()
        pt.set_stream(0)
        pt.bind_rays(None, None)
        pt.bind_radiance(None)
        pt.close()
    text = "".join(json.dumps(l) + "\n" for l in lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "a").write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
