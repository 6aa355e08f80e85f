#!/usr/bin/env python3
"""Time of srt_trace_radiance and srt_trace_light_probes with and without the probe tail on an MI355X — one JSON line per scene.

Per scene (Scene1, Scene_indirect), in a child process of its own under its own time limit (--limit seconds; the first failure
ends the run):

    radiance      the --width x --height camera rays (default 1920 x 1080) at --samples (default 32) samples
    light_probes  a 16 x 16 x 16 grid of probes (4096) x --directions (default 256) directions at --probe-samples (default 16)

each for the rows  B = 8 mode off (the workload without the feature), B = 1 and B = 2 mode off, and B = 1 and B = 2 with the tail
(flags none / DEPTH / DEPTH | STATES).  The tail reads a 16 x 16 x 16 grid over the scene with seeded random finite coefficients,
R = 8 moments and records (a tenth of the probes buried): the cost of a lookup does not depend on what the arrays hold, only
on which corners rule 3s and 7b skip.  Every figure is the median of --launches (default 20) launches after --warmup, each
bracketed by two events on the tracer's stream.  `lookup_ms` of a tail row is its median minus the median of the same B with the
mode off.  The mode-off rows launch the kernels the parent commit has (identical assembly).

    python tools/probe_tail_time.py --out profiles/probe_tail/probe_tail_time.jsonl

The lines go to stdout, or are appended to --out FILE.  GPU box only."""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SCENES = ("Scene1", "Scene_indirect")
GRID = ((-4.0, -1.0, 0.5), (0.5, 0.25, 0.5), (16, 16, 16))
R = 8
ROWS = [("B8_off", 8, None), ("B1_off", 1, None), ("B2_off", 2, None)] + \
       [("B%d_tail_%s" % (b, n), b, f) for b in (1, 2) for n, f in (("none", {}), ("depth", {"depth": True}), ("depth_states", {"depth": True, "states": True}))]


def step(a):
    import ctypes as C

    import numpy as np
    import rays_time as RT
    import torch

    srt = importlib.import_module("software-raytracer_amd")
    scene = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", a.step + ".json"))
    objs, cnt = scene.objects_copy()
    pt = srt.PathTracer(a.width, a.height)
    pt.set_scene(objs, cnt)
    stream = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    pt.set_stream(stream.cuda_stream)
    rng = np.random.RandomState(7)
    P = GRID[2][0] * GRID[2][1] * GRID[2][2]
    co = rng.uniform(0.0, 1.0, (P, 9, 4)).astype(np.float32)
    m1 = rng.uniform(0.3, 3.0, (P, R * R)).astype(np.float32)
    mo = np.zeros((P, R * R, 4), np.float32)
    mo[..., 0], mo[..., 1] = m1, m1 * m1 + 0.05
    rec = np.zeros((P, 4), np.float32)
    rec[:, 3] = np.where(rng.rand(P) < 0.1, 2, 0).astype(np.uint32).view(np.float32)
    fp = lambda x: np.ascontiguousarray(x, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    pt.set_probe_grid(*GRID)
    pt._ck(pt.L.srt_write_probe_grid_coefficients(pt._h, fp(co), P))
    pt._ck(pt.L.srt_write_probe_grid_depth(pt._h, fp(mo), P, R))
    pt._ck(pt.L.srt_write_probe_grid_states(pt._h, fp(rec), P))
    o, d = RT.camera_rays(torch, a.width, a.height)
    torch.cuda.synchronize()
    pt.bind_rays(o, d)
    positions = srt.probe_grid_positions(*GRID)
    out = {"device": torch.cuda.get_device_name(0)}

    def mode(flags):
        if flags is None:
            pt.probe_tail(enabled=False)
        else:
            pt.probe_tail(enabled=True, **flags)

    for name, bounces, flags in ROWS:
        mode(flags)
        t = RT.timed(torch, stream, a.launches, a.warmup, {"x": lambda: pt.trace_radiance(samples=a.samples, bounces=bounces, seed=0)})["x"]
        out["radiance_" + name] = t
    first = True
    for name, bounces, flags in ROWS:
        mode(flags)
        kw = dict(positions=positions, directions=a.directions) if first else {}
        first = False
        pt.trace_light_probes(samples=a.probe_samples, bounces=bounces, seed=0, **kw)
        t = RT.timed(torch, stream, a.launches, a.warmup, {"x": lambda: pt.trace_light_probes(samples=a.probe_samples, bounces=bounces, seed=0)})["x"]
        out["light_probes_" + name] = t
    for kind in ("radiance_", "light_probes_"):
        for name, bounces, flags in ROWS:
            if flags is not None:
                out[kind + name]["lookup_ms"] = round(out[kind + name]["median_ms"] - out[kind + "B%d_off" % bounces]["median_ms"], 4)
    mode({"depth": True, "states": True, "count_work": True})
    pt.trace_radiance(samples=a.samples, bounces=1, seed=0)
    out["radiance_B1_tail_work"] = pt.probe_tail_work()
    pt.wait()
    pt.set_stream(0)
    pt.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--directions", type=int, default=256)
    ap.add_argument("--probe-samples", dest="probe_samples", type=int, default=16)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a scene may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=SCENES, default=None, help="(internal) run one scene in this process and print its JSON")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step(a)))
        return 0
    for scene in SCENES:  # each in a fresh process, under its own limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--step", scene] + [x for k in ("width", "height", "samples", "directions", "probe_samples", "launches", "warmup")
                                                                             for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            sys.stderr.write("probe_tail_time: scene %s ran into its limit of %d s; stopping\n" % (scene, a.limit))
            return 1
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            sys.stderr.write("probe_tail_time: scene %s failed (exit %d); stopping\n%s\n" % (scene, r.returncode, r.stderr[-2000:]))
            return 1
        line = {"tool": "probe_tail_time", "scene": scene, "width": a.width, "height": a.height, "samples": a.samples, "probes": 4096,
                "directions": a.directions, "probe_samples": a.probe_samples, "launches": a.launches, "warmup": a.warmup, "runs": "one run"}
        line.update(json.loads(res[-1][len("RESULT "):]))
        text = json.dumps(line) + "\n"
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(text)
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
