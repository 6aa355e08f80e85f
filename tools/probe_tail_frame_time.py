#!/usr/bin/env python3
"""Time of a frame under the probe tail (srt_render_adaptive_tail) on an MI355X — one JSON line per scene.

Per scene (Scene1, Scene_indirect), in a child process of its own under its own time limit (--limit seconds; the first failure
ends the run), a --width x --height frame (default 1920 x 1080) with a uniform budget of --samples (default 32) from n = 0:

    adaptive_B8, adaptive_B1         srt_render_adaptive at 8 bounces and at 1 (the mode is ignored)
    tail_B1_none / _depth / _depth_states
                                     srt_render_adaptive_tail at 1 bounce, flags none, DEPTH, DEPTH | STATES
    radiance_B1_tail_depth_states    srt_trace_radiance under the mode (DEPTH | STATES) on the frame's camera rays at 1 bounce

The counts buffer holds 0 and every adaptive launch runs with SRT_ADAPTIVE_KEEP_COUNTS, so each launch adds the same samples from
n = 0 and no fill stands between the launches.  The tail reads tools/probe_tail_time.py's inputs: a 16 x 16 x 16 grid over the scene
with seeded random finite coefficients, R = 8 moments and records (a tenth of the probes buried).  Every figure is the median of
--launches (default 20) launches after --warmup, each bracketed by two events on the tracer's stream.  Derived:

    lookup_ms     tail_B1_x minus adaptive_B1: the cost of the lookups
    tile_form_ms  tail_B1_depth_states minus radiance_B1_tail_depth_states: the cost of the tile form (camera rays made in the
                  kernel, per-lane sample bounds, the ticket, tone mapping and the framebuffer) against the strip form

    python tools/probe_tail_frame_time.py --out profiles/probe_tail_frame/probe_tail_frame_time.jsonl

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
TAIL_ROWS = (("none", {}), ("depth", {"depth": True}), ("depth_states", {"depth": True, "states": True}))


def step(a):
    import ctypes as C

    import numpy as np
    import rays_time as RT
    import torch
    from probe_tail_time import GRID, R

    srt = importlib.import_module("software-raytracer_amd")
    scene = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", a.step + ".json"))
    objs, cnt = scene.objects_copy()
    pt = srt.PathTracer(a.width, a.height)
    pt.set_scene(objs, cnt)
    pt.set_camera(srt.default_camera())
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
    pt.set_sample_counts(0)
    pt.write_sample_budget(np.full((a.height, a.width), a.samples, np.uint32))
    out = {"device": torch.cuda.get_device_name(0)}

    def timed(fn):
        return RT.timed(torch, stream, a.launches, a.warmup, {"x": fn})["x"]

    pt.probe_tail(enabled=False)
    for b in (8, 1):
        out["adaptive_B%d" % b] = timed(lambda: pt.render_adaptive(bounces=b, seed=0, keep_counts=True))
    for name, flags in TAIL_ROWS:
        pt.probe_tail(enabled=True, **flags)
        out["tail_B1_" + name] = t = timed(lambda: pt.render_adaptive_tail(bounces=1, seed=0, keep_counts=True))
        t["lookup_ms"] = round(t["median_ms"] - out["adaptive_B1"]["median_ms"], 4)
    out["radiance_B1_tail_depth_states"] = timed(lambda: pt.trace_radiance(samples=a.samples, bounces=1, seed=0))
    out["tile_form_ms"] = round(out["tail_B1_depth_states"]["median_ms"] - out["radiance_B1_tail_depth_states"]["median_ms"], 4)
    out["tail_B1_over_adaptive_B8"] = round(out["tail_B1_depth_states"]["median_ms"] / out["adaptive_B8"]["median_ms"], 4)
    pt.probe_tail(enabled=True, depth=True, states=True, count_work=True)
    pt.render_adaptive_tail(bounces=1, seed=0, keep_counts=True, count_work=True)
    out["tail_B1_work"], out["tail_B1_adaptive_work"] = pt.probe_tail_work(), pt.adaptive_work()
    pt.wait()
    pt.set_stream(0)
    pt.bind_rays(None, None)
    pt.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=32)
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
        cmd = [sys.executable, os.path.abspath(__file__), "--step", scene] + [x for k in ("width", "height", "samples", "launches", "warmup")
                                                                             for x in ("--" + k, str(getattr(a, k)))]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            sys.stderr.write("probe_tail_frame_time: scene %s ran into its limit of %d s; stopping\n" % (scene, a.limit))
            return 1
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            sys.stderr.write("probe_tail_frame_time: scene %s failed (exit %d); stopping\n%s\n" % (scene, r.returncode, r.stderr[-2000:]))
            return 1
        line = {"tool": "probe_tail_frame_time", "scene": scene, "width": a.width, "height": a.height, "samples": a.samples, "probes": 4096,
                "launches": a.launches, "warmup": a.warmup, "runs": "one run"}
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
