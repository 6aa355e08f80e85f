#!/usr/bin/env python3
"""Time of SRT_ADAPTIVE_SUN_SAMPLING in srt_render_adaptive and srt_render_adaptive_tail on an MI355X — one JSON line per scene.

Per scene — Scene1, Scene_indirect and BASELINE config 4's mesh scene (tools/rays_time.py's) — in a child process of its own
under its own time limit (--limit seconds; the first failure ends the run), a --width x --height frame (default 1920 x 1080) with a
uniform budget of --samples (default 32) from n = 0, flag off and flag on alternating:

    adaptive_B8   srt_render_adaptive at 8 bounces
    tail_B1       srt_render_adaptive_tail at 1 bounce with DEPTH | STATES (Scene1 and Scene_indirect; tools/probe_tail_time.py's
                  inputs: a 16 x 16 x 16 grid, seeded random coefficients, R = 8 moments, a tenth of the probes buried)
    radiance_B8   srt_trace_radiance on the same camera rays at 8 bounces, the strip form of adaptive_B8

The counts buffer holds 0 and every adaptive launch runs with SRT_ADAPTIVE_KEEP_COUNTS, so each launch adds the same samples from
n = 0.  Every figure is the median of --launches (default 20) launches after --warmup, each bracketed by two events on the tracer's
stream.  With each row the work records of both launches: under the flag wave_calls additionally counts the wave-level any-hit
invocations (rule AS8), so the difference is their number; closest_calls is the same.

    python tools/adaptive_sun_time.py --out profiles/adaptive_sun/adaptive_sun_time.jsonl

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

SCENES = {"Scene1": ("Scene1", None, True), "Scene_indirect": ("Scene_indirect", None, True), "config4_mesh224": ("Scene1", (224, 224), False)}


def step(a):
    import ctypes as C

    import numpy as np
    import rays_time as RT
    import torch
    from probe_tail_time import GRID, R

    srt = importlib.import_module("software-raytracer_amd")
    base, mesh, with_tail = SCENES[a.step]
    scene = RT.load_scene(srt, mesh) if mesh is not None else srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", base + ".json"))
    objs, cnt = scene.objects_copy()
    pt = srt.PathTracer(a.width, a.height)
    if mesh is not None:
        marr, mn = scene.meshes()
        pt.set_meshes(C.cast(marr, C.POINTER(srt.Mesh)), mn)
    pt.set_scene(objs, cnt)
    pt.set_camera(srt.default_camera())
    stream = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    pt.set_stream(stream.cuda_stream)
    o, d = RT.camera_rays(torch, a.width, a.height)
    torch.cuda.synchronize()
    pt.bind_rays(o, d)
    pt.set_sample_counts(0)
    pt.write_sample_budget(np.full((a.height, a.width), a.samples, np.uint32))
    out = {"device": torch.cuda.get_device_name(0)}

    def row(call, work):
        t = RT.timed(torch, stream, a.launches, a.warmup, {k: (lambda s=s: call(s, False)) for k, s in (("off", False), ("on", True))})
        r = dict(off=t["off"], on=t["on"], on_over_off=round(t["on"]["median_ms"] / t["off"]["median_ms"], 3))
        for k, s in (("off", False), ("on", True)):
            call(s, True)
            w = work()
            r["wave_calls_" + k], r["closest_calls_" + k], r["samples_" + k] = w["wave_calls"], w["closest_calls"], w["samples"]
        return r

    pt.probe_tail(enabled=False)
    out["adaptive_B8"] = row(lambda s, c: pt.render_adaptive(bounces=8, seed=0, keep_counts=True, sun_sampling=s, count_work=c), pt.adaptive_work)
    out["radiance_B8"] = row(lambda s, c: pt.trace_radiance(samples=a.samples, bounces=8, seed=0, sun_sampling=s, count_work=c), pt.radiance_work)
    out["tile_over_strip_on"] = round(out["adaptive_B8"]["on"]["median_ms"] / out["radiance_B8"]["on"]["median_ms"], 3)
    if with_tail:
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
        pt.probe_tail(enabled=True, depth=True, states=True, count_work=True)
        out["tail_B1"] = r = row(lambda s, c: pt.render_adaptive_tail(bounces=1, seed=0, keep_counts=True, sun_sampling=s, count_work=c), pt.adaptive_work)
        for k, s in (("off", False), ("on", True)):
            pt.render_adaptive_tail(bounces=1, seed=0, keep_counts=True, sun_sampling=s)
            r["tail_work_" + k] = pt.probe_tail_work()
        pt.probe_tail(enabled=False)
    pt.wait()
    pt.set_stream(0)
    pt.bind_rays(None, None)
    pt.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a scene may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=list(SCENES), default=None, help="(internal) run one scene in this process and print its JSON")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step(a)))
        return 0
    for scene in [s for s in a.scenes.split(",") if s]:  # each in a fresh process, under its own limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--step", scene] + [x for k in ("width", "height", "samples", "launches", "warmup")
                                                                             for x in ("--" + k, str(getattr(a, k)))]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            sys.stderr.write("adaptive_sun_time: scene %s ran into its limit of %d s; stopping\n" % (scene, a.limit))
            return 1
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            sys.stderr.write("adaptive_sun_time: scene %s failed (exit %d); stopping\n%s\n" % (scene, r.returncode, r.stderr[-2000:]))
            return 1
        line = {"tool": "adaptive_sun_time", "scene": scene, "width": a.width, "height": a.height, "samples": a.samples, "launches": a.launches,
                "warmup": a.warmup, "runs": "one run"}
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
