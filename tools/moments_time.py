#!/usr/bin/env python3
"""Kernel time and quality of the variance from the temporal history (srt_moments_output, srt_temporal_variance) on an MI355X —
JSON lines.

    python tools/moments_time.py time [--width 1920 --height 1080]   # profiles/denoise/moments_time_1080p.jsonl
    python tools/moments_time.py quality                             # profiles/denoise/moments_quality.jsonl

time: Scene1 and its first-hit buffers rendered once for each of two nearby cameras; the tracer is bound to a torch stream
(srt_set_stream) and its guides and variance to torch tensors.  The timed calls alternate between the two cameras, so that every
call reprojects over a real 2 x 2 footprint; the accumulator is rewritten from a copy before every call, outside the events.
After --warmup calls, each of --launches calls is bracketed by two events on that stream and the median is reported:
srt_temporal_accumulate with the moments output off and on (SRT_VARIANCE_ALBEDO), in the same run, then srt_temporal_variance
at radius 3 with every pixel old (min_frames = 0) and with every pixel young (min_frames = inf).
quality: the procedure of tests/test_gpu_moments.py — a scene at 96 x 64, 8 bounces, 8 frames of 1 spp of a moving camera against
2048 spp of the last camera; MSE of the tone-mapped values c / (1 + c) over hit pixels of the unfiltered temporal result, of
srt_temporal_variance + srt_denoise_variance and of srt_denoise on it, all at their defaults.

The lines go to stdout, or are appended to --out FILE.  GPU box only (profiles/denoise/ holds the committed lines).
"""
import argparse
import ctypes as C
import importlib
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
QUALITY_SCENES = ("Scene1", "Scene_indirect")


def _tracer(srt, scene, w, h):
    objs, n = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", scene + ".json")).objects_copy()
    pt = srt.PathTracer(w, h)
    pt.set_scene(objs, n)
    pt.set_camera(srt.default_camera())
    return pt, objs


def camera(srt, pos, yaw_deg):
    a = math.radians(yaw_deg)
    c = srt.default_camera()
    c.position = (C.c_float * 3)(*[float(v) for v in pos])
    c.right = (C.c_float * 3)(math.cos(a), 0.0, -math.sin(a))
    c.forward = (C.c_float * 3)(math.sin(a), 0.0, math.cos(a))
    return c


def moving_cameras(srt, frames):
    return [camera(srt, (0.004 * k, 0.0, 0.01 * k), 0.15 * k) for k in range(frames)]


def quality_figures(srt, scene="Scene1", w=96, h=64, bounces=8, frames=8, ref_spp=2048):
    pt, keep = _tracer(srt, scene, w, h)
    cams = moving_cameras(srt, frames)
    pt.moments_output(True, albedo=True)
    for k, cam in enumerate(cams):
        pt.set_camera(cam)
        pt.render(spp=1, bounces=bounces, seed=1000 + k)
        pt.render_gbuffer()
        pt.temporal(samples=1, gbuffer=False)
    plain = pt.accumulator()
    hit = pt.gbuffer("object") >= 0
    lm = pt.moments()[..., 2]
    pt.temporal_variance()
    var = pt.variance_map()
    pt.denoise_variance(gbuffer=False)
    dv = pt.denoised()
    pt.denoise(gbuffer=False)
    dn = pt.denoised()
    pt.render(spp=ref_spp, bounces=bounces, seed=777)
    ref = pt.accumulator()
    pt.close()

    def tm(x):
        return (x[..., :3] / (1.0 + x[..., :3]))[hit].astype(np.float64)

    def mse(x):
        return float(np.mean((tm(x) - tm(ref)) ** 2))

    d = srt.capi.TEMPORAL_VARIANCE_DEFAULTS
    return {"tool": "moments_time", "mode": "quality", "scene": scene, "width": w, "height": h, "bounces": bounces, "frames": frames,
            "spp": 1, "ref_spp": ref_spp, "hit_pixels": int(hit.sum()), "young_pixels": int((hit & (lm < d["min_frames"])).sum()),
            "mean_variance": float(np.mean(var[hit], dtype=np.float64)), "mse_temporal": mse(plain),
            "mse_temporal_variance": mse(dv), "mse_denoise": mse(dn)}


def time_passes(srt, a):
    import torch

    w, h = a.width, a.height
    pt, keep = _tracer(srt, a.scene, w, h)
    stream = torch.cuda.Stream(device=0)
    pt.set_stream(stream.cuda_stream)
    cams = moving_cameras(srt, 2)
    sets = []
    for cam in cams:
        bufs = {"object": torch.empty((h, w), dtype=torch.int32, device="cuda:0")}
        for k in ("normal_depth", "position", "albedo"):
            bufs[k] = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        for k, t in bufs.items():
            pt.bind_gbuffer(k, t)
        pt.set_camera(cam)
        pt.render_gbuffer()
        sets.append(bufs)
    var = torch.empty((h, w), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    pt.bind_variance(var)
    pt.render(spp=1, bounces=8, seed=0)
    pt.wait()
    acc0 = pt.accumulator()
    turn = [0]

    def next_frame():
        i = turn[0] = 1 - turn[0]
        for k, t in sets[i].items():
            pt.bind_gbuffer(k, t)
        pt.set_camera(cams[i])
        pt.write_accumulator(acc0)

    def timed(call, before=None):
        for _ in range(a.warmup):
            if before:
                before()
            call()
        ms = []
        for _ in range(a.launches):
            if before:
                before()
            b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b.record(stream)
            call()
            e.record(stream)
            stream.synchronize()
            ms.append(b.elapsed_time(e))
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}

    head = {"tool": "moments_time", "mode": "time", "device": torch.cuda.get_device_name(0), "scene": a.scene, "width": w, "height": h,
            "launches": a.launches, "warmup": a.warmup}
    lines = []
    for on in (False, True):
        pt.moments_output(on, albedo=True)
        t = timed(lambda: pt.temporal(samples=1, gbuffer=False), before=next_frame)
        lines.append(dict(head, **{"pass": "srt_temporal_accumulate", "moments": int(on)}, **t))
    lines[1]["on_off_ratio"] = round(lines[1]["median_ms"] / lines[0]["median_ms"], 3)
    for name, mf in (("old", 0.0), ("young", float("inf"))):
        t = timed(lambda: pt.temporal_variance(min_frames=mf, radius=3))
        if name == "old":  # compulsory traffic per pixel: the record (16 B) and the object (4 B) read, 4 B written
            t["compulsory_gbs"] = round(w * h * 24 / (t["median_ms"] * 1e-3) / 1e9, 1)
        lines.append(dict(head, **{"pass": "srt_temporal_variance", "pixels": name, "min_frames": str(mf), "radius": 3}, **t))
    pt.bind_variance(None)
    for k in sets[0]:
        pt.bind_gbuffer(k, None)
    pt.set_stream(0)
    pt.close()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["time", "quality"])
    ap.add_argument("--scene", default="Scene1")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the lines to this file instead of printing them")
    a = ap.parse_args()
    srt = importlib.import_module("software-raytracer_amd")
    lines = time_passes(srt, a) if a.mode == "time" else [quality_figures(srt, s) for s in QUALITY_SCENES]
    text = "".join(json.dumps(line) + "\n" for line in lines)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
