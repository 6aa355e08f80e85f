#!/usr/bin/env python3
"""Kernel time and noise reduction of the temporal reprojection (srt_temporal_accumulate) on an MI355X — JSON lines.

    python tools/temporal_time.py time --width 1920 --height 1080    # median time of one call, with and without the framebuffer
    python tools/temporal_time.py time --width 3840 --height 2160
    python tools/temporal_time.py quality                            # the figures of tests/test_gpu_temporal.py (defaults)
    python tools/temporal_time.py sweep                              # the small parameter sweep that chose the defaults

time: Scene1 rendered at 1 spp with its first-hit guides made once; the tracer runs on a torch stream (srt_set_stream); after
--warmup calls (so that the history is valid and every tap is tested), each of --launches calls is bracketed by two events
on that stream and the median is reported, next to `render_kernel_ms` (a 1-spp, 8-bounce srt_render of the same frame) for
scale, and the compulsory bytes per pixel.
quality / sweep: Scene1 and Scene_indirect at 320 x 180, 8 bounces, 16 frames of 1 spp while the camera moves
(tests/test_gpu_temporal.py: moving_cameras) against an independent-seed 1024-spp render at the last camera; MSE of the
tone-mapped values c / (1 + c) over hit pixels, temporal against the plain 1-spp last frame, and the shift of the mean
linear colour against the reference.

GPU box only (profiles/temporal/ holds the committed lines).
"""
import argparse
import ctypes as C
import importlib
import itertools
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# compulsory traffic per hit pixel: object 4 B, normal / depth, point and accumulator 16 B each read; about three history
# float4 (16 B each) read, the four taps of neighbouring pixels sharing lines; 16 B accumulator and 48 B history written
BYTES_PER_PIXEL = 4 + 16 * 3 + 16 * 3 + 16 + 48


def _tracer(srt, scene, w, h):
    objs, n = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", scene + ".json")).objects_copy()
    pt = srt.PathTracer(w, h)
    pt.set_scene(objs, n)
    pt.set_camera(srt.default_camera())
    return pt, objs


def camera(srt, pos, yaw_deg):
    a = math.radians(yaw_deg)
    c = srt.Camera()
    c.position = (C.c_float * 3)(*[float(v) for v in pos])
    c.right = (C.c_float * 3)(math.cos(a), 0.0, -math.sin(a))
    c.up = (C.c_float * 3)(0.0, 1.0, 0.0)
    c.forward = (C.c_float * 3)(math.sin(a), 0.0, math.cos(a))
    c.fov_degrees = 55
    return c


def moving_cameras(srt, frames):
    # (the same sequence as tests/test_gpu_temporal.py)
    return [camera(srt, (0.004 * k, 0.0, 0.01 * k), 0.15 * k) for k in range(frames)]


def time_calls(srt, a):
    import torch

    w, h = a.width, a.height
    pt, keep = _tracer(srt, a.scene, w, h)
    stream = torch.cuda.Stream(device=0)
    pt.set_stream(stream.cuda_stream)
    render_ms = []
    for i in range(2 + 5):
        pt.render(spp=1, bounces=8, seed=0, reset=True)
        if i >= 2:
            render_ms.append(pt.stats().kernel_ms)
    pt.render_gbuffer(outputs=srt.capi.TEMPORAL_GUIDES)
    hits = int((pt.gbuffer("object") >= 0).sum())
    d = srt.capi.TEMPORAL_DEFAULTS
    for fb in (False, True):
        for _ in range(a.warmup):
            pt.temporal(samples=1, framebuffer=fb, gbuffer=False)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
        for b, e in ev:
            b.record(stream)
            pt.temporal(samples=1, framebuffer=fb, gbuffer=False)
            e.record(stream)
        stream.synchronize()
        ms = [b.elapsed_time(e) for b, e in ev]
        med = statistics.median(ms)
        compulsory = w * h * (BYTES_PER_PIXEL + (4 if fb else 0))
        print(json.dumps({
            "tool": "temporal_time", "mode": "time", "device": torch.cuda.get_device_name(0), "scene": a.scene, "width": w,
            "height": h, "framebuffer": fb, "max_samples": d["max_samples"], "plane_tolerance": d["plane_tolerance"],
            "normal_threshold": d["normal_threshold"], "launches": a.launches, "warmup": a.warmup,
            "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "render_kernel_ms": round(statistics.median(render_ms), 4),
            "render": "srt_render 1 spp, 8 bounces, same frame (median of 5)", "hit_pixels": hits,
            "compulsory_bytes_per_pixel": BYTES_PER_PIXEL + (4 if fb else 0),
            "compulsory_gbs": round(compulsory / (med * 1e-3) / 1e9, 1),
        }), flush=True)
    pt.set_stream(0)
    pt.close()


def _run(srt, pt, cams, frames, **kw):
    for k, cam in enumerate(cams[:frames]):
        pt.set_camera(cam)
        pt.render(spp=1, bounces=8, seed=1000 + k)
        pt.render_gbuffer(outputs=srt.capi.TEMPORAL_GUIDES)
        noisy = pt.accumulator()
        pt.temporal(samples=1, gbuffer=False, reset=k == 0, **kw)
    return noisy, pt.accumulator()


def quality(srt, a, grid):
    w, h, frames = 320, 180, 16
    cams = moving_cameras(srt, frames)
    for scene in ("Scene1", "Scene_indirect"):
        pt, keep = _tracer(srt, scene, w, h)
        pt.set_camera(cams[-1])
        pt.render(spp=1024, bounces=8, seed=777)
        ref = pt.accumulator()
        pt.render_gbuffer(outputs=srt.capi.TEMPORAL_GUIDES)
        hit = pt.gbuffer("object") >= 0

        def tm(x):
            return (x[..., :3] / (1.0 + x[..., :3]))[hit].astype(np.float64)

        def lin(x):
            return float(np.mean(x[..., :3][hit], dtype=np.float64))

        for kw in grid:
            noisy, got = _run(srt, pt, cams, frames, **kw)
            mse_noisy = float(np.mean((tm(noisy) - tm(ref)) ** 2))
            mse_t = float(np.mean((tm(got) - tm(ref)) ** 2))
            line = {"tool": "temporal_time", "mode": a.mode, "scene": scene, "width": w, "height": h, "bounces": 8, "frames": frames,
                    "spp": 1, "ref_spp": 1024}
            line.update(kw)
            line.update({"mse_1spp": mse_noisy, "mse_temporal": mse_t, "mse_ratio": round(mse_t / mse_noisy, 4),
                         "mean_shift": round(abs(lin(got) / lin(ref) - 1), 5),
                         "mean_shift_1spp": round(abs(lin(noisy) / lin(ref) - 1), 5),
                         "mean_history_length": round(float(np.mean(pt.history_length()[hit])), 3)})
            print(json.dumps(line), flush=True)
        pt.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["time", "quality", "sweep"])
    ap.add_argument("--scene", default="Scene1")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    srt = importlib.import_module("software-raytracer_amd")
    if a.mode == "time":
        time_calls(srt, a)
    elif a.mode == "quality":
        quality(srt, a, [{}])
    else:
        grid = [dict(max_samples=m, plane_tolerance=t, normal_threshold=n)
                for m, t, n in itertools.product([8.0, 16.0, 32.0, 64.0], [0.005, 0.02, 0.05], [-1.0, 0.9, 0.99])]
        quality(srt, a, grid)


if __name__ == "__main__":
    main()
