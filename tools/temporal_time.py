#!/usr/bin/env python3
"""Kernel time and noise reduction of the temporal reprojection (srt_temporal_accumulate) on an MI355X — JSON lines.

    python tools/temporal_time.py time --width 1920 --height 1080    # median time of one call, with and without the framebuffer
    python tools/temporal_time.py time --width 3840 --height 2160
    python tools/temporal_time.py quality                            # the figures of tests/test_gpu_temporal.py (defaults)
    python tools/temporal_time.py sweep                              # the small parameter sweep that chose the defaults
    python tools/temporal_time.py motion --width 1920 --height 1080  # the call with a motion table and / or the motion output
    python tools/temporal_time.py motion --base build/ab/libsrt_parent.so   # ... and the plain call against another build

time: Scene1 rendered at 1 spp with its first-hit guides made once; the tracer runs on a torch stream (srt_set_stream); after
--warmup calls (so that the history is valid and every tap is tested), each of --launches calls is bracketed by two events
on that stream and the median is reported, next to `render_kernel_ms` (a 1-spp, 8-bounce srt_render of the same frame) for
scale, and the compulsory bytes per pixel.
motion: as time (no framebuffer), for the four instantiations: plain, motion output, motion table (every object of the scene
moved back and forth by srt_update_scene between the calls, so every call uploads a table and gathers from it), and both; the
update itself is outside the bracket.  With --base PATH (a build of the library without these entry points, e.g. the parent
commit's) the PLAIN call is also timed on that build, twice, interleaved call by call with this build in one process: the
two base series give the A/A spread the new build's median has to lie within.
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


def _open_base(srt, path):
    """A build that may lack the newer entry points: only what the plain temporal call needs is declared."""
    L = C.CDLL(os.path.join(ROOT, path))
    ctx, cap = C.c_void_p, srt.capi
    for name, args in (("srt_create", [C.c_int, C.c_int, C.c_int, C.POINTER(ctx)]), ("srt_destroy", [ctx]),
                       ("srt_set_scene", [ctx, C.POINTER(cap.Object), C.c_size_t]), ("srt_set_camera", [ctx, C.POINTER(cap.Camera)]),
                       ("srt_set_stream", [ctx, C.c_void_p]), ("srt_render", [ctx, C.POINTER(cap.RenderParams)]),
                       ("srt_render_gbuffer", [ctx, C.POINTER(cap.GBufferParams)]), ("srt_wait", [ctx]),
                       ("srt_temporal_params_default", [C.POINTER(cap.TemporalParams)]),
                       ("srt_temporal_accumulate", [ctx, C.POINTER(cap.TemporalParams)])):
        getattr(L, name).argtypes = args
        getattr(L, name).restype = C.c_int
    L.srt_last_error.argtypes = [ctx]
    L.srt_last_error.restype = C.c_char_p
    return L


def _bracket(torch, stream, calls, launches, warmup, between=None):
    """Per-call event times of several callables run in turn (interleaved), `between` (untimed) before each."""
    ms = [[] for _ in calls]
    for r in range(warmup + launches):
        for i, call in enumerate(calls):
            if between:
                between(i)
            b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b.record(stream)
            call()
            e.record(stream)
            if r >= warmup:
                ms[i].append((b, e))
    stream.synchronize()
    return [[b.elapsed_time(e) for b, e in row] for row in ms]


def motion_calls(srt, a):
    import torch

    w, h = a.width, a.height
    stream = torch.cuda.Stream(device=0)
    scene_file = os.path.join(ROOT, "software-raytracer_amd", "scenes", a.scene + ".json")
    objs, n = srt.host.Scene(scene_file).objects_copy()
    moved = (srt.Object * n)()
    for i in range(n):
        moved[i] = objs[i]
        moved[i].position = (C.c_float * 3)(objs[i].position[0] + 0.01, objs[i].position[1], objs[i].position[2] + 0.005)
    base = dict(tool="temporal_time", mode="motion", device=torch.cuda.get_device_name(0), scene=a.scene, width=w, height=h,
                objects=n, launches=a.launches, warmup=a.warmup)

    def tracer(lib):
        pt = srt.PathTracer(w, h, lib=lib)
        pt.set_scene(objs, n)
        pt.set_camera(srt.default_camera())
        pt.set_stream(stream.cuda_stream)
        pt.render(spp=1, bounces=8, seed=0, reset=True)
        pt.render_gbuffer(outputs=srt.capi.TEMPORAL_GUIDES)
        return pt

    pt = tracer(None)
    flip = [0]

    def update(_):
        flip[0] ^= 1
        pt.update_scene(moved if flip[0] else objs, n)
        pt.wait()  # the scene upload is not part of the call that is timed

    for table, mv in ((False, False), (False, True), (True, False), (True, True)):
        pt.motion_output(mv)
        ms = _bracket(torch, stream, [lambda: pt.temporal(samples=1, gbuffer=False)], a.launches, a.warmup, update if table else None)[0]
        med = statistics.median(ms)
        extra = (16 if table else 0) + (16 if mv else 0)
        line = dict(base, table=table, motion_output=mv, median_ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                    compulsory_bytes_per_pixel=BYTES_PER_PIXEL + extra, extra_bytes_per_pixel=extra,
                    compulsory_gbs=round(w * h * (BYTES_PER_PIXEL + extra) / (med * 1e-3) / 1e9, 1))
        print(json.dumps(line), flush=True)
    pt.motion_output(False)
    pt.update_scene(objs, n)
    if a.base:
        old = _open_base(srt, a.base)
        pts = [tracer(old), pt, tracer(old)]
        rows = _bracket(torch, stream, [lambda p=p: p.temporal(samples=1, gbuffer=False) for p in pts], a.launches, a.warmup)
        med = [statistics.median(r) for r in rows]
        spread = abs(med[0] - med[2]) / min(med[0], med[2])
        ratio = med[1] / (0.5 * (med[0] + med[2]))
        print(json.dumps(dict(base, comparison="plain call, interleaved", base_library=a.base, base_a_median_ms=round(med[0], 4),
                              new_median_ms=round(med[1], 4), base_b_median_ms=round(med[2], 4), base_aa_spread=round(spread, 4),
                              new_vs_base_mean=round(ratio, 4), within_aa=bool(abs(ratio - 1) <= spread))), flush=True)
        for p in (pts[0], pts[2]):
            p.set_stream(0)
            p.close()
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
    ap.add_argument("mode", choices=["time", "quality", "sweep", "motion"])
    ap.add_argument("--base", default="", help="motion: another build of the library to time the plain call against")
    ap.add_argument("--scene", default="Scene1")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    srt = importlib.import_module("software-raytracer_amd")
    if a.mode == "time":
        time_calls(srt, a)
    elif a.mode == "motion":
        motion_calls(srt, a)
    elif a.mode == "quality":
        quality(srt, a, [{}])
    else:
        grid = [dict(max_samples=m, plane_tolerance=t, normal_threshold=n)
                for m, t, n in itertools.product([8.0, 16.0, 32.0, 64.0], [0.005, 0.02, 0.05], [-1.0, 0.9, 0.99])]
        quality(srt, a, grid)


if __name__ == "__main__":
    main()
