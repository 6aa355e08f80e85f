#!/usr/bin/env python3
"""Kernel time and noise reduction of the denoiser (srt_denoise) on an MI355X — JSON lines.

    python tools/denoise_time.py time --width 1920 --height 1080     # median time of L = 1..5 (one line per L)
    python tools/denoise_time.py time --width 3840 --height 2160
    python tools/denoise_time.py quality                             # the noise-reduction figures of tests/test_gpu_denoise.py
    python tools/denoise_time.py sweep                               # the small parameter sweep that chose the defaults

time: Scene1 rendered at 1 spp and its first-hit buffers made once; the tracer is bound to a torch stream (srt_set_stream),
its guides and result to torch tensors; after --warmup calls, each of --launches srt_denoise calls (all levels) is bracketed
by two events on that stream and the median is reported, next to `render_kernel_ms` (a 1-spp, 8-bounce srt_render of the
same frame) for scale, and the bytes per pixel and level the kernel asks of the memory system.
quality / sweep: Scene1 and Scene_indirect at 320 x 180, 4 spp against an independent-seed 1024-spp render; MSE of the
tone-mapped values c / (1 + c) over hit pixels, denoised against noisy, and the shift of the mean linear colour (and of
the tone-mapped mean, which the tone map's concavity moves up on any smoothing).

GPU box only (profiles/denoise/ holds the committed lines).
"""
import argparse
import importlib
import itertools
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _tracer(srt, scene, w, h):
    objs, n = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", scene + ".json")).objects_copy()
    pt = srt.PathTracer(w, h)
    pt.set_scene(objs, n)
    pt.set_camera(srt.default_camera())
    return pt, objs


def time_levels(srt, a):
    import torch

    w, h = a.width, a.height
    pt, keep = _tracer(srt, a.scene, w, h)
    stream = torch.cuda.Stream(device=0)
    pt.set_stream(stream.cuda_stream)
    bufs = {"object": torch.empty((h, w), dtype=torch.int32, device="cuda:0")}
    for k in ("normal_depth", "position", "albedo"):
        bufs[k] = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
    out = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    for k, t in bufs.items():
        pt.bind_gbuffer(k, t)
    pt.bind_denoised(out)
    render_ms = []
    for i in range(2 + 5):
        pt.render(spp=1, bounces=8, seed=0, reset=True)
        if i >= 2:
            render_ms.append(pt.stats().kernel_ms)
    pt.render_gbuffer()
    hits = int((bufs["object"] >= 0).sum().item())
    d = srt.capi.DENOISE_DEFAULTS
    for levels in range(1, a.max_levels + 1):
        for _ in range(a.warmup):
            pt.denoise(iterations=levels, gbuffer=False)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
        for b, e in ev:
            b.record(stream)
            pt.denoise(iterations=levels, gbuffer=False)
            e.record(stream)
        stream.synchronize()
        ms = [b.elapsed_time(e) for b, e in ev]
        med = statistics.median(ms)
        # compulsory traffic: per level, object (4 B), colour, normal/depth and point (16 B each) read and 16 B stored per
        # pixel; the preparation pass reads the accumulator and the albedo and stores 16 B
        compulsory = w * h * (4 + 16 * 4) * levels + w * h * (4 + 16 * 3)
        print(json.dumps({
            "tool": "denoise_time", "mode": "time", "device": torch.cuda.get_device_name(0), "scene": a.scene, "width": w,
            "height": h, "iterations": levels, "sigma_color": d["sigma_color"], "sigma_normal": d["sigma_normal"],
            "sigma_plane": d["sigma_plane"], "flags": d["flags"], "launches": a.launches, "warmup": a.warmup,
            "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "ms_per_level": round(med / levels, 4), "render_kernel_ms": round(statistics.median(render_ms), 4),
            "render": "srt_render 1 spp, 8 bounces, same frame (median of 5)", "hit_pixels": hits,
            "compulsory_gbs": round(compulsory / (med * 1e-3) / 1e9, 1),
        }), flush=True)
    pt.bind_denoised(None)
    for k in bufs:
        pt.bind_gbuffer(k, None)
    pt.set_stream(0)
    pt.close()


def _frames(srt, scene, w, h, spp, ref_spp):
    pt, keep = _tracer(srt, scene, w, h)
    pt.render(spp=ref_spp, bounces=4, seed=777)
    ref = pt.accumulator()
    pt.render(spp=spp, bounces=4, seed=1)
    pt.render_gbuffer()
    hit = pt.gbuffer("object") >= 0
    return pt, keep, ref, pt.accumulator(), hit


def _score(pt, ref, noisy, hit, **kw):
    pt.denoise(gbuffer=False, **kw)
    den = pt.denoised()

    def tm(x):
        return (x[..., :3] / (1.0 + x[..., :3]))[hit].astype(np.float64)

    mse_noisy = float(np.mean((tm(noisy) - tm(ref)) ** 2))
    mse_den = float(np.mean((tm(den) - tm(ref)) ** 2))

    def lin(x):
        return float(np.mean(x[..., :3][hit], dtype=np.float64))

    return {"mse_noisy": mse_noisy, "mse_denoised": mse_den, "mse_ratio": round(mse_den / mse_noisy, 4),
            "mean_shift": round(abs(lin(den) / lin(noisy) - 1), 5),
            "tone_mapped_mean_shift": round(abs(float(np.mean(tm(den))) / float(np.mean(tm(noisy))) - 1), 5)}


def quality(srt, a, grid):
    w, h = 320, 180
    for scene in ("Scene1", "Scene_indirect"):
        pt, keep, ref, noisy, hit = _frames(srt, scene, w, h, 4, 1024)
        for kw in grid:
            line = {"tool": "denoise_time", "mode": a.mode, "scene": scene, "width": w, "height": h, "spp": 4, "ref_spp": 1024}
            line.update(kw)
            line.update(_score(pt, ref, noisy, hit, **kw))
            print(json.dumps(line), flush=True)
        pt.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["time", "quality", "sweep"])
    ap.add_argument("--scene", default="Scene1")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--max-levels", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    srt = importlib.import_module("software-raytracer_amd")
    if a.mode == "time":
        time_levels(srt, a)
    elif a.mode == "quality":
        quality(srt, a, [{}])
    else:
        grid = [dict(iterations=it, sigma_normal=sn, sigma_plane=sx, sigma_color=sc)
                for it, sn, sx, sc in itertools.product([4, 5], [0.0, 32.0, 128.0], [0.0, 0.01, 0.02, 0.05], [0.0, 2.0])]
        quality(srt, a, grid)


if __name__ == "__main__":
    main()
