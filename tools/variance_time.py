#!/usr/bin/env python3
"""Kernel time and quality of the variance estimate and the variance-guided filter (srt_variance, srt_denoise_variance) on an
MI355X — JSON lines.

    python tools/variance_time.py time [--width 1920 --height 1080]   # profiles/denoise/variance_time_1080p.jsonl
    python tools/variance_time.py quality                             # profiles/denoise/variance_quality.jsonl

time: Scene1 rendered as two halves of 1 spp and its first-hit buffers made once; the tracer is bound to a torch stream
(srt_set_stream), its guides, half, variance and result to torch tensors; after --warmup calls, each of --launches calls is
bracketed by two events on that stream and the median is reported: srt_variance without and with SRT_VARIANCE_MERGE (not
merging in the timed loop twice: the accumulator is rewritten from a copy before every merging call, outside the events),
srt_denoise_variance at the library's defaults and srt_denoise at its defaults, all in the same run.
quality: the procedure of tests/test_gpu_variance.py — Scene1 at 96 x 64, 8 bounces, two halves of 4 spp against 2048 spp of the
same library; MSE of the tone-mapped values c / (1 + c) over hit pixels of the merged mean, of srt_denoise_variance and of
srt_denoise on the merged mean, both at their defaults.

The lines go to stdout, or are appended to --out FILE.  GPU box only (profiles/denoise/ holds the committed lines).
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HALF_SEED = 0x9E3779B9


def _tracer(srt, scene, w, h):
    objs, n = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", scene + ".json")).objects_copy()
    pt = srt.PathTracer(w, h)
    pt.set_scene(objs, n)
    pt.set_camera(srt.default_camera())
    return pt, objs


def render_halves(pt, spp_half, bounces, seed):
    """Half A into the accumulator, half B (seed ^ 0x9E3779B9) into the handle's half buffer through bind_output."""
    pt.render(spp=spp_half, bounces=bounces, seed=seed)
    pt.bind_output(None, pt.half_ptr())
    pt.render(spp=spp_half, bounces=bounces, seed=seed ^ HALF_SEED)
    pt.bind_output()


def quality_figures(srt, scene="Scene1", w=96, h=64, bounces=8, spp_half=4, ref_spp=2048):
    pt, keep = _tracer(srt, scene, w, h)
    pt.render(spp=ref_spp, bounces=bounces, seed=777)
    ref = pt.accumulator()
    render_halves(pt, spp_half, bounces, 1)
    pt.render_gbuffer()
    hit = pt.gbuffer("object") >= 0
    pt.variance(gbuffer=False)  # defaults: ALBEDO | MERGE
    merged = pt.accumulator()
    var = pt.variance_map()
    pt.denoise_variance(gbuffer=False)
    dv = pt.denoised()
    pt.denoise(gbuffer=False)
    dn = pt.denoised()
    pt.close()

    def tm(x):
        return (x[..., :3] / (1.0 + x[..., :3]))[hit].astype(np.float64)

    def mse(x):
        return float(np.mean((tm(x) - tm(ref)) ** 2))

    return {"tool": "variance_time", "mode": "quality", "scene": scene, "width": w, "height": h, "bounces": bounces,
            "spp": 2 * spp_half, "ref_spp": ref_spp, "hit_pixels": int(hit.sum()), "mean_variance": float(np.mean(var[hit], dtype=np.float64)),
            "mse_merged": mse(merged), "mse_denoise_variance": mse(dv), "mse_denoise": mse(dn)}


def time_passes(srt, a):
    import torch

    w, h = a.width, a.height
    pt, keep = _tracer(srt, a.scene, w, h)
    stream = torch.cuda.Stream(device=0)
    pt.set_stream(stream.cuda_stream)
    bufs = {"object": torch.empty((h, w), dtype=torch.int32, device="cuda:0")}
    for k in ("normal_depth", "position", "albedo"):
        bufs[k] = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
    out = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
    half = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    var = torch.empty((h, w), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    for k, t in bufs.items():
        pt.bind_gbuffer(k, t)
    pt.bind_denoised(out)
    pt.bind_half(half)
    pt.bind_variance(var)
    pt.render(spp=1, bounces=8, seed=0)
    pt.bind_output(None, half.data_ptr())
    pt.render(spp=1, bounces=8, seed=HALF_SEED)
    pt.bind_output()
    pt.render_gbuffer()
    pt.wait()
    acc0 = pt.accumulator()

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

    dv, dn = srt.capi.DENOISE_VARIANCE_DEFAULTS, srt.capi.DENOISE_DEFAULTS
    head = {"tool": "variance_time", "mode": "time", "device": torch.cuda.get_device_name(0), "scene": a.scene, "width": w, "height": h,
            "launches": a.launches, "warmup": a.warmup}
    lines = []
    for merge in (False, True):
        t = timed(lambda: pt.variance(albedo=True, merge=merge, gbuffer=False), before=(lambda: pt.write_accumulator(acc0)) if merge else None)
        # compulsory traffic per pixel: two halves (32 B), object (4 B), albedo (16 B) read; 4 B written, 12 B more when merging
        t["compulsory_gbs"] = round(w * h * (32 + 4 + 16 + 4 + (12 if merge else 0)) / (t["median_ms"] * 1e-3) / 1e9, 1)
        lines.append(dict(head, **{"pass": "srt_variance", "flags": 1 | (2 if merge else 0)}, **t))
    pt.write_accumulator(acc0)
    pt.variance(albedo=True, merge=True, gbuffer=False)
    t = timed(lambda: pt.denoise_variance(gbuffer=False))
    lines.append(dict(head, **{"pass": "srt_denoise_variance"}, **dv, **t, ms_per_level=round(t["median_ms"] / dv["iterations"], 4)))
    t = timed(lambda: pt.denoise(gbuffer=False))
    lines.append(dict(head, **{"pass": "srt_denoise"}, **dn, **t, ms_per_level=round(t["median_ms"] / dn["iterations"], 4)))
    pt.bind_denoised(None)
    pt.bind_half(None)
    pt.bind_variance(None)
    for k in bufs:
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
    lines = time_passes(srt, a) if a.mode == "time" else [quality_figures(srt)]
    text = "".join(json.dumps(line) + "\n" for line in lines)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
