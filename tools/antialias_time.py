#!/usr/bin/env python3
"""Kernel times and the quality figure of the anti-aliasing passes (srt_render_subsamples, srt_antialias) on an MI355X — JSON lines.

    python tools/antialias_time.py time [--out profiles/antialias/antialias_time.jsonl]
    python tools/antialias_time.py quality [--out profiles/antialias/antialias_quality.jsonl]

time: Scene1 at 1080p and 4K, rendered at 1 spp with its OBJECT guide made once; the tracer runs on a torch stream
(srt_set_stream).  For k = 2, 3 and 4, after --warmup calls each of --launches calls of srt_render_subsamples and of srt_antialias
(with and without SRT_AA_FRAMEBUFFER) is bracketed by two events on that stream; median, minimum and maximum are reported.  The
OBJECT-only srt_render_gbuffer pass is timed the same way in the same run, so that the sub-sample pass reads as a multiple of it.
quality: Scene1 at 96 x 54, k = 4, 64 spp, 4 bounces.  The ground truth of pixel (x, y) is the mean of the 16 accumulator pixels
(2k x + 2i - (k-1), 2k y + 2j - (k-1)) of a 768 x 432 render with the same camera and spp and another seed — the pixels whose
rays ARE the sub-samples' rays; border pixels with a negative coordinate are left out.  The figure is the mean squared error of
c / (1 + c) over the pixels that have a foreign sub-sample, for the raw and for the anti-aliased frame.

GPU box only (profiles/antialias/ holds the committed lines).
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


def _tracer(srt, scene, w, h):
    objs, n = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", scene + ".json")).objects_copy()
    pt = srt.PathTracer(w, h)
    pt.set_scene(objs, n)
    pt.set_camera(srt.default_camera())
    return pt, objs


def _bracket(torch, stream, call, launches, warmup):
    for _ in range(warmup):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for b, e in ev:
        b.record(stream)
        call()
        e.record(stream)
    stream.synchronize()
    return [b.elapsed_time(e) for b, e in ev]


def _ms(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def time_calls(srt, a, emit):
    import torch

    stream = torch.cuda.Stream(device=0)
    for w, h in ((1920, 1080), (3840, 2160)):
        pt, keep = _tracer(srt, a.scene, w, h)
        pt.set_stream(stream.cuda_stream)
        base = dict(tool="antialias_time", mode="time", device=torch.cuda.get_device_name(0), scene=a.scene, width=w, height=h,
                    launches=a.launches, warmup=a.warmup)
        pt.render(spp=1, bounces=8, seed=0)
        ms = _bracket(torch, stream, lambda: pt.render_gbuffer(outputs=srt.capi.GBUF_OBJECT), a.launches, a.warmup)
        t_obj = statistics.median(ms)
        emit(dict(base, call="srt_render_gbuffer", outputs="object", **_ms(ms)))
        for k in (2, 3, 4):
            ms = _bracket(torch, stream, lambda: pt.render_subsamples(k), a.launches, a.warmup)
            emit(dict(base, call="srt_render_subsamples", k=k, **_ms(ms), over_object_gbuffer=round(statistics.median(ms) / t_obj, 3)))
            for fb in (False, True):
                ms = _bracket(torch, stream, lambda: pt.antialias(k, framebuffer=fb, guides=False), a.launches, a.warmup)
                # compulsory traffic of an interior pixel: K plane values and the object 4 B each, the colour read and written
                bpp = 4 * (k * k + 1) + 32 + (4 if fb else 0)
                emit(dict(base, call="srt_antialias", k=k, framebuffer=fb, **_ms(ms), compulsory_bytes_per_pixel=bpp,
                          compulsory_gbs=round(w * h * bpp / (statistics.median(ms) * 1e-3) / 1e9, 1)))
        pt.set_stream(0)
        pt.close()


def tone(v):
    v = np.asarray(v)[..., :3].astype(np.float64)
    return v / (1.0 + v)


def quality_figures(srt, scene="Scene1", w=96, h=54, k=4, spp=64, bounces=4, seed=1, truth_seed=2):
    """The procedure of the module text.  Returns a dict: the edge pixels counted, the summed and the mean squared error of the
    raw and of the anti-aliased frame over them, and the number of pixels the pass changed."""
    big, keep_big = _tracer(srt, scene, 2 * k * w, 2 * k * h)
    big.render(spp=spp, bounces=bounces, seed=truth_seed)
    hi = big.accumulator()
    big.close()
    pt, keep = _tracer(srt, scene, w, h)
    pt.render(spp=spp, bounces=bounces, seed=seed)
    raw = pt.accumulator()
    pt.antialias(k)
    aa = pt.antialiased()
    obj, sub = pt.gbuffer("object"), pt.subsamples()
    pt.close()
    truth = np.zeros((h, w, 3))
    xs, ys = np.arange(1, w), np.arange(1, h)  # (x = 0 and y = 0 have sub-samples left of / below the big frame)
    for j in range(k):
        for i in range(k):
            X, Y = 2 * k * xs + 2 * i - (k - 1), 2 * k * ys + 2 * j - (k - 1)
            truth[1:, 1:] += hi[np.ix_(Y, X)][..., :3].astype(np.float64)
    truth /= k * k
    edge = (sub != obj[None]).any(axis=0)
    edge[0, :] = edge[:, 0] = False
    t = truth / (1.0 + truth)
    e_raw, e_aa = ((tone(raw) - t) ** 2)[edge], ((tone(aa) - t) ** 2)[edge]
    changed = int((np.ascontiguousarray(raw).view(np.uint32) != np.ascontiguousarray(aa).view(np.uint32)).any(axis=2).sum())
    return dict(scene=scene, width=w, height=h, k=k, spp=spp, bounces=bounces, seed=seed, truth_seed=truth_seed,
                edge_pixels=int(edge.sum()), changed_pixels=changed, sse_raw=float(e_raw.sum()), sse_antialiased=float(e_aa.sum()),
                mse_raw=float(e_raw.mean()), mse_antialiased=float(e_aa.mean()))


def quality(srt, a, emit):
    q = quality_figures(srt, a.scene)
    emit(dict(tool="antialias_time", mode="quality", **q, ratio=round(q["mse_antialiased"] / q["mse_raw"], 4)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["time", "quality"])
    ap.add_argument("--scene", default="Scene1")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", help="also append the lines to this file (e.g. profiles/antialias/antialias_time.jsonl)")
    a = ap.parse_args()
    srt = importlib.import_module("software-raytracer_amd")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")

    {"time": time_calls, "quality": quality}[a.mode](srt, a, emit)


if __name__ == "__main__":
    main()
