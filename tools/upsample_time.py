#!/usr/bin/env python3
"""Kernel time and reconstruction quality of the guided upsampler (srt_upsample) on an MI355X — JSON lines.

    python tools/upsample_time.py time      # median time of one call at 1080p and 4K, steps 2 and 8, next to srt_temporal_accumulate
    python tools/upsample_time.py quality   # the figures of tests/test_gpu_upsample.py (defaults)
    python tools/upsample_time.py e2e       # Scene1 1080p, 8 bounces: render at steps 2 + guides + upsample against render at steps 1
    python tools/upsample_time.py sweep     # the small sweep of the two sigmas that chose the defaults

time: Scene1 rendered at 1 spp in steps x steps blocks with its first-hit guides made once; the tracer runs on a torch stream
(srt_set_stream); after --warmup calls each of --launches calls is bracketed by two events on that stream and the median is
reported, with the compulsory bytes per pixel.  srt_temporal_accumulate — also one pass with a 2 x 2 gather over the same
guides — is timed the same way in the same run (after its warm-up the history is valid, so every tap is tested): the yardstick.
quality: Scene1 and Scene_indirect at 320 x 180.  Preview shader (no RNG, so the steps = 1 frame is the exact truth) at steps
2, 4 and 8, and the path-traced branch (64 spp, 4 bounces, same seed) at steps 2: MSE of the tone-mapped values c / (1 + c)
against the steps = 1 frame, block image and upsampled image, over all pixels and over those within `steps` of an
object-index edge.
e2e: --spp samples per pixel (default 4) both ways, the three calls of the reconstruction bracketed together; the error of
either frame is its tone-mapped MSE against a 1024-spp steps = 1 frame of another seed.
sweep: the e2e frame (steps 2) and the 1080p preview (steps 2 and 8) for a grid of sigma_normal x sigma_plane.

GPU box only (profiles/upsample/ holds the committed lines).
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

# compulsory traffic per pixel: object 4 B, normal / depth, point and the pixel's own accumulator value 16 B each read, 16 B
# result written; the four anchors' 52 B each are shared by the steps^2 pixels of a block
BYTES_PER_PIXEL = 4 + 16 * 3 + 16


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


def time_calls(srt, a):
    import torch

    stream = torch.cuda.Stream(device=0)
    for w, h in ((1920, 1080), (3840, 2160)):
        pt, keep = _tracer(srt, a.scene, w, h)
        pt.set_stream(stream.cuda_stream)
        base = dict(tool="upsample_time", mode="time", device=torch.cuda.get_device_name(0), scene=a.scene, width=w, height=h,
                    launches=a.launches, warmup=a.warmup)
        med = {}
        for steps in (2, 8):
            pt.render(spp=1, bounces=8, seed=0, steps=steps)
            pt.render_gbuffer(outputs=srt.capi.UPSAMPLE_GUIDES)
            for fb in (False, True):
                ms = _bracket(torch, stream, lambda: pt.upsample(steps=steps, framebuffer=fb, gbuffer=False), a.launches, a.warmup)
                bpp = BYTES_PER_PIXEL + (4 if fb else 0)
                line = dict(base, call="srt_upsample", steps=steps, framebuffer=fb, **_ms(ms), compulsory_bytes_per_pixel=bpp,
                            compulsory_gbs=round(w * h * bpp / (statistics.median(ms) * 1e-3) / 1e9, 1))
                med[(steps, fb)] = statistics.median(ms)
                print(json.dumps(line), flush=True)
        pt.render(spp=1, bounces=8, seed=0)
        pt.render_gbuffer(outputs=srt.capi.TEMPORAL_GUIDES)
        for fb in (False, True):
            ms = _bracket(torch, stream, lambda: pt.temporal(samples=1, framebuffer=fb, gbuffer=False), a.launches, a.warmup)
            t = statistics.median(ms)
            print(json.dumps(dict(base, call="srt_temporal_accumulate", framebuffer=fb, **_ms(ms),
                                  upsample_over_temporal={"steps%d" % s: round(med[(s, fb)] / t, 3) for s in (2, 8)})), flush=True)
        pt.set_stream(0)
        pt.close()


def _near_edges(obj, reach):
    # (as tests/test_gpu_upsample.py)
    edge = np.zeros(obj.shape, bool)
    edge[:, 1:] |= obj[:, 1:] != obj[:, :-1]
    edge[:, :-1] |= obj[:, 1:] != obj[:, :-1]
    edge[1:, :] |= obj[1:, :] != obj[:-1, :]
    edge[:-1, :] |= obj[1:, :] != obj[:-1, :]
    for axis, n in ((0, obj.shape[0]), (1, obj.shape[1])):
        grown = edge.copy()
        for s in range(1, reach + 1):
            i, j = [slice(None)] * 2, [slice(None)] * 2
            i[axis], j[axis] = slice(s, n), slice(0, n - s)
            grown[tuple(i)] |= edge[tuple(j)]
            grown[tuple(j)] |= edge[tuple(i)]
        edge = grown
    return edge


def _mse(x, ref, mask=None):
    tm = lambda v: v[..., :3].astype(np.float64) / (1.0 + v[..., :3].astype(np.float64))  # noqa: E731
    d = (tm(x) - tm(ref)) ** 2
    return float(np.mean(d if mask is None else d[mask]))


def quality(srt, a):
    w, h = 320, 180
    for scene in ("Scene1", "Scene_indirect"):
        pt, keep = _tracer(srt, scene, w, h)
        pt.render_gbuffer()
        obj = pt.gbuffer("object")
        for branch, kw, all_steps in (("preview", dict(spp=1, preview=True), (2, 4, 8)), ("path traced", dict(spp=64, bounces=4, seed=21), (2,))):
            pt.render(**kw)
            truth = pt.accumulator()
            for steps in all_steps:
                pt.render(steps=steps, **kw)
                blocks = pt.accumulator()
                pt.upsample(steps=steps, gbuffer=False)
                up = pt.upsampled()
                edges = _near_edges(obj, steps)
                line = dict(tool="upsample_time", mode="quality", scene=scene, width=w, height=h, branch=branch, steps=steps,
                            spp=kw["spp"], edge_pixels=int(edges.sum()), **{k: v for k, v in srt.capi.upsample_defaults().items() if k.startswith("sigma")})
                for what, mask in (("all", None), ("edges", edges)):
                    mb, mu = _mse(blocks, truth, mask), _mse(up, truth, mask)
                    line.update({"mse_blocks_" + what: mb, "mse_upsampled_" + what: mu, "ratio_" + what: round(mu / mb, 4)})
                print(json.dumps(line), flush=True)
        pt.close()


def _e2e_tracer(srt, a, torch):
    w, h = 1920, 1080
    pt, keep = _tracer(srt, "Scene1", w, h)
    pt.render(spp=1024, bounces=8, seed=777)
    ref = pt.accumulator()
    return pt, keep, ref, w, h


def e2e(srt, a):
    import torch

    pt, keep, ref, w, h = _e2e_tracer(srt, a, torch)
    stream = torch.cuda.Stream(device=0)
    pt.set_stream(stream.cuda_stream)

    def full():
        pt.render(spp=a.spp, bounces=8, seed=1)

    def rebuilt():
        pt.render(spp=a.spp, bounces=8, seed=1, steps=2)
        pt.render_gbuffer(outputs=srt.capi.UPSAMPLE_GUIDES)
        pt.upsample(steps=2, gbuffer=False)

    t_full = _bracket(torch, stream, full, a.launches, a.warmup)
    full_img = pt.accumulator()
    t_reb = _bracket(torch, stream, rebuilt, a.launches, a.warmup)
    blocks, up = pt.accumulator(), pt.upsampled()
    print(json.dumps(dict(tool="upsample_time", mode="e2e", device=torch.cuda.get_device_name(0), scene="Scene1", width=w, height=h,
                          bounces=8, spp=a.spp, ref_spp=1024, launches=a.launches, warmup=a.warmup,
                          render_steps1_ms=_ms(t_full), render_steps2_gbuffer_upsample_ms=_ms(t_reb),
                          time_ratio=round(statistics.median(t_reb) / statistics.median(t_full), 4),
                          mse_steps1=_mse(full_img, ref), mse_steps2_blocks=_mse(blocks, ref), mse_steps2_upsampled=_mse(up, ref),
                          **{k: v for k, v in srt.capi.upsample_defaults().items() if k.startswith("sigma")})), flush=True)
    pt.set_stream(0)
    pt.close()


def sweep(srt, a):
    import torch

    pt, keep, ref, w, h = _e2e_tracer(srt, a, torch)
    grid = list(itertools.product([0.0, 8.0, 32.0, 128.0], [0.0, 0.005, 0.02, 0.1]))
    pt.render_gbuffer(outputs=srt.capi.UPSAMPLE_GUIDES)
    obj = pt.gbuffer("object")
    cases = [("path traced", dict(spp=a.spp, bounces=8, seed=1), 2, ref)]
    pt.render(spp=1, preview=True)
    truth = pt.accumulator()
    cases += [("preview", dict(spp=1, preview=True), s, truth) for s in (2, 8)]
    for branch, kw, steps, target in cases:
        pt.render(steps=steps, **kw)
        edges = _near_edges(obj, steps)
        for sn, sx in grid:
            pt.upsample(steps=steps, sigma_normal=sn, sigma_plane=sx, gbuffer=False)
            up = pt.upsampled()
            print(json.dumps(dict(tool="upsample_time", mode="sweep", scene="Scene1", width=w, height=h, branch=branch, steps=steps,
                                  spp=kw["spp"], sigma_normal=sn, sigma_plane=sx, mse_all=_mse(up, target),
                                  mse_edges=_mse(up, target, edges))), flush=True)
    pt.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["time", "quality", "e2e", "sweep"])
    ap.add_argument("--scene", default="Scene1")
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    srt = importlib.import_module("software-raytracer_amd")
    {"time": time_calls, "quality": quality, "e2e": e2e, "sweep": sweep}[a.mode](srt, a)


if __name__ == "__main__":
    main()
