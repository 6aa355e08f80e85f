#!/usr/bin/env python3
"""Kernel time of the first-hit buffers (srt_render_gbuffer) on an MI355X — one JSON line.

The tracer is bound to a torch stream (srt_set_stream) and its outputs to torch tensors (srt_bind_gbuffer); after
--warmup launches, each of --launches launches is bracketed by two events on that stream and the median of their
times is reported.  Next to it: `render_kernel_ms`, the median srt_stats.kernel_ms of a 1-spp, 8-bounce srt_render
of the same frame (one sample-frame of the path tracer), for scale.

    python tools/gbuffer_time.py --scene Scene1 --width 1920 --height 1080 --outputs all
    python tools/gbuffer_time.py --scene Scene1 --width 3840 --height 2160 --outputs object

GPU box only (profiles/gbuffer/ holds the committed lines).
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="Scene1")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--outputs", default="all", help="all, or a comma-separated list of object,normal_depth,position,albedo")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import torch

    srt = importlib.import_module("software-raytracer_amd")
    names = list(srt.capi.GBUFFERS) if a.outputs == "all" else a.outputs.split(",")
    mask = srt.capi.gbuffer_outputs(names)
    w, h = a.width, a.height
    scene = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", a.scene + ".json"))
    objs, n = scene.objects_copy()
    pt = srt.PathTracer(w, h)
    pt.set_scene(objs, n)
    pt.set_camera(srt.default_camera())
    stream = torch.cuda.Stream(device=0)
    pt.set_stream(stream.cuda_stream)
    bufs = {}
    for k in names:
        _, dtype, ch = srt.capi.GBUFFERS[k]
        shape = (h, w) if ch == 1 else (h, w, ch)
        bufs[k] = torch.empty(shape, dtype=torch.int32 if ch == 1 else torch.float32, device="cuda:0")
        pt.bind_gbuffer(k, bufs[k])
    for _ in range(a.warmup):
        pt.render_gbuffer(outputs=mask)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
    for b, e in ev:
        b.record(stream)
        pt.render_gbuffer(outputs=mask)
        e.record(stream)
    stream.synchronize()
    ms = [b.elapsed_time(e) for b, e in ev]
    # one sample-frame of the path tracer on the same frame, for scale (its own events: srt_stats.kernel_ms)
    render_ms = []
    for i in range(2 + 5):
        pt.render(spp=1, bounces=8, seed=0, reset=True)
        if i >= 2:
            render_ms.append(pt.stats().kernel_ms)
    hits = int((pt.gbuffer("object") >= 0).sum()) if "object" in names else None
    bytes_px = sum(4 if srt.capi.GBUFFERS[k][2] == 1 else 16 for k in names)
    med = statistics.median(ms)
    print(json.dumps({
        "tool": "gbuffer_time", "device": torch.cuda.get_device_name(0), "scene": a.scene, "width": w, "height": h,
        "outputs": names, "launches": a.launches, "warmup": a.warmup,
        "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
        "render_kernel_ms": round(statistics.median(render_ms), 4), "render": "srt_render 1 spp, 8 bounces, same frame (median of 5)",
        "bytes_per_pixel": bytes_px, "store_gbs": round(bytes_px * w * h / (med * 1e-3) / 1e9, 1),
        "mrays_per_s": round(w * h / (med * 1e-3) / 1e6, 1), "hit_pixels": hits,
    }))
    for k in names:
        pt.bind_gbuffer(k, None)
    pt.set_stream(0)
    pt.close()


if __name__ == "__main__":
    main()
