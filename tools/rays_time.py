#!/usr/bin/env python3
"""Time of the ray queries (srt_trace_rays) on an MI355X — JSON lines.

For each scene — Scene1, and BASELINE config 4's (Scene1 with its big ball as a 224 x 224 lat-long sphere, 99,904 triangles) —
two batches:

    coherent     the camera rays of a --width x --height frame in pixel order (GetRayDirection's arithmetic in torch float32),
                 traced with OBJECT | NORMAL_DEPTH and with all five outputs, next to srt_render_gbuffer (OBJECT | NORMAL_DEPTH)
                 of the same frame in the same process, the launches of the three alternating
    incoherent   --random (default 2^21) rays with origins uniform in a box around the scene and uniformly random directions,
                 all five outputs

The tracer is bound to a torch stream (srt_set_stream), rays and outputs to torch tensors (srt_bind_rays, srt_bind_ray_output,
srt_bind_gbuffer); after --warmup launches of each kind, each of --launches launches is bracketed by two events on that stream
and the median of their times is reported.

    python tools/rays_time.py --out profiles/rays/rays_time.jsonl

The lines go to stdout, or are appended to --out FILE.  GPU box only."""
import argparse
import ctypes as C
import importlib
import json
import math
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MESH_OBJECT = 64  # Scene1's big ball (r = 1)
SCENES = {"Scene1": None, "config4_mesh224": (224, 224)}
ELEM_BYTES = {"object": 4, "normal_depth": 16, "position": 16, "albedo": 16, "occluded": 4}


def load_scene(srt, mesh):
    path = os.path.join(ROOT, "software-raytracer_amd", "scenes", "Scene1.json")
    if mesh is None:
        return srt.host.Scene(path)
    doc = json.load(open(path))
    doc["SceneObjects"][MESH_OBJECT]["Renderer"] = {"Type": "Mesh", "Primitive": "UVSphere", "Radius": 1.0, "Stacks": mesh[0], "Slices": mesh[1]}
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(doc, f)
    try:
        scene = srt.host.Scene(f.name)
    finally:
        os.unlink(f.name)
    assert scene.error == "", scene.error
    return scene


def camera_rays(torch, w, h, fov=55.0):
    """The rays of the default camera (origin, identity basis) in pixel order x + y * w, GetRayDirection's arithmetic in float32."""
    clip = 0.01
    ld = clip * math.tan(math.radians(fov) / 2.0)
    rd = ld * (w / h)
    xs = torch.arange(w, dtype=torch.float32, device="cuda:0") / w * 2 - 1
    ys = torch.arange(h, dtype=torch.float32, device="cuda:0") / h * 2 - 1
    d = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
    d[..., 0] = (xs * rd)[None, :]
    d[..., 1] = (ys * ld)[:, None]
    d[..., 2] = clip
    d[..., :3] /= torch.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])[..., None]
    d[..., 3] = float("inf")
    return torch.zeros((w * h, 4), dtype=torch.float32, device="cuda:0"), d.reshape(-1, 4).contiguous()


def random_rays(torch, n, seed):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    lo = torch.tensor([-5.0, -1.0, 0.0], device="cuda:0")
    hi = torch.tensor([5.0, 4.0, 10.0], device="cuda:0")
    o = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
    o[:, :3] = lo + (hi - lo) * torch.rand((n, 3), generator=g, device="cuda:0")
    d = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
    v = torch.randn((n, 3), generator=g, device="cuda:0")
    d[:, :3] = v / torch.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])[:, None]
    d[:, 3] = float("inf")
    return o, d


def timed(torch, stream, launches, warmup, calls):
    """Median / min / max event time of each call in `calls` (name -> function), the calls alternating launch by launch."""
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    ev = {k: [] for k in calls}
    for _ in range(launches):
        for k, fn in calls.items():
            b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b.record(stream)
            fn()
            e.record(stream)
            ev[k].append((b, e))
    stream.synchronize()
    out = {}
    for k, pairs in ev.items():
        ms = [b.elapsed_time(e) for b, e in pairs]
        out[k] = {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--random", type=int, default=1 << 21)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    srt = importlib.import_module("software-raytracer_amd")
    c = srt.capi
    w, h = a.width, a.height
    lines = []
    for name in a.scenes.split(","):
        scene = load_scene(srt, SCENES[name])
        objs, n = scene.objects_copy()
        pt = srt.PathTracer(w, h)
        if SCENES[name] is not None:
            marr, mn = scene.meshes()
            pt.set_meshes(C.cast(marr, C.POINTER(srt.Mesh)), mn)
        pt.set_scene(objs, n)
        pt.set_camera(srt.default_camera())
        stream = torch.cuda.Stream(device=0)
        big = max(w * h, a.random)
        out = {k: torch.empty((big,) if ELEM_BYTES[k] == 4 else (big, 4), dtype=torch.int32 if ELEM_BYTES[k] == 4 else torch.float32, device="cuda:0")
               for k in ELEM_BYTES}
        gb = {"object": torch.empty((h, w), dtype=torch.int32, device="cuda:0"), "normal_depth": torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")}
        co, cd = camera_rays(torch, w, h)
        ro, rdir = random_rays(torch, a.random, 1)
        torch.cuda.synchronize()
        pt.set_stream(stream.cuda_stream)
        for k in out:
            pt.bind_ray_output(k, out[k])
        for k in gb:
            pt.bind_gbuffer(k, gb[k])
        two = c.GBUF_OBJECT | c.GBUF_NORMAL_DEPTH
        base = {"tool": "rays_time", "device": torch.cuda.get_device_name(0), "scene": name, "launches": a.launches, "warmup": a.warmup}
        # coherent: the frame's camera rays next to the G-buffer pass
        pt.bind_rays(co, cd)
        t = timed(torch, stream, a.launches, a.warmup, {"gbuffer": lambda: pt.render_gbuffer(outputs=two), "trace_two": lambda: pt.trace_rays(outputs=two),
                                                        "trace_all": lambda: pt.trace_rays(outputs=c.RAYS_ALL)})
        same = bool(torch.equal(out["object"][:w * h].view(h, w), gb["object"]))
        hits = int((out["object"][:w * h] >= 0).sum())
        for key, outs in (("trace_two", ["object", "normal_depth"]), ("trace_all", list(ELEM_BYTES))):
            med = t[key]["median_ms"]
            lines.append(dict(base, batch="coherent", rays=w * h, width=w, height=h, outputs=outs, **t[key],
                              gbuffer_median_ms=t["gbuffer"]["median_ms"], ratio_to_gbuffer=round(med / t["gbuffer"]["median_ms"], 3),
                              bytes_per_ray=32 + sum(ELEM_BYTES[k] for k in outs), mrays_per_s=round(w * h / (med * 1e-3) / 1e6, 1),
                              hit_rays=hits, object_equals_gbuffer=same))
        # incoherent: random rays
        pt.bind_rays(ro, rdir)
        t = timed(torch, stream, a.launches, a.warmup, {"trace_all": lambda: pt.trace_rays(outputs=c.RAYS_ALL)})
        med = t["trace_all"]["median_ms"]
        lines.append(dict(base, batch="incoherent", rays=a.random, outputs=list(ELEM_BYTES), **t["trace_all"], bytes_per_ray=32 + sum(ELEM_BYTES.values()),
                          mrays_per_s=round(a.random / (med * 1e-3) / 1e6, 1), hit_rays=int((out["object"][:a.random] >= 0).sum())))
        pt.wait()
        pt.bind_rays(None, None)
        for k in out:
            pt.bind_ray_output(k, None)
        for k in gb:
            pt.bind_gbuffer(k, None)
        pt.set_stream(0)
        pt.close()
    text = "".join(json.dumps(line) + "\n" for line in lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
