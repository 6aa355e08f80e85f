#!/usr/bin/env python3
"""Time and counted work of the any-hit queries (srt_trace_occlusion) next to srt_trace_rays(OCCLUDED) on an MI355X — JSON lines.

For each scene — Scene1, BASELINE config 4's (Scene1 with its big ball as a 224 x 224 lat-long sphere, 99,904 triangles) and
Scene_indirect — two ray sets of --rays (default 2^20) rays whose origins are the first hits of a 1024 x 1024 G-buffer pass
(SRT_GBUF_POSITION lifted 1e-4 along the normal; pixels that miss keep the origin (0, 0, 0)):

    shadow       every ray points at the default environment's sun, t_max = +inf
    hemisphere   a uniformly random direction of the hemisphere around the normal, t_max = 1 (ambient occlusion)

The tracer is bound to a torch stream, rays and the output to torch tensors; after --warmup launches of each kind, each of
--launches launches is bracketed by two events on that stream, the two calls alternating, and the median is reported.  The
work counts are those of one further srt_trace_occlusion with SRT_OCCLUSION_COUNT_WORK; both calls' outputs are compared.

    python tools/occlusion_time.py --out profiles/rays/occlusion_time.jsonl

The lines go to stdout, or are appended to --out FILE.  GPU box only."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rays_time as R  # noqa: E402  (load_scene's mesh variant, timed)

SCENES = {"Scene1": ("Scene1", None), "config4_mesh224": ("Scene1", (224, 224)), "Scene_indirect": ("Scene_indirect", None)}


def load_scene(srt, base, mesh):
    if base == "Scene1":
        return R.load_scene(srt, mesh)
    return srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", base + ".json"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    srt = importlib.import_module("software-raytracer_amd")
    side = 1024
    n = a.rays
    assert 1 <= n <= side * side, "--rays: at most %d (one ray per pixel of the G-buffer pass)" % (side * side)
    lines = []
    for name in a.scenes.split(","):
        base_scene, mesh = SCENES[name]
        scene = load_scene(srt, base_scene, mesh)
        objs, cnt = scene.objects_copy()
        pt = srt.PathTracer(side, side)
        if mesh is not None:
            marr, mn = scene.meshes()
            pt.set_meshes(C.cast(marr, C.POINTER(srt.Mesh)), mn)
        pt.set_scene(objs, cnt)
        pt.set_camera(srt.default_camera())
        stream = torch.cuda.Stream(device=0)
        pos = torch.zeros((side, side, 4), dtype=torch.float32, device="cuda:0")
        nd = torch.zeros((side, side, 4), dtype=torch.float32, device="cuda:0")
        out = torch.empty((n,), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        pt.set_stream(stream.cuda_stream)
        pt.bind_gbuffer("position", pos)
        pt.bind_gbuffer("normal_depth", nd)
        pt.render_gbuffer(outputs=["position", "normal_depth"])
        stream.synchronize()
        p, nrm = pos.view(-1, 4)[:n], nd.view(-1, 4)[:n, :3]
        origins = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
        origins[:, :3] = p[:, :3] + nrm * 1e-4
        g = torch.Generator(device="cuda:0")
        g.manual_seed(3)
        sun = torch.tensor([-1.0, 1.0, 1.0], device="cuda:0")
        shadow = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
        shadow[:, :3], shadow[:, 3] = sun / sun.norm(), float("inf")
        v = torch.randn((n, 3), generator=g, device="cuda:0")
        v = v / v.norm(dim=1, keepdim=True)
        v = torch.where(((v * nrm).sum(dim=1, keepdim=True) < 0), -v, v)
        hemi = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
        hemi[:, :3], hemi[:, 3] = v, 1.0
        torch.cuda.synchronize()
        pt.bind_ray_output("occluded", out)
        info = {"tool": "occlusion_time", "device": torch.cuda.get_device_name(0), "scene": name, "rays": n, "launches": a.launches, "warmup": a.warmup,
                "first_hit_rays": int((p[:, 3] == 1.0).sum())}
        for set_name, dirs in (("shadow", shadow), ("hemisphere", hemi)):
            pt.bind_rays(origins, dirs)
            t = R.timed(torch, stream, a.launches, a.warmup, {"closest": lambda: pt.trace_rays(outputs="occluded"), "any_hit": lambda: pt.trace_occlusion()})
            pt.trace_rays(outputs="occluded")
            stream.synchronize()
            closest = out.clone()
            pt.trace_occlusion(count_work=True)
            stream.synchronize()
            work = pt.occlusion_work()
            lines.append(dict(info, ray_set=set_name, t_max="inf" if set_name == "shadow" else 1.0,
                              closest_median_ms=t["closest"]["median_ms"], closest_min_ms=t["closest"]["min_ms"],
                              any_hit_median_ms=t["any_hit"]["median_ms"], any_hit_min_ms=t["any_hit"]["min_ms"],
                              any_hit_to_closest=round(t["any_hit"]["median_ms"] / t["closest"]["median_ms"], 3),
                              outputs_equal=bool(torch.equal(closest, out)), work=work))
        pt.wait()
        pt.bind_rays(None, None)
        pt.bind_ray_output("occluded", None)
        pt.bind_gbuffer("position", None)
        pt.bind_gbuffer("normal_depth", None)
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
