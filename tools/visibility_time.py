#!/usr/bin/env python3
"""Time of the per-pixel visibility pass (srt_render_visibility) on an MI355X next to the same segments sent through
srt_write_rays + srt_trace_occlusion — JSON lines.

Scene1 at --width x --height (default 1920 x 1080), the default camera and environment, ambient occlusion with n = --samples
(default 1, 4, 16) segments of unbounded length per pixel plus the sun segment.  Per n:

    fused        srt_render_visibility(AO | SUN) from the G-buffer that is already on the device: --launches launches after
                 --warmup, each bracketed by two events on the tracer's stream; median / min / max
    round_trip   what a caller had to do before: the segments are built on the host from the read-back guides
                 (tests/visibility_reference.py, the numpy form of the header's rules; not timed), then srt_write_rays (the
                 upload of 32 B per segment), srt_trace_occlusion, srt_read_ray_output and the reduction, timed on the host
                 clock as one unit; and the srt_trace_occlusion launches alone by events, as `fused`

The two answers are compared bit for bit and the work counts of one further counting call are recorded.

    python tools/visibility_time.py --out profiles/visibility/visibility_time.jsonl

The lines go to stdout, or are appended to --out FILE.  GPU box only."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rays_time as R  # noqa: E402  (load_scene, timed)
import visibility_reference as VR  # noqa: E402  (the segments in numpy binary32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samples", default="1,4,16")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    srt = importlib.import_module("software-raytracer_amd")
    w, h = a.width, a.height
    scene = R.load_scene(srt, None)
    objs, cnt = scene.objects_copy()
    pt = srt.PathTracer(w, h)
    pt.set_scene(objs, cnt)
    pt.set_camera(srt.default_camera())
    stream = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    pt.set_stream(stream.cuda_stream)
    pt.render_gbuffer(outputs=["object", "normal_depth", "position"])
    obj, nd, pos = pt.gbuffer("object"), pt.gbuffer("normal_depth"), pt.gbuffer("position")
    sun_direction = [float(v) for v in srt.default_environment().sun_direction]
    info = {"tool": "visibility_time", "device": torch.cuda.get_device_name(0), "scene": "Scene1", "width": w, "height": h, "launches": a.launches,
            "warmup": a.warmup, "hit_pixels": int((obj != -1).sum())}
    lines = []
    for n in [int(x) for x in a.samples.split(",")]:
        fused = R.timed(torch, stream, a.launches, a.warmup, {"fused": lambda: pt.render_visibility(n)})["fused"]
        pt.render_visibility(n, count_work=True)
        ao, sun, work = pt.visibility("ao"), pt.visibility("sun"), pt.visibility_work()
        # the same segments by the caller's route: AO segments pixel-major, then the sun segments
        pix, O4, D4 = VR.ao_segments(obj, nd, pos, n)
        spix, c, lit, SO4, SD4 = VR.sun_segments(obj, nd, pos, sun_direction)
        origins, directions = np.concatenate([O4, SO4]), np.concatenate([D4, SD4])
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            pt.write_rays(origins, directions)
            pt.trace_occlusion()
            occ = pt.ray_output("occluded")
            ao2 = VR.ao_image(obj, pix, occ[:len(O4)], n)
            sun2 = VR.sun_image(obj, spix, c, lit, occ[len(O4):])
            walls.append((time.perf_counter() - t0) * 1e3)
        trace = R.timed(torch, stream, a.launches, a.warmup, {"any_hit": lambda: pt.trace_occlusion()})["any_hit"]
        lines.append(dict(info, ao_samples=n, segments=int(len(origins)), ray_bytes=int(origins.nbytes + directions.nbytes),
                          fused_median_ms=fused["median_ms"], fused_min_ms=fused["min_ms"], fused_max_ms=fused["max_ms"],
                          round_trip_wall_ms=round(min(walls), 3), trace_occlusion_median_ms=trace["median_ms"], trace_occlusion_min_ms=trace["min_ms"],
                          fused_to_trace_occlusion=round(fused["median_ms"] / trace["median_ms"], 3),
                          outputs_equal=bool(np.array_equal(ao.view(np.uint32), ao2.view(np.uint32)) and np.array_equal(sun.view(np.uint32), sun2.view(np.uint32))),
                          work=work))
    pt.wait()
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
