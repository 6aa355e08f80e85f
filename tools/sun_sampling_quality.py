#!/usr/bin/env python3
"""What sun sampling at diffuse bounces (SRT_RADIANCE_SUN_SAMPLING, SRT_LIGHT_PROBE_SUN_SAMPLING) buys in error — JSON lines, one run.

frame (per scene of --scenes, default Scene1,Scene2; --width x --height, default 480 x 270): the camera rays through
srt_trace_radiance at --samples (16) samples and 8 bounces, flag off and flag on.  Reference: srt_render at --reference (4096)
samples and 8 bounces, which has no flag: both estimators converge to it.  Error: the relative luminance RMSE
|L - ref| / (ref + 0.01) over the hit pixels.  Rows: off and on at equal samples with the median time of 5 event-timed launches;
then the flag OFF at the sample count that costs what the flag on costs (samples * t_on / t_off, at least 1) with its measured
time: the equal-time comparison.

probes (per scene): a 6 x 3 x 6 grid of probes over the scene, --directions (256) directions, ONE 16-sample frame, flag off and
on: the RMSE of the DC luminance (coefficient 0) against a 256-sample trace without the flag, relative to that reference's mean.

    python tools/sun_sampling_quality.py --out profiles/sun_sampling/sun_sampling_quality.jsonl

The lines go to stdout, or are appended to --out FILE.  GPU box only."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def lum(c):
    c = np.asarray(c, np.float64)
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def frame_setup(srt, name, w, h, reference, bounces=8):
    """A tracer with the frame's camera rays bound and rmse(samples, sun): the error of one srt_trace_radiance over the hit pixels."""
    import rays_time as RT
    import torch

    objs, cnt = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", name + ".json")).objects_copy()
    pt = srt.PathTracer(w, h)
    pt.set_scene(objs, cnt)
    pt.set_camera(srt.default_camera())
    for first in range(1, reference + 1, 256):
        pt.render(spp=min(256, reference + 1 - first), bounces=bounces, seed=2, first_sample=first, reset=(first == 1))
    ref = lum(pt.accumulator()).reshape(-1)
    pt.render_gbuffer()
    mask = pt.gbuffer("object").reshape(-1) != -1
    o, d = RT.camera_rays(torch, w, h)
    torch.cuda.synchronize()
    pt.bind_rays(o, d)
    pt._keep = (o, d)

    def rmse(samples, sun, seed=11):
        pt.trace_radiance(samples=samples, bounces=bounces, seed=seed, sun_sampling=sun)
        e = (lum(pt.radiance(w * h)) - ref)[mask] / (ref[mask] + 0.01)
        return float(np.sqrt(np.mean(e * e)))

    return pt, rmse, dict(pixels=int(mask.sum()))


def frame(srt, a, name):
    import rays_time as RT
    import torch

    pt, rmse, info = frame_setup(srt, name, a.width, a.height, a.reference)
    stream = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    pt.set_stream(stream.cuda_stream)
    out = dict(tool="sun_sampling_quality", part="frame", scene=name, width=a.width, height=a.height, samples=a.samples, bounces=8, reference=a.reference,
               runs="one run", **info)

    def ms(samples, sun):
        return RT.timed(torch, stream, 5, 2, {"x": lambda: pt.trace_radiance(samples=samples, bounces=8, seed=11, sun_sampling=sun)})["x"]["median_ms"]

    for k, sun in (("off", False), ("on", True)):
        out[k] = {"rmse": round(rmse(a.samples, sun), 4), "ms": ms(a.samples, sun)}
    n = max(1, int(round(a.samples * out["on"]["ms"] / out["off"]["ms"])))
    out["off_equal_time"] = {"samples": n, "rmse": round(rmse(n, False), 4), "ms": ms(n, False)}
    out["ratio_off_over_on"] = round(out["off"]["rmse"] / out["on"]["rmse"], 3)
    out["ratio_off_equal_time_over_on"] = round(out["off_equal_time"]["rmse"] / out["on"]["rmse"], 3)
    pt.wait()
    pt.set_stream(0)
    pt.bind_rays(None, None)
    pt.close()
    return out


def probes(srt, a, name):
    objs, cnt = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", name + ".json")).objects_copy()
    pt = srt.PathTracer(64, 64)
    pt.set_scene(objs, cnt)
    pos = srt.probe_grid_positions((-2.5, 0.0, 1.0), (1.0, 0.75, 1.2), (6, 3, 6))
    pt.trace_light_probes(pos, a.directions, samples=256, bounces=8, seed=5)
    ref = lum(pt.light_probe_coefficients()[:, 0, :3])
    out = dict(tool="sun_sampling_quality", part="probes", scene=name, probes=len(pos), directions=a.directions, samples=16, bounces=8, reference_samples=256,
               runs="one run")
    for k, sun in (("off", False), ("on", True)):
        pt.trace_light_probes(samples=16, bounces=8, seed=9, sun_sampling=sun)
        e = lum(pt.light_probe_coefficients()[:, 0, :3]) - ref
        out[k] = {"dc_rmse_over_mean": round(float(np.sqrt(np.mean(e * e)) / np.mean(ref)), 4)}
    out["ratio_off_over_on"] = round(out["off"]["dc_rmse_over_mean"] / out["on"]["dc_rmse_over_mean"], 3)
    pt.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="Scene1,Scene2")
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--reference", type=int, default=4096)
    ap.add_argument("--directions", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    srt = importlib.import_module("software-raytracer_amd")
    lines = []
    for name in a.scenes.split(","):
        lines.append(frame(srt, a, name))
        lines.append(probes(srt, a, name))
    text = "".join(json.dumps(l) + "\n" for l in lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "a").write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
