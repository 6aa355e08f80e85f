#!/usr/bin/env python3
"""Time of srt_trace_light_probes on an MI355X next to the route it replaces — one JSON line per scene.

Scene1 and Scene_indirect, --probes (default 4096) probes on a 16 x 16 x 16 grid inside the scenes' bounds, --directions (default
256) spherical Fibonacci directions, --samples (default 16) samples of --bounces (default 8) bounces, seed 0.  One child process
per scene under its own time limit (--limit seconds); the first failure ends the run and nothing is written.  Per scene:

    device     --launches launches after --warmup of four calls, alternating launch by launch, each bracketed by two events on
               the tracer's stream; median / min / max of each:
                 probes_coefficients   srt_trace_light_probes, COEFFICIENTS only
                 probes_radiance       the same with the RADIANCE output as well
                 radiance_a, _b        srt_trace_radiance on the same P*K rays, bound as an explicit batch: the device time of
                                       the route without the fused pass, twice, so that the spread between the two is the
                                       yardstick for the ratio probes_coefficients / radiance_a
    host       the whole route without the fused pass on the host clock, once after a warm-up: build the P*K rays, srt_write_rays,
               srt_trace_radiance, srt_read_radiance, project onto the nine coefficients with numpy
    bytes      what each route moves to and from the device

    python tools/light_probe_time.py --out profiles/light_probes/light_probe_time.jsonl

The lines go to stdout, or are appended to --out FILE.  GPU box only."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SCENES = ("Scene1", "Scene_indirect")
LO, HI = (-2.4, -0.8, 0.5), (2.4, 1.4, 6.0)  # inside Scene_indirect's room, around Scene1's spheres


def grid(np, count):
    side = max(1, round(count ** (1.0 / 3.0)))
    while side ** 3 < count:
        side += 1
    ax = [np.linspace(LO[i], HI[i], side, dtype=np.float32) for i in range(3)]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    pos = np.zeros((side ** 3, 4), dtype=np.float32)
    pos[:, 0], pos[:, 1], pos[:, 2] = x.ravel(), y.ravel(), z.ravel()
    return pos[:count]


def basis_terms(np, d):
    x, y, z, w = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
    b = np.stack([np.full_like(x, 0.282095), 0.488603 * y, 0.488603 * z, 0.488603 * x, 1.092548 * (x * y), 1.092548 * (y * z),
                  0.315392 * (3.0 * (z * z) - 1.0), 1.092548 * (x * z), 0.546274 * (x * x - y * y)], axis=1)
    return (w[:, None] * b).astype(np.float32)


def step_scene(a):
    import numpy as np
    import torch

    import rays_time as R

    srt = importlib.import_module("software-raytracer_amd")
    scene = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", a.step + ".json"))
    objs, cnt = scene.objects_copy()
    pt = srt.PathTracer(64, 64)  # (the frame size plays no part)
    pt.set_scene(objs, cnt)
    stream = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    pt.set_stream(stream.cuda_stream)
    pos, d = grid(np, a.probes), srt.light_probe_sphere(a.directions)
    P, K = pos.shape[0], d.shape[0]
    kw = dict(samples=a.samples, bounces=a.bounces, seed=0)

    def build_rays():
        return np.repeat(pos, K, axis=0), np.tile(d, (P, 1))

    o, dd = build_rays()
    to, td = torch.from_numpy(o).to("cuda:0"), torch.from_numpy(dd).to("cuda:0")
    torch.cuda.synchronize()
    pt.bind_rays(to, td)
    pt.trace_light_probes(pos, d, **kw)
    t = R.timed(torch, stream, a.launches, a.warmup, {
        "probes_coefficients": lambda: pt.trace_light_probes(**kw),
        "probes_radiance": lambda: pt.trace_light_probes(radiance=True, **kw),
        "radiance_a": lambda: pt.trace_radiance(**kw),
        "radiance_b": lambda: pt.trace_radiance(**kw)})
    pt.trace_light_probes(radiance=True, count_work=True, **kw)
    coeff, rad, work = pt.light_probe_coefficients(), pt.light_probe_radiance(), pt.light_probe_work()
    pt.trace_radiance(**kw)
    equal = int((pt.radiance().view(np.uint32) == rad.reshape(-1, 4).view(np.uint32)).all(axis=1).sum())
    pt.bind_rays(None, None)

    def host_route():
        t0 = time.perf_counter()
        ho, hd = build_rays()
        pt.write_rays(ho, hd)
        pt.trace_radiance(**kw)
        L = pt.radiance().reshape(P, K, 4)
        c = np.einsum("pkl,kc->pcl", L[..., :3], basis_terms(np, d))
        return (time.perf_counter() - t0) * 1e3, c

    host_route()
    host_ms, c = host_route()
    err = float(np.abs(c - coeff[..., :3]).max() / max(1e-30, float(np.abs(coeff[..., :3]).max())))
    pt.wait()
    pt.set_stream(0)
    pt.close()
    out = {"scene": a.step, "device": torch.cuda.get_device_name(0), "probes": P, "directions": K, "rays": work["rays"], "waves": work["waves"],
           "wave_calls": work["wave_calls"], "closest_calls": work["closest_calls"], "radiance_elements_equal_to_trace_radiance": equal,
           "host_route_ms": round(host_ms, 3), "host_projection_max_relative_difference": err,
           "bytes_up_probes": 16 * (P + K), "bytes_down_probes": 144 * P, "bytes_up_route": 32 * P * K, "bytes_down_route": 16 * P * K}
    for k, v in t.items():
        out.update({k + "_median_ms": v["median_ms"], k + "_min_ms": v["min_ms"], k + "_max_ms": v["max_ms"]})
    out["probes_to_radiance"] = round(out["probes_coefficients_median_ms"] / out["radiance_a_median_ms"], 4)
    out["radiance_b_to_radiance_a"] = round(out["radiance_b_median_ms"] / out["radiance_a_median_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--probes", type=int, default=4096)
    ap.add_argument("--directions", type=int, default=256)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=180, help="seconds a scene may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=SCENES, default=None, help="(internal) run one scene in this process and print its JSON")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step_scene(a)))
        return 0
    lines = []
    for scene in SCENES:  # each in a fresh process, under its own limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--step", scene] + [x for k in ("probes", "directions", "samples", "bounces", "launches", "warmup")
                                                                             for x in ("--" + k, str(getattr(a, k)))]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            sys.stderr.write("light_probe_time: scene %s ran into its limit of %d s; stopping\n" % (scene, a.limit))
            return 1
        res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not res:
            sys.stderr.write("light_probe_time: scene %s failed (exit %d); stopping\n%s\n" % (scene, r.returncode, r.stderr[-2000:]))
            return 1
        line = {"tool": "light_probe_time", "samples": a.samples, "bounces": a.bounces, "launches": a.launches, "warmup": a.warmup}
        line.update(json.loads(res[-1][len("RESULT "):]))
        lines.append(json.dumps(line) + "\n")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.writelines(lines)
    sys.stdout.writelines(lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
