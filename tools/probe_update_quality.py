#!/usr/bin/env python3
"""Quality of the hysteresis blend (srt_blend_probes) on an MI355X — JSON lines.

Part "static".  Static Scene_indirect, the spacing-1 grid over the hit points of the --width x --height frame (default 480 x 270: 210 probes), a
relocating classification, the list of active probes, --directions (64) directions, 8 bounces.  The yardstick is one trace of
--reference (4096) samples.  Per samples-per-frame n (--per-frame, default 1, 2, 4) and per hysteresis (--hystereses, default 0.8,
0.9, 0.97; fast_hysteresis the same, so that change detection does not act), --frames (16) frames f of one listed trace of n samples
with seed = f and RESET, each blended into a history that was reset first.  Reported per frame count 1, 2, 4, 8, 16: the RMSE of the
DC coefficients of the history and of the last frame alone against the yardstick over the listed probes, their ratio, and the
ratio independent frames would give: sqrt(h^(2(F-1)) + (1-h) (1 - h^(2(F-1))) / (1+h)).

    python tools/probe_update_quality.py --out profiles/probe_update/probe_update_quality.jsonl

Part "moving".  The same grid, --move-samples (4) samples per frame, no depth maps.  Frames 1 .. 7 blend the scene as it is from a reset
history; in front of frame 8 object --object (52: the big sphere) moves by --step (1.5, 0, 0) (srt_update_scene), the grid is classified
and listed again and the first-hit guides are rendered again; frames 8 .. 8 + --after (48) go on blending.  After every frame from 8
on the frame is shaded from the history (srt_shade_probe_grid_states, normal weight) and compared, over the hit pixels, with the
yardstick: the moved scene's probes traced once with --reference samples and shaded the same way.  The converged value of a setting
is the mean RMSE of the last 8 of --after frames blended in the moved scene from a reset history (no memory of the old scene);
"recovered_after" counts the frames from 8 until the RMSE first falls below twice that value (null: not within --after).  Settings:
hysteresis 0.8 / 0.9 / 0.97 x change detection off (fast_hysteresis = hysteresis) or on with fast_hysteresis 0.5 and change_threshold
0.1 / 0.25 / 0.5 x SRT_PROBE_BLEND_PREVIOUS_STATES off or on (the records of the old scene handed to the blend of frame 8).

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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from probe_depth_time import open_tracer  # noqa: E402
from probe_grid_time import bounds_grid  # noqa: E402


def moving(a, srt, torch, pt, scene, grid, rec0, pos0, words0):
    """Part "moving": see the module's docstring.  Returns the JSON lines."""
    P, K, n = grid.probes, a.directions, a.move_samples
    dev = "cuda:%d" % pt.device
    step = [np.float32(v) for v in a.step.split(",")]
    objs0, count = scene.objects_copy()
    objs1, _ = scene.objects_copy()
    for k in range(3):
        objs1[a.object].position[k] = np.float32(objs1[a.object].position[k]) + step[k]
    hist = torch.zeros((P * 9, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    pt.bind_probe_history("coefficients", hist)

    def enter(objs, first):
        """Make `objs` the scene: update, classify, list, guides; returns (records, positions, list words, hit mask)."""
        if first:
            pt.set_scene(objs, count)
        else:
            pt.update_scene(objs, count)
        pt.classify_probes(directions=K, relocate=True, positions=True)
        rec, pos = pt.probe_states_output("records"), pt.probe_states_output("positions")
        pt.bind_probe_grid_states(rec)
        pt.list_probes()
        words = pt.probe_list_output(P)
        pt.bind_probe_list(words)
        pt.render_gbuffer(outputs=["object", "normal_depth", "position"])
        return rec, pos, words, pt.gbuffer("object") != -1

    def shaded():
        pt.shade_probe_grid_states(coefficients=hist, normal_weight=True)
        return pt.probe_grid_output()[..., :3].astype(np.float64)

    # the yardstick: the moved scene, every probe traced once with many samples, shaded the same way
    rec1, pos1, words1, hit1 = enter(objs1, True)
    pt.trace_light_probes(pos1, None, samples=a.reference, bounces=a.bounces, seed=2000)
    pt.shade_probe_grid_states(coefficients=pt.light_probe_coefficients(), normal_weight=True)
    ref = pt.probe_grid_output()[..., :3].astype(np.float64)
    rmse = lambda img: float(np.sqrt(np.mean((img[hit1] - ref[hit1]) ** 2)))
    flips = int((((rec0[:, 3].copy().view(np.uint32) ^ rec1[:, 3].copy().view(np.uint32)) & 10) != 0).sum())
    moved_offsets = int((rec0[:, :3].view(np.uint32) != rec1[:, :3].view(np.uint32)).any(axis=1).sum())
    settings = []
    for hy in (0.8, 0.9, 0.97):
        settings.append((hy, hy, 0.25, False))
        for th in (0.1, 0.25, 0.5):
            settings.append((hy, min(0.5, hy), th, True))
    lines = []
    for hy, fast, th, detect in settings:
        kw = dict(hysteresis=hy, fast_hysteresis=fast, change_threshold=th, listed=True)
        # the converged value: the moved scene alone, from a reset history
        enter(objs1, True)
        pt.reset_probe_history(P)
        tail = []
        for f in range(1, a.after + 1):
            pt.trace_light_probes(pos1 if f == 1 else None, None, samples=n, bounces=a.bounces, seed=5000 + f, listed=True)
            pt.blend_probes(**kw)
            if f > a.after - 8:
                tail.append(rmse(shaded()))
        converged = float(np.mean(tail))
        for previous in (False, True):
            rec, pos, words, _ = enter(objs0, True)
            pt.reset_probe_history(P)
            for f in range(1, 8):
                pt.trace_light_probes(pos if f == 1 else None, None, samples=n, bounces=a.bounces, seed=f, listed=True)
                pt.blend_probes(**kw)
            enter(objs1, False)
            if previous:
                pt.bind_probe_previous_states(rec)
            curve, recovered, work8 = [], None, None
            for f in range(8, 8 + a.after + 1):
                pt.trace_light_probes(pos1 if f == 8 else None, None, samples=n, bounces=a.bounces, seed=f, listed=True)
                pt.blend_probes(previous_states=previous and f == 8, count_work=f == 8, **kw)
                if f == 8:
                    work8 = pt.probe_blend_work()
                e = rmse(shaded())
                curve.append(round(e, 5))
                if recovered is None and e <= 2.0 * converged:
                    recovered = f - 8
            lines.append({"tool": "probe_update_quality", "part": "moving", "device": torch.cuda.get_device_name(0), "scene": a.scene, "width": a.width,
                          "height": a.height, "probes": P, "listed_before": int(words0[0]), "listed_after": int(words1[0]), "directions": K, "bounces": a.bounces,
                          "samples_per_frame": n, "object": a.object, "step": [float(v) for v in step], "records_bit_flips": flips, "records_offset_changes": moved_offsets,
                          "reference_samples": a.reference, "hysteresis": hy, "change_detection": detect, "fast_hysteresis": fast, "change_threshold": th,
                          "previous_states": previous, "converged_rmse": round(converged, 5), "recovered_after": recovered, "rmse_frame_8": curve[0],
                          "rmse_8_16_24_32_48": [curve[i] for i in (8, 16, 24, 32, min(48, len(curve) - 1)) if i < len(curve)], "frame_8_work": work8})
    pt.wait()
    pt.bind_probe_history("coefficients", None)
    pt.bind_probe_previous_states(None)
    pt.bind_probe_list(None)
    pt.bind_probe_grid_states(None)
    pt.L.srt_bind_probe_grid_coefficients(pt._h, None, 0)
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="Scene_indirect")
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    ap.add_argument("--spacing", type=float, default=1.0)
    ap.add_argument("--directions", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--reference", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--per-frame", default="1,2,4")
    ap.add_argument("--hystereses", default="0.8,0.9,0.97")
    ap.add_argument("--parts", default="static,moving")
    ap.add_argument("--object", type=int, default=52)
    ap.add_argument("--step", default="1.5,0,0")
    ap.add_argument("--move-samples", type=int, default=4)
    ap.add_argument("--after", type=int, default=48)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    srt = importlib.import_module("software-raytracer_amd")
    pt, scene = open_tracer(srt, a.scene, a.width, a.height)
    parts = a.parts.split(",")
    pt.render_gbuffer(outputs=["object", "normal_depth", "position"])
    grid = bounds_grid(pt.gbuffer("object"), pt.gbuffer("position"), a.spacing)
    P = grid.probes
    pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
    pt.classify_probes(directions=a.directions, relocate=True, positions=True)
    rec, pos = pt.probe_states_output("records"), pt.probe_states_output("positions")
    pt.bind_probe_grid_states(rec)
    pt.list_probes()
    words = pt.probe_list_output(P)
    n_listed = int(words[0])
    idx = words[4:4 + n_listed].astype(np.int64)
    pt.bind_probe_list(words)
    pt.trace_light_probes(pos, None, samples=a.reference, bounces=a.bounces, seed=1000)
    truth = pt.light_probe_coefficients()[idx, 0, :3].astype(np.float64)
    rmse = lambda v: float(np.sqrt(np.mean((v[idx, 0, :3].astype(np.float64) - truth) ** 2)))
    lines = []
    for n in ([int(s) for s in a.per_frame.split(",")] if "static" in parts else []):
        for hy in [float(s) for s in a.hystereses.split(",")]:
            pt.reset_probe_history(P)
            rows = []
            for f in range(1, a.frames + 1):
                pt.trace_light_probes(samples=n, bounces=a.bounces, seed=f, listed=True)
                pt.blend_probes(hysteresis=hy, fast_hysteresis=hy, listed=True)
                if f in (1, 2, 4, 8, 16, a.frames):
                    e_frame, e_hist = rmse(pt.light_probe_coefficients()), rmse(pt.probe_history("coefficients"))
                    h2 = hy ** (2 * (f - 1))
                    rows.append({"frames": f, "rmse_frame": round(e_frame, 6), "rmse_history": round(e_hist, 6), "ratio": round(e_hist / e_frame, 4),
                                 "independent": round((h2 + (1 - hy) * (1 - h2) / (1 + hy)) ** 0.5, 4)})
            lines.append({"tool": "probe_update_quality", "device": torch.cuda.get_device_name(0), "scene": a.scene, "width": a.width, "height": a.height,
                          "grid_spacing": a.spacing, "grid_counts": list(grid.counts), "probes": P, "listed": n_listed, "directions": a.directions, "bounces": a.bounces,
                          "reference_samples": a.reference, "samples_per_frame": n, "hysteresis": hy, "after": rows})
    if "moving" in parts:
        lines += moving(a, srt, torch, pt, scene, grid, rec, pos, words)
    pt.close()
    text = "".join(json.dumps(line) + "\n" for line in lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
