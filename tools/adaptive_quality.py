#!/usr/bin/env python3
"""Adaptive against uniform sampling at an equal total sample count on an MI355X — one JSON line per scene and threshold.

For each scene (default Scene1 and Scene_indirect) at --width x --height (default 1920 x 1080), the default camera, --bounces
bounces:

    reference  srt_render at --reference (default 4096) samples, seed 12345
    adaptive   the two-half workflow of include/srt_pathtrace.h: --seed-samples (default 8) samples per half (seeds 0 and
               0x9E3779B9), the guides once, --rounds (default 2) rounds of srt_variance, srt_sample_budget (threshold from
               --thresholds, default 0.1,0.05,0.025; floor and max_budget the library's) and srt_render_adaptive on both halves, then
               srt_variance with MERGE; total = the sum over the pixels of twice the per-half count
    uniform    srt_render with seed 0 at ceil(total / pixels) samples per pixel: never fewer samples than adaptive had

The metric is the relative luminance RMSE over hit pixels, sqrt(mean(((lum x - lum ref) / (lum ref + 0.01))^2)) with Rec. 709
luminance.  Every (scene, threshold) runs in a child process of its own under its own time limit (--limit seconds); the first
failure ends the run.  What comes out is reported as it is, also where adaptive loses.

    python tools/adaptive_quality.py --out profiles/adaptive/adaptive_quality.jsonl

Lines go to stdout, or are appended to --out FILE.  GPU box only."""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lum(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def step(a):
    import numpy as np

    srt = importlib.import_module("software-raytracer_amd")
    scene = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", a.scene + ".json"))
    objs, cnt = scene.objects_copy()
    pt = srt.PathTracer(a.width, a.height)
    pt.set_scene(objs, cnt)
    pt.set_camera(srt.default_camera())
    px = a.width * a.height

    def rmse(acc, ref, hit):
        x, r = lum(acc[..., :3].astype(np.float64))[hit], lum(ref[..., :3].astype(np.float64))[hit]
        return float(np.sqrt(np.mean(((x - r) / (r + 0.01)) ** 2)))

    pt.render(spp=a.reference, bounces=a.bounces, seed=12345)
    ref = pt.accumulator()
    pt.render_gbuffer()
    hit = pt.gbuffer("object") >= 0
    # adaptive: the seed in two halves, the rounds, the merge
    n, seed_b, half = a.seed_samples, 0x9E3779B9, pt.half_ptr()
    pt.render(spp=n, bounces=a.bounces, seed=0)
    pt.bind_output(None, half)
    pt.render(spp=n, bounces=a.bounces, seed=seed_b)
    pt.bind_output()
    pt.set_sample_counts(n)
    budgets = []
    for _ in range(a.rounds):
        pt.variance(merge=False, gbuffer=False)
        pt.sample_budget(threshold=a.threshold)
        budgets.append(pt.budget_total())
        pt.render_adaptive(bounces=a.bounces, seed=0, keep_counts=True)
        pt.bind_output(None, half)
        pt.render_adaptive(bounces=a.bounces, seed=seed_b)
        pt.bind_output()
    pt.variance(merge=True, gbuffer=False)
    merged = pt.accumulator()
    counts = pt.sample_counts().astype(np.int64)
    total = int(2 * counts.sum())
    spp = -(-total // px)
    pt.render(spp=spp, bounces=a.bounces, seed=0)
    uniform = pt.accumulator()
    pt.render(spp=2 * n, bounces=a.bounces, seed=0)
    seeded = pt.accumulator()
    pt.close()
    ra, ru = rmse(merged, ref, hit), rmse(uniform, ref, hit)
    return {"tool": "adaptive_quality", "scene": a.scene, "width": a.width, "height": a.height, "bounces": a.bounces, "reference_samples": a.reference,
            "seed_samples_per_half": n, "rounds": a.rounds, "threshold": a.threshold, "hit_pixels": int(hit.sum()), "round_budgets_per_half": budgets,
            "adaptive_total_samples": total, "adaptive_samples_per_pixel": round(total / px, 3), "adaptive_max_samples_of_a_pixel": int(2 * counts.max()),
            "uniform_samples_per_pixel": spp, "rmse_uniform_seed_only": round(rmse(seeded, ref, hit), 5), "rmse_adaptive": round(ra, 5),
            "rmse_uniform_equal_total": round(ru, 5), "adaptive_to_uniform": round(ra / ru, 4) if ru else None}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="Scene1,Scene_indirect")
    ap.add_argument("--thresholds", default="0.1,0.05,0.025")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--reference", type=int, default=4096)
    ap.add_argument("--seed-samples", dest="seed_samples", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds a step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--scene", default=None, help="(internal) with --threshold: run one step in this process and print its JSON")
    ap.add_argument("--threshold", type=float, default=None)
    a = ap.parse_args()
    if a.scene:
        print("RESULT " + json.dumps(step(a)))
        return 0
    for scene in a.scenes.split(","):
        for tau in a.thresholds.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--scene", scene, "--threshold", tau] + [
                x for k in ("width", "height", "bounces", "reference", "seed_samples", "rounds") for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                sys.stderr.write("adaptive_quality: %s at %s ran into its limit of %d s; stopping\n" % (scene, tau, a.limit))
                return 1
            res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not res:
                sys.stderr.write("adaptive_quality: %s at %s failed (exit %d); stopping\n%s\n" % (scene, tau, r.returncode, r.stderr[-2000:]))
                return 1
            text = res[-1][len("RESULT "):] + "\n"
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(text)
            sys.stdout.write(text)
            sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
