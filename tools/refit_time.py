#!/usr/bin/env python3
"""What an object move costs on an MI355X with and without the refit of the mesh BVH (srt_update_mode) — JSON lines.

    python tools/refit_time.py [--out profiles/refit/refit_time.jsonl]

Two scenes: BASELINE config 4's (Scene1 with its big ball as a 224 x 224 lat-long sphere, 99,904 triangles) and Scene1 with the
ball as a small mesh (16 x 20, 600 triangles).  For each, in one process and one context per setting, the median of --moves
wall-clock times of srt_update_scene + srt_wait (after --warmup moves):
    rebuild        SRT_UPDATE_REBUILD moving the mesh: the behaviour before the refit existed, the yardstick
    refit          SRT_UPDATE_REFIT moving the mesh (path 2)
    kept           SRT_UPDATE_REFIT moving a sphere (path 3)
and what the refitted tree costs to trace: bvh_child_tests and kernel_ms of one 4-spp render (1280 x 720, 8 bounces) after a
refit that moved the mesh by 0, 0.1 and 2 times its extent, next to the same list set afresh (`tree` lines).
The lines go to stdout, or are appended to --out FILE.  GPU box only."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MESH_OBJECT, SPHERE_OBJECT = 64, 3  # Scene1's big ball (r = 1, extent 2) and one of its small spheres
SCENES = {"config4_mesh224": (224, 224), "scene1_mesh16x20": (16, 20)}


def scene_with_mesh(srt, stacks, slices):
    doc = json.load(open(os.path.join(ROOT, "software-raytracer_amd", "scenes", "Scene1.json")))
    doc["SceneObjects"][MESH_OBJECT]["Renderer"] = {"Type": "Mesh", "Primitive": "UVSphere", "Radius": 1.0, "Stacks": stacks, "Slices": slices}
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(doc, f)
    try:
        scene = srt.host.Scene(f.name)
    finally:
        os.unlink(f.name)
    assert scene.error == "", scene.error
    return scene


def tracer(srt, scene, w, h, refit):
    marr, mn = scene.meshes()
    objs, n = scene.objects_copy()
    pt = srt.PathTracer(w, h)
    pt.update_mode(refit)
    pt.set_meshes(C.cast(marr, C.POINTER(srt.Mesh)), mn)
    pt.set_scene(objs, n)
    pt.set_camera(srt.default_camera())
    pt.wait()
    return pt, objs, n


def shift(objs, index, base, d):
    objs[index].position = (C.c_float * 3)(base[0] + d[0], base[1] + d[1], base[2] + d[2])


def time_moves(srt, scene, a, refit, index, want_path):
    pt, objs, n = tracer(srt, scene, 64, 36, refit)
    base = list(objs[index].position)
    ms = []
    for k in range(a.warmup + a.moves):
        shift(objs, index, base, (0.01 * (k + 1), 0.0, 0.005 * (k + 1)))
        t0 = time.perf_counter()
        pt.update_scene(objs, n)
        pt.wait()
        t1 = time.perf_counter()
        if k >= a.warmup:
            ms.append((t1 - t0) * 1e3)
            assert pt.update_info()["path"] == want_path, pt.update_info()
    info = pt.update_info()
    pt.close()
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "path": info["path"],
            "levels": info["levels"], "triangles": info["triangles"], "nodes": info["nodes"]}


def tree_cost(srt, scene, a, extents):
    """One 4-spp render after a refit by `extents` times the mesh's extent (2), and after a fresh set of the same list."""
    out = {}
    for how in ("refit", "fresh"):
        pt, objs, n = tracer(srt, scene, a.width, a.height, True)
        base = list(objs[MESH_OBJECT].position)
        if how == "refit":  # (there and on to the target, so that a move by 0 is a refit too)
            shift(objs, MESH_OBJECT, base, (0.0, 0.0, 1.0))
            pt.update_scene(objs, n)
        shift(objs, MESH_OBJECT, base, (2.0 * extents, 0.0, 0.0))
        if how == "refit":
            pt.update_scene(objs, n)
            assert pt.update_info()["path"] == 2
        else:
            pt.set_scene(objs, n)
        pt.render(spp=4, bounces=8, seed=0, count_work=True)
        pt.wait()
        out[how + "_bvh_child_tests"] = pt.work_counts().as_dict()["bvh_child_tests"]
        pt.render(spp=4, bounces=8, seed=0)  # (timed without the counters)
        pt.wait()
        out[how + "_kernel_ms"] = round(float(pt.stats().kernel_ms), 4)
        pt.close()
    out["child_tests_ratio"] = round(out["refit_bvh_child_tests"] / max(out["fresh_bvh_child_tests"], 1), 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--moves", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--out", default=None, help="append the lines to this file instead of printing them")
    a = ap.parse_args()
    import torch

    srt = importlib.import_module("software-raytracer_amd")
    lines = []
    for name, (stacks, slices) in SCENES.items():
        scene = scene_with_mesh(srt, stacks, slices)
        head = {"tool": "refit_time", "device": torch.cuda.get_device_name(0), "scene": name, "moves": a.moves, "warmup": a.warmup}
        for setting, refit, index, path in (("rebuild", False, MESH_OBJECT, 1), ("refit", True, MESH_OBJECT, 2), ("kept", True, SPHERE_OBJECT, 3)):
            lines.append(dict(head, mode="update", setting=setting, **time_moves(srt, scene, a, refit, index, path)))
        for extents in (0.0, 0.1, 2.0):
            lines.append(dict(head, mode="tree", moved_extents=extents, width=a.width, height=a.height, spp=4, bounces=8,
                              **tree_cost(srt, scene, a, extents)))
    text = "".join(json.dumps(line) + "\n" for line in lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
