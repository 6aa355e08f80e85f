#!/usr/bin/env python3
"""The image passes of several BUILDS of the library against each other, in ONE process on one box: what tests/ab_libs.py does
for srt_render, for srt_denoise, srt_denoise_variance, srt_upsample, srt_temporal_accumulate, srt_antialias and the three probe-grid
shading calls (srt_shade_probe_grid, srt_shade_probe_grid_depth, srt_shade_probe_grid_states).
usage: python tests/ab_passes.py --libs base=path/a.so,new=path/b.so [--part bits,time] [--rounds 15] [--noise base,base2]

bits: at the frame shapes SHAPES (one pixel, a tile seam, partial tiles both ways, a partial third workgroup across, the
prefilter's apron at all four frame edges and inside), on the guides of tests/pass_edge_inputs.py bound as torch tensors and a
seeded variance with exact zeros, every library runs the same calls on a tracer of its own; the raw bytes of every result
buffer and of the framebuffer must be the same in all libraries, NaN payloads included.  A difference names the pass, the
shape and the parameters, and the exit status is 1.
time: 1920 x 1080 on Scene1's real guides (as tools/denoise_time.py and tools/variance_time.py set them up), one tracer per
library on one stream; every call is bracketed by two events, the libraries take turns within a round, and the median per
(call, library) is printed with its ratio to the first library.  With --noise a,b (two copies of one build under two file
names) the noise floor of a call is the relative difference of the medians of a and b, and every other library passes the call
when its median is at most the slower copy's plus that floor."""
import argparse
import importlib
import itertools
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pass_edge_inputs as pe  # noqa: E402
from probe_grid_time import bounds_grid  # noqa: E402
import test_gpu_temporal as tp  # noqa: E402

SHAPES = [(1, 1), (9, 9), (17, 15), (33, 18), (37, 21), (64, 48)]


def _cuda(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _bind_guides(pt, tensors):
    for k, v in tensors.items():
        pt.bind_gbuffer(k, v)


def seeded_variance(w, h):
    """Non-negative, about a fifth of it exactly 0."""
    rng = np.random.default_rng(pe.shape_seed(w, h) + 17)
    var = rng.uniform(0.0, 0.5, (h, w)).astype(np.float32)
    var[rng.random((h, w)) < 0.2] = 0.0
    return var


def pass_results(srt, L, w, h):
    """[(what, bytes)] of every call of the bits part on one tracer of library L."""
    acc, obj, nd, pos, alb = pe.guides(w, h, pe.shape_seed(w, h))
    keep = {"object": _cuda(obj), "normal_depth": _cuda(nd), "position": _cuda(pos), "albedo": _cuda(alb), "variance": _cuda(seeded_variance(w, h))}
    out = []

    def took(what, **buffers):
        for name, a in buffers.items():
            out.append(("%s at %d x %d: %s" % (what, w, h, name), np.ascontiguousarray(a).tobytes()))

    pt = srt.PathTracer(w, h, lib=L)
    _bind_guides(pt, {k: keep[k] for k in ("object", "normal_depth", "position", "albedo")})
    pt.bind_variance(keep["variance"])
    pt.write_accumulator(acc)
    for levels, albedo in itertools.product((1, 2, 5), (False, True)):
        for sc in (0.0, 0.5):
            pt.denoise(iterations=levels, sigma_color=sc, albedo=albedo, framebuffer=True, gbuffer=False)
            took("srt_denoise iterations %d albedo %d sigma_color %g" % (levels, albedo, sc), denoised=pt.denoised(), framebuffer=pt.framebuffer())
        for sl in (0.0, 4.0):
            pt.denoise_variance(iterations=levels, sigma_luminance=sl, albedo=albedo, framebuffer=True, gbuffer=False)
            took("srt_denoise_variance iterations %d albedo %d sigma_luminance %g" % (levels, albedo, sl), denoised=pt.denoised(),
                 framebuffer=pt.framebuffer())
    for steps, stripe in itertools.product((2, 3), (0, 5)):
        what = "srt_upsample steps %d stripe %d" % (steps, stripe)
        pt.upsample(steps=steps, stripe_width=stripe, framebuffer=True, gbuffer=False)
        took(what, upsampled=pt.upsampled(), framebuffer=pt.framebuffer())
        pt.upsample(steps=steps, stripe_width=stripe, in_place=True, framebuffer=True, gbuffer=False)
        took(what + " in place", accumulator=pt.accumulator(), framebuffer=pt.framebuffer())
        pt.write_accumulator(acc)
    # srt_antialias on the same OBJECT guide
    _, _, sub, _ = pe.antialias_inputs(w, h, 2)
    keep["sub"] = _cuda(sub)
    pt.bind_subsamples(keep["sub"])
    pt.antialias(2, framebuffer=True, guides=False)
    took("srt_antialias k 2", antialiased=pt.antialiased(), framebuffer=pt.framebuffer())
    # two frames of srt_temporal_accumulate: guides cast from two cameras (test_gpu_temporal.MOVES), so that history is found
    rng = np.random.default_rng(pe.shape_seed(w, h) + 29)
    for frame, (p, yaw, fov) in enumerate(tp.MOVES[1:3]):
        cam = tp.camera(srt, p, yaw, fov)
        for k, v in zip(tp.GUIDES, tp.cast(cam, w, h)):
            keep["t%d %s" % (frame, k)] = _cuda(v)
            pt.bind_gbuffer(k, keep["t%d %s" % (frame, k)])
        pt.set_camera(cam)
        pt.write_accumulator(np.concatenate([rng.uniform(0.02, 3.0, (h, w, 3)), rng.choice([0.0, 1.0], (h, w, 1))], -1).astype(np.float32))
        pt.temporal(samples=1, framebuffer=True, gbuffer=False)
        took("srt_temporal_accumulate frame %d" % frame, accumulator=pt.accumulator(), history_length=pt.history_length(), framebuffer=pt.framebuffer())
    pt.close()
    del keep
    return out


def probe_inputs(probes, spacing, R, seed):
    """Seeded inputs of the three probe-grid shading calls: coefficients (P, 9, 4), depth moments (P, R*R, 4) whose mean distances
    lie on both sides of a corner's distance, and records (P, 4) with offsets within 0.45 of the spacing and about 30 % BURIED."""
    rng = np.random.default_rng(seed)
    coeff = rng.uniform(-1.0, 2.0, (probes, 9, 4)).astype(np.float32)
    m1 = rng.uniform(0.1, 1.5, (probes, R * R)) * float(np.linalg.norm(spacing))
    depth = np.stack([m1, m1 * m1 + rng.uniform(0.0, 0.5, m1.shape), rng.uniform(0.0, 4.0, m1.shape), rng.uniform(0.0, 1.0, m1.shape)], -1).astype(np.float32)
    rec = np.zeros((probes, 4), np.float32)
    rec[:, :3] = rng.uniform(-0.45, 0.45, (probes, 3)) * np.asarray(spacing, np.float64)[None, :]
    rec[:, 3] = np.where(rng.random(probes) < 0.3, 2, 0).astype(np.uint32).view(np.float32)  # SRT_PROBE_BURIED
    return coeff, depth, rec


def probe_grid_results(srt, L, w, h, scene):
    """[(what, bytes)] of srt_shade_probe_grid, _depth and _states on one tracer of library L: the output and the work record of
    every flag combination the calls' own tests iterate over, on the guides of pass_results and a seeded 3 x 3 x 3 grid."""
    import ctypes as C

    _, obj, nd, pos, alb = pe.guides(w, h, pe.shape_seed(w, h))
    keep = {"object": _cuda(obj), "normal_depth": _cuda(nd), "position": _cuda(pos), "albedo": _cuda(alb)}
    rng = np.random.default_rng(pe.shape_seed(w, h) + 41)
    origin = np.array([-0.2, -0.2, 1.5]) + rng.uniform(0.0, 0.1, 3)  # (the points lie in [0, 0.01 w] x [0, 0.01 h] x [2, 5.7]; some are clamped)
    spacing = np.array([rng.uniform(0.2, 0.4), rng.uniform(0.2, 0.4), rng.uniform(1.5, 2.0)])
    coeff, depth, rec = probe_inputs(27, spacing, 8, pe.shape_seed(w, h) + 43)
    out = []
    pt = srt.PathTracer(w, h, lib=L)
    pt.set_scene(*scene)
    _bind_guides(pt, keep)
    pt.set_probe_grid(origin, spacing, (3, 3, 3))

    def took(what):
        work = srt.capi.ProbeGridWork()
        pt._ck(L.srt_get_probe_grid_work(pt._h, C.byref(work)))
        out.append(("%s at %d x %d: output" % (what, w, h), pt.probe_grid_output().tobytes()))
        out.append(("%s at %d x %d: work" % (what, w, h), bytes(work)))

    first = True
    for vis, nw, al in itertools.product((False, True), repeat=3):
        pt.shade_probe_grid(coefficients=coeff if first else None, visibility=vis, normal_weight=nw, albedo=al, count_work=True)
        took("srt_shade_probe_grid visibility %d normal_weight %d albedo %d" % (vis, nw, al))
        first = False
    for nw, al in itertools.product((False, True), repeat=2):
        pt.shade_probe_grid_depth(moments=depth, resolution=8, normal_weight=nw, albedo=al, count_work=True)
        took("srt_shade_probe_grid_depth normal_weight %d albedo %d" % (nw, al))
        for with_depth in (False, True):
            pt.shade_probe_grid_states(states=rec, depth=with_depth, normal_weight=nw, albedo=al, count_work=True)
            took("srt_shade_probe_grid_states depth %d normal_weight %d albedo %d" % (with_depth, nw, al))
    pt.wait()
    for k in keep:
        pt.bind_gbuffer(k, None)
    pt.close()
    del keep
    return out


def compare_bits(srt, libs):
    """The number of result buffers that differ from the first library's."""
    differ = compared = 0
    scene = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", "Scene1.json")).objects_copy()
    for w, h in SHAPES:
        results = [pass_results(srt, L, w, h) + probe_grid_results(srt, L, w, h, scene) for _, L in libs]
        for (name, _), got in zip(libs[1:], results[1:]):
            assert [what for what, _ in got] == [what for what, _ in results[0]]
            for (what, a), (_, b) in zip(results[0], got):
                compared += 1
                if a != b:
                    differ += 1
                    n = int(np.count_nonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8)))
                    print("!!! %s: %s DIFFERS from %s in %d of %d bytes" % (what, name, libs[0][0], n, len(a)), flush=True)
    print("bits: %d buffers compared against %s, %d differ" % (compared, libs[0][0], differ), flush=True)
    return differ


def time_calls(srt, libs, a):
    import torch

    w, h = 1920, 1080
    objs, n = srt.host.Scene(os.path.join(ROOT, "software-raytracer_amd", "scenes", "Scene1.json")).objects_copy()
    stream = torch.cuda.Stream(device=0)
    guides = {"object": torch.empty((h, w), dtype=torch.int32, device="cuda:0")}
    for k in ("normal_depth", "position", "albedo"):
        guides[k] = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
    half = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    var = torch.empty((h, w), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    pts, outs, acc = [], [], None
    for _, L in libs:
        pt = srt.PathTracer(w, h, lib=L)
        pt.set_scene(objs, n)
        pt.set_camera(srt.default_camera())
        pt.set_stream(stream.cuda_stream)
        _bind_guides(pt, guides)
        pt.bind_half(half)
        pt.bind_variance(var)
        outs.append(torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0"))
        torch.cuda.synchronize()
        pt.bind_denoised(outs[-1])
        if acc is None:  # the first library renders the two halves of 1 spp, the guides and the variance that all of them read
            pt.render(spp=1, bounces=8, seed=0)
            pt.bind_output(None, half.data_ptr())
            pt.render(spp=1, bounces=8, seed=0x9E3779B9)
            pt.bind_output()
            pt.render_gbuffer()
            pt.variance(albedo=True, merge=True, gbuffer=False)
            pt.wait()
            acc = pt.accumulator()
        else:
            pt.write_accumulator(acc)
        pts.append(pt)
    calls = [
        ("srt_denoise defaults", lambda pt: pt.denoise(gbuffer=False)),
        ("srt_denoise sigma_color 0.5", lambda pt: pt.denoise(sigma_color=0.5, gbuffer=False)),
        ("srt_denoise_variance defaults", lambda pt: pt.denoise_variance(gbuffer=False)),
        ("srt_denoise_variance sigma_luminance 0", lambda pt: pt.denoise_variance(sigma_luminance=0.0, gbuffer=False)),
        ("srt_upsample steps 2", lambda pt: pt.upsample(steps=2, gbuffer=False)),
        ("srt_shade_probe_grid no flags", lambda pt: pt.shade_probe_grid()),
        ("srt_shade_probe_grid visibility normal_weight", lambda pt: pt.shade_probe_grid(visibility=True, normal_weight=True)),
        ("srt_shade_probe_grid_depth normal_weight", lambda pt: pt.shade_probe_grid_depth(normal_weight=True)),
        ("srt_shade_probe_grid_states depth", lambda pt: pt.shade_probe_grid_states(depth=True)),
        ("srt_shade_probe_grid_states no depth", lambda pt: pt.shade_probe_grid_states()),
    ]
    # the probe grid of tools/probe_grid_time.py: spacing 1 over the bounds of the frame's hit points, and seeded inputs
    torch.cuda.synchronize()
    grid = bounds_grid(guides["object"].cpu().numpy(), guides["position"].cpu().numpy(), 1.0)
    coeff, depth, rec = probe_inputs(grid.probes, grid.spacing, 8, 7)
    for pt in pts:
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        pt.shade_probe_grid_states(coefficients=coeff, states=rec, moments=depth, resolution=8)
        pt.wait()
    ms = {(c, i): [] for c, _ in calls for i in range(len(libs))}
    for r in range(a.warm + a.rounds):
        for cname, call in calls:
            for i, pt in enumerate(pts):
                b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                b.record(stream)
                call(pt)
                e.record(stream)
                stream.synchronize()
                if r >= a.warm:
                    ms[cname, i].append(b.elapsed_time(e))
    names = [name for name, _ in libs]
    noise = [names.index(x) for x in a.noise.split(",")] if a.noise else None
    for cname, _ in calls:
        med = [statistics.median(ms[cname, i]) for i in range(len(libs))]
        for i, name in enumerate(names):
            print("%-40s %-9s median %8.4f ms  min %8.4f  x%.4f vs %s" % (cname, name, med[i], min(ms[cname, i]), med[i] / med[0], names[0]), flush=True)
        if noise:
            x, y = med[noise[0]], med[noise[1]]
            floor, slower = abs(x - y) / min(x, y), max(x, y)
            for i, name in enumerate(names):
                if i not in noise:
                    print("%-40s %-9s x%.4f of the slower copy, noise floor %.4f: %s" %
                          (cname, name, med[i] / slower, floor, "passes" if med[i] <= slower * (1.0 + floor) else "SLOWER"), flush=True)
    for pt in pts:
        pt.bind_denoised(None)
        pt.bind_half(None)
        pt.bind_variance(None)
        for k in guides:
            pt.bind_gbuffer(k, None)
        pt.set_stream(0)
        pt.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--libs", required=True)
    ap.add_argument("--part", default="bits,time")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--noise", default=None, help="two names of --libs that are copies of one build")
    a = ap.parse_args()
    srt = importlib.import_module("software-raytracer_amd")
    libs = []
    for item in a.libs.split(","):
        name, path = item.split("=")
        libs.append((name, srt.capi.open_library(os.path.join(ROOT, path))))
    differ = compare_bits(srt, libs) if "bits" in a.part.split(",") else 0
    if "time" in a.part.split(","):
        time_calls(srt, libs, a)
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
