#!/usr/bin/env python3
"""What a scrolled history is worth (srt_scroll_probes) on an MI355X — one JSON line.

Scene_indirect at 24 x 20, the grid of tests/test_gpu_probe_scroll.py's loop tests (origin -2.5 -1 0.5, spacing 1.25 0.75 1.5, 5 x 4 x 5
probes), a relocating classification, the list of active probes, --directions (64) directions, --bounces (8), hysteresis =
fast_hysteresis = --hysteresis (0.8: change detection does not act).  --frames (16) frames of one listed one-sample trace (seed = the
frame) are blended from a reset history.  Then the grid moves by --shift (1, 0, 0):

    scrolled   srt_scroll_probes with COEFFICIENTS | STATES and SET_GRID, srt_classify_probes, the records and the list made current,
               one listed one-sample trace (seed = frames + 1), srt_blend_probes with LISTED | PREVIOUS_STATES
    reset      what there was before: srt_set_probe_grid on the moved grid, srt_reset_probe_history, the same trace, srt_blend_probes
               with LISTED

The yardstick is one trace of --reference (256) samples at the moved grid's positions.  Reported: the RMSE of the DC luminance
(Rec. 709 of coefficient 0) over the retained probes (rule SC1) that the moved grid lists, for both routes, and their ratio; the
probes compared, those of them whose record changed (they restart under either route), and the blend's work record.

    python tools/probe_scroll_quality.py --out profiles/probe_scroll/probe_scroll_quality.jsonl

The line goes to stdout, or is appended to --out FILE.  One run; GPU box only."""
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
import probe_grid_reference as PG  # noqa: E402
import probe_scroll_reference as SC  # noqa: E402
import probe_update_reference as PU  # noqa: E402

GRID = PG.Grid((-2.5, -1.0, 0.5), (1.25, 0.75, 1.5), (5, 4, 5))


def enter(pt, P, K):
    """Classify the handle's grid and make the records and the list current; returns (records, positions, words)."""
    pt.classify_probes(directions=K, relocate=True, positions=True)
    rec, pos = pt.probe_states_output("records"), pt.probe_states_output("positions")
    pt.bind_probe_grid_states(rec)
    pt.list_probes()
    words = pt.probe_list_output(P)
    pt.bind_probe_list(words)
    return rec, pos, words


def measure(srt, pt, grid=GRID, shift=(1, 0, 0), frames=16, directions=64, bounces=8, hysteresis=0.8, reference=256):
    """See the module's docstring; `pt` has its scene set.  Returns a dict."""
    P, K, hy = grid.probes, directions, hysteresis
    try:
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        rec0, pos0, words0 = enter(pt, P, K)
        pt.reset_probe_history(P, which="coefficients")
        for f in range(1, frames + 1):
            pt.trace_light_probes(pos0 if f == 1 else None, None, samples=1, bounces=bounces, seed=f, listed=True)
            pt.blend_probes(hysteresis=hy, fast_hysteresis=hy, listed=True)
        # the scrolled route
        pt.scroll_probes(shift, which=("coefficients", "states"), set_grid=True, count_work=True)
        swork = pt.probe_scroll_work()
        rec1, pos1, words1 = enter(pt, P, K)
        prev = pt.probe_previous_states(P)
        pt.trace_light_probes(pos1, None, samples=1, bounces=bounces, seed=frames + 1, listed=True)
        pt.blend_probes(hysteresis=hy, fast_hysteresis=hy, listed=True, previous_states=True, count_work=True)
        scrolled, bwork = pt.probe_history("coefficients"), pt.probe_blend_work()
        # the yardstick
        pt.trace_light_probes(pos1, None, samples=reference, bounces=bounces, seed=1000)
        truth = pt.light_probe_coefficients()
        # the reset route
        moved = tuple(float(v) for v in SC.scrolled_origin(grid.origin, grid.spacing, shift))
        pt.set_probe_grid(moved, grid.spacing, grid.counts)
        pt.reset_probe_history(P, which="coefficients")
        pt.trace_light_probes(pos1, None, samples=1, bounces=bounces, seed=frames + 1, listed=True)
        pt.blend_probes(hysteresis=hy, fast_hysteresis=hy, listed=True)
        reset = pt.probe_history("coefficients")
    finally:
        pt.wait()
        pt.bind_probe_list(None)
        pt.bind_probe_grid_states(None)
        pt.bind_probe_previous_states(None)
    retained, _ = SC.source_map(grid.counts, shift)
    listed = PU.listed(words1)
    idx = listed[retained[listed]]
    a, b = rec1.view(np.uint32), prev.view(np.uint32)
    changed = (a[:, :3] != b[:, :3]).any(axis=1) | (((a[:, 3] ^ b[:, 3]) & np.uint32(PU.BURIED | PU.IDLE)) != 0)
    y = lambda v: PU.luminance(v[idx, 0]).astype(np.float64)
    rmse = lambda v: float(np.sqrt(np.mean((y(v) - y(truth)) ** 2)))
    e_s, e_r = rmse(scrolled), rmse(reset)
    return dict(probes=P, listed_before=int(words0[0]), listed_after=int(words1[0]), probes_compared=int(idx.shape[0]),
                compared_with_changed_record=int(changed[idx].sum()), scroll_work=swork, blend_work=bwork, rmse_scrolled=e_s, rmse_reset=e_r,
                ratio=e_s / e_r if e_r > 0 else None)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="Scene_indirect")
    ap.add_argument("--shift", default="1,0,0")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--directions", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--hysteresis", type=float, default=0.8)
    ap.add_argument("--reference", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from probe_depth_time import open_tracer

    srt = importlib.import_module("software-raytracer_amd")
    pt, _ = open_tracer(srt, a.scene, 24, 20)
    shift = tuple(int(v) for v in a.shift.split(","))
    r = measure(srt, pt, GRID, shift, a.frames, a.directions, a.bounces, a.hysteresis, a.reference)
    pt.close()
    line = dict(tool="probe_scroll_quality", device=torch.cuda.get_device_name(0), scene=a.scene, grid_origin=[float(v) for v in GRID.origin], grid_spacing=[float(v) for v in GRID.spacing],
                grid_counts=[int(v) for v in GRID.counts], shift=list(shift), frames=a.frames, directions=a.directions, bounces=a.bounces, hysteresis=a.hysteresis,
                reference_samples=a.reference, runs=1, **r)
    text = json.dumps(line) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
