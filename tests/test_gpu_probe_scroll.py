"""The scrolling probe grid (srt_scroll_probes, ABI 7) on the MI355X.  Every comparison of bits is against
tests/probe_scroll_reference.py: grids of 30, 12 and 1005 probes (the last more than one workgroup's waves: what shows a move done
in place), R = 4 and 16, every shift class, the `which` bits singly and together, histories own and bound, a sentinel border around
every caller-owned buffer, the work record; the grid rule through srt_shade_probe_grid; the per-frame loop across a scroll; errors in
order; what keeping the history buys; the layers above."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import probe_grid_reference as PG
import probe_scroll_reference as SC
import probe_update_reference as PU
from conftest import ROOT, scene_path

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
W, H = 24, 20
SENTINEL = -7.0
BORDER = 3
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
GRIDS = [(5, 3, 2), (4, 1, 3), (67, 5, 3)]
# what tests 3, 5 and 6 run on: 100 probes over Scene_indirect, as tests/test_gpu_probe_update.py's grid; origin and spacing dyadic
LOOP_GRID = PG.Grid((-2.5, -1.0, 0.5), (1.25, 0.75, 1.5), (5, 4, 5))
# test 5: measured on an MI355X, one run (profiles/probe_scroll/probe_scroll_quality.jsonl), and the bound halfway between it and 1
MEASURED_RATIO = 0.266
RATIO_BOUND = 0.633


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(U), b.view(U))


def indirect(srt, oracle, w=W, h=H):
    objs = oracle.load_scene_json_py(scene_path("Scene_indirect"))
    oarr, n = oracle.make_objects(objs)
    pt = srt.PathTracer(w, h)
    pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
    pt.set_camera(srt.default_camera())
    pt._keep = oarr
    return pt


@pytest.fixture(scope="module")
def tracer(srt, oracle):
    pt = indirect(srt, oracle)
    yield pt
    pt.close()


def shifts_of(counts):
    """Each axis +-1 alone, a mixed shift, |s| = n - 1, n, n + 1 on one axis, the int32 extremes on one axis, and 0."""
    out = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, -2, 1)]
    n = counts[0]
    out += [(n - 1, 0, 0), (-(n - 1), 0, 0), (n, 0, 0), (-n, 0, 0), (n + 1, 0, 0), (0, 0, -(counts[2] + 1))]
    out += [(I32_MIN, 0, 0), (0, I32_MAX, 0), (I32_MAX, I32_MIN, I32_MAX), (0, 0, 0)]
    return out


def filled(P, n, seed):
    """(P, n, 4) float32, every element distinct, with a quiet NaN with a payload, a negative NaN, a signalling NaN and a -0.0."""
    a = (np.arange(P * n * 4, dtype=np.float64) * 0.25 + 1.0 + seed).astype(F).reshape(P, n, 4)
    assert np.unique(a).shape[0] == a.size
    a.view(U)[P // 2, n // 2] = [0x7FC01234, 0xFFC00001, 0x7F800001, 0x80000000]
    a.view(U)[P - 1, n - 1, 1] = 0x80000000
    return a


def records(P, seed):
    rng = np.random.default_rng(seed)
    rec = PU.records_of(rng.integers(0, 16, P).astype(U), rng.uniform(-0.3, 0.3, (P, 3)))
    rec.view(U)[P // 3, 0] = 0x7FC00055  # (a record's bits move like any others)
    return rec


class Bound:
    """A caller's device buffer of `rows` float4 with BORDER sentinel rows behind it."""

    def __init__(self, torch, dev, rows):
        self.torch, self.rows = torch, rows
        self.t = torch.full((rows + BORDER, 4), SENTINEL, dtype=torch.float32, device=dev)

    def put(self, a):
        self.t[:self.rows].copy_(self.torch.from_numpy(np.ascontiguousarray(a).reshape(-1, 4)))
        self.torch.cuda.synchronize()

    def get(self, shape):
        g = self.t.cpu().numpy()
        assert np.all(g[self.rows:] == F(SENTINEL)), "the border behind the buffer was written"
        return g[:self.rows].reshape(shape)


def waves_ok(work, P):
    return work["waves"] % 4 == 0 and 0 < work["waves"] <= 4 * ((P + 3) // 4)


# ---- 1. bits against the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [4, 16])
@pytest.mark.parametrize("counts", GRIDS)
def test_bound_histories_and_records_against_the_reference(srt, tracer, counts, R):
    import torch

    pt, c = tracer, srt.capi
    grid = PG.Grid((-2.0, -1.0, 1.0), (0.5, 0.5, 0.5), counts)
    P, n = grid.probes, R * R
    dev = "cuda:%d" % pt.device
    Hc, Hm, rec = filled(P, 9, 0), filled(P, n, 7), records(P, P + R)
    th, tm, tr = Bound(torch, dev, P * 9), Bound(torch, dev, P * n), Bound(torch, dev, P)
    pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
    try:
        pt.bind_probe_history("coefficients", th.t)
        pt.bind_probe_history("moments", tm.t)
        pt.reset_probe_history(P, R)
        tr.put(rec)
        pt.bind_probe_grid_states(tr.t[:P])
        seen = dict(retained=0, exposed=0)
        for shift in shifts_of(counts):
            th.put(Hc), tm.put(Hm)
            want = SC.scroll(counts, shift, Hc, Hm, rec)
            for again in range(2 if shift == (1, -2, 1) else 1):  # (the second call scrolls the scrolled arrays)
                pt.scroll_probes(shift, which="all", count_work=True)
                work = pt.probe_scroll_work()
                gc, gm, gp = th.get((P, 9, 4)), tm.get((P, n, 4)), pt.probe_previous_states(P)
                print("%s R %d shift %s: work %s" % (counts, R, shift, work))
                assert same(gc, want["coefficients"]), "coefficients differ at probes %s" % np.flatnonzero((gc.view(U) != want["coefficients"].view(U)).any(axis=(1, 2)))[:8]
                assert same(gm, want["moments"]), "moments differ at probes %s" % np.flatnonzero((gm.view(U) != want["moments"].view(U)).any(axis=(1, 2)))[:8]
                assert same(gp, want["previous"])
                assert same(tr.get((P, 4)), rec)  # the current records are read only
                assert {k: work[k] for k in ("probes", "retained", "exposed")} == want["work"] and work["valid"] == 1 and waves_ok(work, P)
                if again == 0 and shift == (1, -2, 1):
                    want = SC.scroll(counts, shift, want["coefficients"], want["moments"], rec)
            seen["retained"] += want["work"]["retained"]
            seen["exposed"] += want["work"]["exposed"]
        assert seen["retained"] >= P and seen["exposed"] >= P  # the condition on the shifts: both branches of rule SC1 are taken
        # the `which` bits singly: the other arrays keep their bits, the previous records stay what the last call left
        shift = (1, 0, -1) if counts[2] > 1 else (1, 0, 0)
        prev = pt.probe_previous_states(P)
        for which, name in ((c.PROBE_SCROLL_COEFFICIENTS, "coefficients"), (c.PROBE_SCROLL_MOMENTS, "moments"), (c.PROBE_SCROLL_STATES, "states")):
            th.put(Hc), tm.put(Hm)
            pt.scroll_probes(shift, which=which)
            pt.wait()  # (the tensors are read on another stream)
            assert same(th.get((P, 9, 4)), SC.scroll_array(Hc, counts, shift) if name == "coefficients" else Hc), name
            assert same(tm.get((P, n, 4)), SC.scroll_array(Hm, counts, shift) if name == "moments" else Hm), name
            assert same(pt.probe_previous_states(P), SC.scroll_array(rec, counts, shift) if name == "states" else prev), name
            with pytest.raises(srt.SrtError):
                pt.probe_scroll_work()  # the last call did not count
        # shift 0: the histories keep their bits, and _STATES copies the records
        rec2 = records(P, 99)
        tr.put(rec2)
        pt.scroll_probes((0, 0, 0), which="all", count_work=True)
        assert same(th.get((P, 9, 4)), Hc) and same(tm.get((P, n, 4)), Hm) and same(pt.probe_previous_states(P), rec2)
        work = pt.probe_scroll_work()
        assert (work["probes"], work["retained"], work["exposed"]) == (P, P, 0) and waves_ok(work, P)
    finally:
        pt.wait()
        pt.bind_probe_history("coefficients", None)
        pt.bind_probe_history("moments", None)
        pt.bind_probe_grid_states(None)
        pt.bind_probe_previous_states(None)


@pytest.mark.parametrize("counts,R", [((5, 3, 2), 4), ((67, 5, 3), 16)])
def test_own_histories_against_the_reference(srt, tracer, counts, R):
    """The handle's own histories have no write call: they are filled by a blend that restarts every probe (H = N, bits copied)
    from trace outputs bound to tensors that are overwritten from numpy after the trace."""
    import torch

    pt = tracer
    grid = PG.Grid((-2.0, -1.0, 1.0), (0.5, 0.5, 0.5), counts)
    P, n = grid.probes, R * R
    dev = "cuda:%d" % pt.device
    Hc, Hm, rec = filled(P, 9, 3), filled(P, n, 11), records(P, P)
    tc, tm = Bound(torch, dev, P * 9), Bound(torch, dev, P * n)
    pos = srt.probe_grid_positions(grid.origin, grid.spacing, grid.counts)
    pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
    pt.bind_probe_grid_states(rec)
    try:
        pt.bind_light_probe_output("coefficients", tc.t)
        pt.bind_probe_depth_output("moments", tm.t)
        for shift in ((1, -2, 1), (-1, 0, 0), (counts[0] - 1, 0, 0), (0, counts[1], 0), (0, 0, 0), (0, 0, 1), (I32_MAX, 0, 0)):
            pt.trace_light_probes(pos, 1, samples=1, bounces=0)
            pt.trace_probe_depth(resolution=R)
            pt.wait()
            tc.put(Hc), tm.put(Hm)
            pt.reset_probe_history(P, R)
            pt.blend_probes(moments=True)
            assert same(pt.probe_history("coefficients"), Hc) and same(pt.probe_history("moments"), Hm)  # the filling worked
            want = SC.scroll(counts, shift, Hc, Hm, rec)
            pt.scroll_probes(shift, which="all", count_work=True)
            gc, gm = pt.probe_history("coefficients"), pt.probe_history("moments")
            assert same(gc, want["coefficients"]), (shift, np.flatnonzero((gc.view(U) != want["coefficients"].view(U)).any(axis=(1, 2)))[:8])
            assert same(gm, want["moments"]), (shift, np.flatnonzero((gm.view(U) != want["moments"].view(U)).any(axis=(1, 2)))[:8])
            assert same(pt.probe_previous_states(P), want["previous"])
            work = pt.probe_scroll_work()
            assert {k: work[k] for k in ("probes", "retained", "exposed")} == want["work"]
            assert same(tc.get((P, 9, 4)), Hc) and same(tm.get((P, n, 4)), Hm)  # the trace outputs are no part of it
            if shift != (0, 0, 0):  # rule SC5
                with pytest.raises(srt.SrtError) as e:
                    pt.blend_probes(moments=True)
                assert e.value.code == srt.capi.ERR_STATE
            # a second scroll moves what the first left (the spare and the own buffer have changed places)
            pt.scroll_probes((-1, 0, 0), which="both")
            assert same(pt.probe_history("coefficients"), SC.scroll_array(want["coefficients"], counts, (-1, 0, 0)))
            assert same(pt.probe_history("moments"), SC.scroll_array(want["moments"], counts, (-1, 0, 0)))
    finally:
        pt.wait()
        pt.bind_light_probe_output("coefficients", None)
        pt.bind_probe_depth_output("moments", None)
        pt.bind_probe_grid_states(None)
        pt.bind_probe_previous_states(None)


# ---- 2. the grid rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin,spacing", [((-2.5, -1.0, 0.5), (1.25, 0.75, 1.5)), ((-2.45, -1.1, 0.55), (1.2, 0.8, 1.45))], ids=["dyadic", "not_dyadic"])
def test_set_grid_moves_the_origin_by_the_rule(srt, tracer, origin, spacing):
    import torch

    pt = tracer
    counts = (5, 4, 5)
    P = 100
    rng = np.random.default_rng(5)
    co = rng.uniform(0.05, 1.0, (P, 9, 4)).astype(F)
    th = Bound(torch, "cuda:%d" % pt.device, P * 9)
    pt.render_gbuffer()
    try:
        pt.bind_probe_history("coefficients", th.t)
        pt.reset_probe_history(P, which="coefficients")
        pt.set_probe_grid(origin, spacing, counts)
        pt.shade_probe_grid(coefficients=co)
        before = pt.probe_grid_output()
        assert before[..., :3].any()
        for shift in ((1, 0, 0), (-1, 2, -1)):
            pt.set_probe_grid(origin, spacing, counts)
            th.put(co)
            pt.scroll_probes(shift, which="coefficients", set_grid=True)
            pt.shade_probe_grid(coefficients=th.t[:P * 9])
            got = pt.probe_grid_output()
            moved = SC.scrolled_origin(origin, spacing, shift)
            pt.set_probe_grid(tuple(float(v) for v in moved), spacing, counts)
            pt.shade_probe_grid(coefficients=SC.scroll_array(co, counts, shift))
            want = pt.probe_grid_output()
            assert same(got, want), shift
            assert not same(got, before)
            # without the flag the grid stays where it was
            pt.set_probe_grid(origin, spacing, counts)
            th.put(co)
            pt.scroll_probes((0, 0, 0), which="coefficients", set_grid=True)
            pt.scroll_probes(shift, which="coefficients")
            pt.shade_probe_grid(coefficients=co)
            assert same(pt.probe_grid_output(), before)
    finally:
        pt.wait()
        pt.bind_probe_history("coefficients", None)
        pt.L.srt_bind_probe_grid_coefficients(pt._h, None, 0)


# ---- 3. the loop goes on ------------------------------------------------------------------------------------------------------------
def enter(pt, P, K):
    """Classify the handle's grid, make the records and the list current; returns (records, positions, words)."""
    pt.classify_probes(directions=K, relocate=True, positions=True)
    rec, pos = pt.probe_states_output("records"), pt.probe_states_output("positions")
    pt.bind_probe_grid_states(rec)
    pt.list_probes()
    words = pt.probe_list_output(P)
    pt.bind_probe_list(words)
    return rec, pos, words


def test_the_per_frame_loop_goes_on_across_a_scroll(srt, tracer):
    pt, grid, K = tracer, LOOP_GRID, 64
    P, shift = grid.probes, (1, 0, 0)
    try:
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        rec0, pos0, words0 = enter(pt, P, K)
        pt.reset_probe_history(P, which="coefficients")
        for f in range(1, 4):
            pt.trace_light_probes(pos0 if f == 1 else None, None, samples=1, bounces=2, seed=f, listed=True)
            pt.blend_probes(listed=True)
        before = pt.probe_history("coefficients")
        assert before[PU.listed(words0), 0, 3].all()
        # rule SC5's sequence
        pt.scroll_probes(shift, which=("coefficients", "states"), set_grid=True, count_work=True)
        scrolled, prev = SC.scroll_array(before, grid.counts, shift), SC.scroll_array(rec0, grid.counts, shift)
        assert pt.probe_scroll_work()["retained"] == 80
        with pytest.raises(srt.SrtError) as e:
            pt.blend_probes(listed=True)  # the last trace is indexed by the old grid
        assert e.value.code == srt.capi.ERR_STATE
        assert same(pt.probe_history("coefficients"), scrolled) and same(pt.probe_previous_states(P), prev)
        rec1, pos1, words1 = enter(pt, P, K)
        pt.trace_light_probes(pos1, None, samples=1, bounces=2, seed=4, listed=True)
        N = pt.light_probe_coefficients()
        pt.blend_probes(listed=True, previous_states=True, count_work=True)
        got, work = pt.probe_history("coefficients"), pt.probe_blend_work()
        want = PU.blend(scrolled, N, words=words1, states=rec1, previous=prev)
        assert same(got, want["history"])
        # the count, from the reference's map alone: the listed probes that were exposed, had no history, or whose record changed
        retained, source = SC.source_map(grid.counts, shift)
        idx = PU.listed(words1)
        a, b = rec1.view(U), prev.view(U)
        changed = (a[:, :3] != b[:, :3]).any(axis=1) | (((a[:, 3] ^ b[:, 3]) & U(PU.BURIED | PU.IDLE)) != 0)
        empty = np.zeros(P, bool)
        empty[retained] = before[source[retained], 0, 3].view(U) == 0
        restart = ~retained | changed | empty
        print("listed %d: exposed %d, record changed %d, no history %d, restarted %d, work %s" % (
            idx.shape[0], int((~retained)[idx].sum()), int((changed & retained)[idx].sum()), int((empty & ~changed)[idx].sum()), int(restart[idx].sum()), work))
        assert work["restarted"] == int(restart[idx].sum()) == want["work"]["restarted"] and work["probes"] == idx.shape[0]
        kept = idx[~restart[idx]]
        assert kept.shape[0] >= 10 and int((~retained)[idx].sum()) >= 3  # the condition on the inputs: both kinds are listed
        # every retained, unchanged, listed probe: the numpy blend of ITS PRE-SCROLL history with the new trace
        yh, yn = PU.luminance(before[source[kept], 0]), PU.luminance(N[kept, 0])
        d, m = np.abs((yn - yh).astype(F)), np.maximum(np.abs(yh), np.abs(yn))
        h = np.where(d > (F(0.25) * m).astype(F), F(0.5), F(0.9)).astype(F)
        assert same(got[kept], PU.mix(before[source[kept]], N[kept], h))
        assert same(got[idx[~retained[idx]]], N[idx[~retained[idx]]])  # an exposed probe starts over
    finally:
        pt.wait()
        pt.bind_probe_list(None)
        pt.bind_probe_grid_states(None)
        pt.bind_probe_previous_states(None)


# ---- 4. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors_come_in_order_and_touch_nothing(srt, oracle):
    import torch

    c = srt.capi
    objs = oracle.load_scene_json_py(scene_path("Scene_indirect"))
    oarr, n = oracle.make_objects(objs)
    pt = srt.PathTracer(W, H)
    L = pt.L
    grid = PG.Grid((-2.0, -1.0, 1.0), (0.5, 0.5, 0.5), (5, 3, 2))
    P = grid.probes

    def scroll(**kw):
        p = c.ProbeScrollParams()
        assert L.srt_probe_scroll_params_default(C.byref(p)) == c.OK
        p.shift[:] = (1, 0, 0)
        for k, v in kw.items():
            if k in ("reserved", "shift"):
                getattr(p, k)[:] = v
            else:
                setattr(p, k, v)
        return L.srt_scroll_probes(pt._h, C.byref(p))

    def why():
        return L.srt_last_error(pt._h)

    try:
        w = c.ProbeScrollWork()
        buf = np.empty((P, 4), F)
        fp = buf.ctypes.data_as(C.POINTER(C.c_float))
        assert scroll(which=0) == c.ERR_STATE and b"srt_set_scene" in why()  # the scene before the arguments
        pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
        for kw in (dict(which=0), dict(which=8), dict(which=0x80000001), dict(flags=4), dict(flags=0x80000000), dict(reserved=(1, 0, 0)), dict(reserved=(0, 0, 1))):
            assert scroll(**kw) == c.ERR_INVALID_ARG, kw
        assert scroll() == c.ERR_STATE and b"no grid" in why()
        assert scroll(which=0, flags=4) == c.ERR_INVALID_ARG  # the arguments before the grid
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        assert scroll() == c.ERR_STATE and b"no coefficient history" in why()
        th = Bound(torch, "cuda:%d" % pt.device, P * 9)
        Hc = filled(P, 9, 1)
        pt.bind_probe_history("coefficients", th.t)
        pt.reset_probe_history(P - 1, which="coefficients")
        th.put(Hc)
        assert scroll() == c.ERR_STATE and b"probe count" in why()
        pt.reset_probe_history(P, which="coefficients")
        th.put(Hc)
        assert scroll(which=3) == c.ERR_STATE and b"no moment history" in why()
        assert scroll(which=5, flags=3) == c.ERR_STATE and b"no states" in why()
        pt.bind_probe_grid_states(records(P - 1, 1))
        assert scroll(which=5, flags=3) == c.ERR_STATE and b"state count" in why()
        assert scroll(which=4, flags=3) == c.ERR_STATE and b"state count" in why()
        assert scroll(which=5, flags=7) == c.ERR_INVALID_ARG  # still the arguments first
        assert L.srt_scroll_probes(pt._h, None) == c.ERR_INVALID_ARG and L.srt_get_probe_scroll_work(pt._h, None) == c.ERR_INVALID_ARG
        # nothing was touched: the history, the previous records (there are none), the work record (there is none), the grid, and
        # the last trace still counts as the blend's new data
        assert same(th.get((P, 9, 4)), Hc)
        assert L.srt_read_probe_previous_states(pt._h, fp) == c.ERR_STATE and L.srt_get_probe_scroll_work(pt._h, C.byref(w)) == c.ERR_STATE
        pt.classify_probes(positions=True)
        pos = srt.probe_grid_positions(grid.origin, grid.spacing, grid.counts)
        assert same(pt.probe_states_output("positions"), pos)
        pt.trace_light_probes(pos, 1, samples=1, bounces=0)
        assert scroll(which=2) == c.ERR_STATE
        pt.reset_probe_history(P, which="coefficients")
        pt.blend_probes()
        # and a good call goes through
        pt.bind_probe_grid_states(records(P, 1))
        assert scroll(which=5, flags=3) == c.OK and L.srt_get_probe_scroll_work(pt._h, C.byref(w)) == c.OK
        assert (w.valid, w.probes, w.retained, w.exposed) == (1, P, 24, 6)
        pt.wait()
    finally:
        pt.wait()
        pt.bind_probe_history("coefficients", None)
        pt.close()


# ---- 5. what it buys ----------------------------------------------------------------------------------------------------------------
def test_a_scrolled_history_beats_a_reset_one(srt, oracle):
    """Scene_indirect, LOOP_GRID, K = 64, 8 bounces, hysteresis = fast_hysteresis = 0.8: sixteen blended one-sample frames, a scroll
    by one cell along x with the records and the origin, the SC5 sequence and one more frame; against it the route without
    srt_scroll_probes: srt_set_probe_grid on the moved grid, srt_reset_probe_history, the same one frame.  The DC-luminance RMSE over
    the retained probes that the moved grid lists, against a 256-sample trace on the moved grid.  Seventeen independent frames would
    give sqrt(0.8^32 + 0.2 * (1 - 0.8^32) / 1.8) = 0.334 of one frame's error.  tools/probe_scroll_quality.py is the measurement: one
    run on an MI355X gave 0.266 (rmse 0.7815 scrolled against 2.9365 reset, over 78 probes; 20 of the 98 listed probes were exposed
    and restarted), profiles/probe_scroll/probe_scroll_quality.jsonl.  MEASURED_RATIO is that number and RATIO_BOUND = 0.633 lies
    halfway between it and 1, so that the scatter of 78 luminances cannot fail the test while a history that was thrown away (ratio
    1) does."""
    assert abs((0.8 ** 32 + 0.2 * (1 - 0.8 ** 32) / 1.8) ** 0.5 - 0.334) < 1e-3 and abs((MEASURED_RATIO + 1) / 2 - RATIO_BOUND) < 1e-9
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import probe_scroll_quality as Q

    pt = indirect(srt, oracle)
    try:
        r = Q.measure(srt, pt, LOOP_GRID)
        print("retained active probes %d: rmse scrolled %.5f, reset %.5f, ratio %.4f (measured %s, bound %s)" % (
            r["probes_compared"], r["rmse_scrolled"], r["rmse_reset"], r["ratio"], MEASURED_RATIO, RATIO_BOUND))
        assert r["probes_compared"] >= 20
        assert r["ratio"] <= RATIO_BOUND
    finally:
        pt.close()


# ---- 6. the layers above ------------------------------------------------------------------------------------------------------------
def test_host_library_and_cli_give_the_bytes_of_the_c_calls(srt, oracle, tmp_path):
    grid, K = LOOP_GRID, 64
    P = grid.probes
    point = (1.5, 0.6, 3.5)  # the grid's centre is (0, 0.125, 3.5) and a cell 1.25 x 0.75 x 1.5: one cell off along x, none along y and z
    pt = indirect(srt, oracle)
    try:
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        rec0, pos0, _ = enter(pt, P, K)
        pt.reset_probe_history(P, which="coefficients")
        for f in (1, 2):
            pt.trace_light_probes(pos0 if f == 1 else None, None, samples=2, bounces=2, seed=f, listed=True)
            pt.blend_probes(listed=True)
        g = srt.capi.probe_grid(grid.origin, grid.spacing, grid.counts)
        shift = pt.probe_grid_follow(g, point, which=("coefficients", "states"), count_work=True)
        assert shift == (1, 0, 0) == SC.follow(grid.origin, grid.spacing, grid.counts, point)
        swork = pt.probe_scroll_work()
        rec1, pos1, words1 = enter(pt, P, K)
        pt.trace_light_probes(pos1, None, samples=2, bounces=2, seed=3, listed=True)
        pt.blend_probes(listed=True, previous_states=True, count_work=True)
        hist, bwork = pt.probe_history("coefficients"), pt.probe_blend_work()
        assert 0 < bwork["restarted"] < bwork["probes"]
    finally:
        pt.close()
    r = srt.host.Renderer(W, H)
    try:
        r.set_scene(srt.host.Scene(scene_path("Scene_indirect")))
        r.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        hrec, hpos = r.classify_probes(P, K, relocate=True, positions=True)
        assert same(hrec, rec0) and same(hpos, pos0)
        r.list_probes(hrec)
        r.reset_probe_history(P)
        for f in (1, 2):
            r.trace_light_probes_listed(hpos if f == 1 else None, K if f == 1 else None, samples=2, bounces=2, seed=f)
            r.blend_probes(listed=True)
        assert r.follow_probe_grid(point) == shift
        hrec1, hpos1 = r.classify_probes(P, K, relocate=True, positions=True)
        assert same(hrec1, rec1) and same(hpos1, pos1)
        assert same(r.list_probes(hrec1), words1)
        r.trace_light_probes_listed(hpos1, None, samples=2, bounces=2, seed=3)
        r.blend_probes(listed=True, previous_states=True, count_work=True)
        assert same(r.probe_history("coefficients"), hist) and r.probe_blend_work() == bwork
        # scroll_probes by hand gives the same record as the counting follow above
        r.scroll_probes((0, 0, 0), which="states", count_work=True)
        assert r.probe_scroll_work()["probes"] == swork["probes"] == P and swork["retained"] == 80
    finally:
        r.close()
    # the command line: three feedback rounds, the grid moved by (1, 0, -1) after round 2
    cshift, rounds, after = (1, 0, -1), 3, 2
    pt = indirect(srt, oracle)
    try:
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        origin = grid.origin
        pos = srt.probe_grid_positions(origin, grid.spacing, grid.counts)
        pt.set_probe_grid(origin, grid.spacing, grid.counts)
        pt.reset_probe_history(P, which="coefficients")
        for f in range(1, rounds + 1):
            if f > 1:
                pt._ck(pt.L.srt_write_probe_grid_coefficients(pt._h, fp(pt.probe_history("coefficients")), P))
            pt.probe_tail(enabled=f > 1, count_work=True)
            pt.trace_light_probes(pos, K, samples=16, bounces=1, seed=f)
            pt.blend_probes()
            if f == after:
                pt.scroll_probes(cshift, which="coefficients", set_grid=True, count_work=True)
                cwork = pt.probe_scroll_work()
                origin = tuple(float(v) for v in SC.scrolled_origin(origin, grid.spacing, cshift))
                pos = srt.probe_grid_positions(origin, grid.spacing, grid.counts)
        pt.probe_tail(enabled=False)
        history = pt.probe_history("coefficients")
        pt.render_gbuffer()
        pt.set_probe_grid(origin, grid.spacing, grid.counts)
        pt.shade_probe_grid(coefficients=history)
        image = pt.probe_grid_output()
    finally:
        pt.close()
    cli = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
    img = tmp_path / "irradiance.f32"
    gridarg = ",".join([repr(float(v)) for v in list(grid.origin) + list(grid.spacing)] + [str(int(v)) for v in grid.counts])
    run = subprocess.run([cli, "--scene", scene_path("Scene_indirect"), "--width", str(W), "--height", str(H), "--probe-grid", gridarg, "--probe-directions", str(K),
                          "--probe-feedback", str(rounds), "--probe-bounces", "1", "--probe-scroll", "%d,%d,%d" % cshift, "--probe-scroll-after", str(after),
                          "--irradiance-out", str(img)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "probe scroll after round 2 by 1,0,-1: %d probes, %d retained, %d exposed" % (P, cwork["retained"], cwork["exposed"]) in run.stderr
    assert img.read_bytes() == image.tobytes()
