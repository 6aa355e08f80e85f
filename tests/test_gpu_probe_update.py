"""The list of active probes and the hysteresis blend (srt_list_probes, srt_blend_probes, ABI 7) on the MI355X.  Every comparison is
bit for bit against tests/probe_update_reference.py: lists of 1 .. 8925 records around the wave, the workgroup and the chunk sizes,
all listed / none / alternating / the synthetic room's classification, another skip_mask, a bound output with a sentinel border and
repeated calls; the blend at R = 4, 8 and 16 with and without the moments, the list and the previous records, its work record, its
restarts, the histories own and bound; errors in order."""
import ctypes as C

import numpy as np
import pytest

import probe_grid_reference as PG
import probe_states_reference as PS
import probe_update_reference as PU
from test_gpu_probe_states import tracer
from test_gpu_visibility import scene1

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
WORD_SENTINEL = 0x5A5A5A5A
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 8925]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(U), b.view(U))


@pytest.fixture(scope="module")
def room(srt, oracle):
    objs = PS.synthetic_room()
    pt = tracer(srt, oracle, (objs, None))
    yield pt, objs
    pt.close()


@pytest.fixture(scope="module")
def plain(srt, oracle):
    """A tracer with a scene and no grid: srt_list_probes then takes any number of records."""
    pt = tracer(srt, oracle, (PS.synthetic_room(), None))
    yield pt
    pt.close()


@pytest.fixture(scope="module")
def lit(srt, oracle):
    """Scene1 under its sky (the room is closed and dark: every radiance there is 0) and a grid of 100 probes over it."""
    objs, _ = scene1(oracle)
    pt = tracer(srt, oracle, (objs, None))
    yield pt, objs, PG.Grid((-4.0, -1.5, 1.0), (1.0, 1.0, 1.0), (5, 4, 5))
    pt.close()


def record_sets(P):
    rng = np.random.default_rng(P)
    offsets = rng.uniform(-0.2, 0.2, (P, 3))
    yield "all", PU.records_of(np.zeros(P, U), offsets)
    yield "none", PU.records_of(np.full(P, PU.BURIED | PU.INSIDE, U), offsets)
    yield "alternating", PU.records_of(np.where(np.arange(P) % 2 == 0, 0, PU.IDLE).astype(U), offsets)
    yield "random", PU.records_of(rng.integers(0, 16, P).astype(U), offsets)


# ---- the list ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", SIZES)
def test_lists_of_every_size_against_the_reference(srt, plain, P):
    pt = plain
    for name, rec in record_sets(P):
        want = PU.probe_list(rec)
        pt.bind_probe_grid_states(rec)
        pt.list_probes(count_work=True)
        got, work = pt.probe_list_output(P), pt.probe_list_work()
        print("P %d %s: listed %d, work %s" % (P, name, want[0], work))
        assert same(got, want), "%s: differs at words %s" % (name, np.flatnonzero(got != want)[:8])
        assert work == dict(valid=1, probes=P, listed=int(want[0]), waves=4)
    # another skip mask, on the random records; counting off; the same call twice
    for mask in (0, PU.MOVED, PU.INSIDE | PU.IDLE, PU.STATE_BITS):
        want = PU.probe_list(rec, mask)
        for _ in range(2):
            pt.list_probes(skip_mask=mask)
            assert same(pt.probe_list_output(P), want), mask
    with pytest.raises(srt.SrtError):
        pt.probe_list_work()  # the last call did not count


def test_the_rooms_classification_listed_into_a_bound_buffer_with_a_sentinel_border(srt, room):
    import torch

    pt, objs = room
    grid = PS.room_grid()
    P = grid.probes
    pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
    dev = "cuda:%d" % pt.device
    rec_t = torch.zeros((P, 4), dtype=torch.float32, device=dev)
    out = torch.full((4 + P + 9,), WORD_SENTINEL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    try:
        pt.bind_probe_states_output("records", rec_t)
        pt.classify_probes(directions=64, relocate=True)
        pt.bind_probe_grid_states(rec_t)  # device to device: no copy
        want_rec = PS.classify(grid, objs, srt.light_probe_sphere(64), PS.RELOCATE)["records"]
        want = PU.probe_list(want_rec)
        assert 5 <= want[0] <= P - 5
        for _ in range(2):
            pt.list_probes(output=out, count_work=True)
            pt.wait()
            g = out.cpu().numpy().view(U)
            assert same(g[:4 + P], want) and np.all(g[4 + P:] == WORD_SENTINEL)
            assert same(pt.probe_list_output(P), want) and pt.probe_list_work()["listed"] == int(want[0])
        # a state count other than the grid's is refused, and nothing is touched
        pt.bind_probe_grid_states(want_rec[:P - 1])
        out.fill_(WORD_SENTINEL)
        torch.cuda.synchronize()
        with pytest.raises(srt.SrtError):
            pt.list_probes()
        pt.wait()
        assert np.all(out.cpu().numpy().view(U) == WORD_SENTINEL)
    finally:
        pt.wait()
        pt.bind_probe_states_output("records", None)
        pt.bind_probe_list_output(None)
        pt.bind_probe_grid_states(None)
    # back on the own buffer
    pt.bind_probe_grid_states(want_rec)
    pt.list_probes()
    assert same(pt.probe_list_output(P), want)


# ---- the blend --------------------------------------------------------------------------------------------------------------------
def perturbed(N, seed, zero_every=7):
    """A history next to the new data N: each probe scaled by a factor around the change threshold; every `zero_every`-th is empty."""
    rng = np.random.default_rng(seed)
    H = (N * rng.uniform(0.6, 1.5, (N.shape[0], 1, 1))).astype(F)
    H += rng.uniform(-0.01, 0.01, N.shape).astype(F)
    H[::zero_every] = 0.0
    return H


def previous_of(rec, seed):
    """Records that differ from `rec` at some probes: an offset lane, the BURIED bit, the IDLE bit, or only bits that do not count."""
    rng = np.random.default_rng(seed)
    prev = rec.copy()
    pick = rng.integers(0, 8, rec.shape[0])
    prev[pick == 0, 0] += F(0.125)
    st = PU.state_bits(prev)
    st = np.where(pick == 1, st ^ PU.BURIED, np.where(pick == 2, st ^ PU.IDLE, np.where(pick == 3, st ^ (PU.MOVED | PU.INSIDE), st))).astype(U)
    prev[:, 3] = st.view(F)
    return prev


@pytest.mark.parametrize("R", [4, 8, 16])
def test_the_blend_against_the_reference_with_every_flag_combination(srt, lit, R):
    import torch

    pt, objs, grid = lit
    P = grid.probes
    d = srt.light_probe_sphere(64)
    rec = PS.classify(grid, objs, d, PS.RELOCATE)["records"]
    pos = PS.classify(grid, objs, d, PS.RELOCATE)["positions"]
    words = PU.probe_list(rec)
    assert 5 <= words[0] <= P - 5
    prev = previous_of(rec, R)
    pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
    pt.trace_light_probes(pos, d, samples=2, bounces=3, seed=R)
    pt.trace_probe_depth(resolution=R, sharpness=3, max_distance=4.0)
    N, DN = pt.light_probe_coefficients(), pt.probe_depth_output("moments")
    H, DH = perturbed(N, R), perturbed(DN, R + 1, 5)
    dev = "cuda:%d" % pt.device
    th = torch.zeros((P * 9 + 3, 4), dtype=torch.float32, device=dev)
    tdh = torch.zeros((P * R * R + 3, 4), dtype=torch.float32, device=dev)
    pt.bind_probe_grid_states(rec)
    pt.bind_probe_previous_states(prev)
    pt.bind_probe_list(words)
    try:
        pt.bind_probe_history("coefficients", th)
        pt.bind_probe_history("moments", tdh)
        pt.reset_probe_history(P, R)
        pt.wait()
        assert not th.cpu().numpy().any() and not tdh.cpu().numpy().any()
        seen = dict(restarted=0, changed=0, kept=0)
        for moments in (False, True):
            for listed in (False, True):
                for previous in (False, True):
                    th[:P * 9].copy_(torch.from_numpy(H.reshape(-1, 4)))
                    tdh[:P * R * R].copy_(torch.from_numpy(DH.reshape(-1, 4)))
                    th[P * 9:] = -7.0
                    tdh[P * R * R:] = -7.0
                    torch.cuda.synchronize()
                    want = PU.blend(H, N, DH if moments else None, DN if moments else None, words=words if listed else None,
                                    states=rec if previous else None, previous=prev if previous else None, hysteresis=F(0.9), fast_hysteresis=F(0.5),
                                    depth_hysteresis=F(0.8), change_threshold=F(0.25))
                    pt.blend_probes(depth_hysteresis=0.8, moments=moments, listed=listed, previous_states=previous, count_work=True)
                    got, gotd, work = pt.probe_history("coefficients"), pt.probe_history("moments"), pt.probe_blend_work()
                    print("R %d moments %d listed %d previous %d: work %s" % (R, moments, listed, previous, work))
                    assert same(got, want["history"]), "coefficients differ at probes %s" % np.flatnonzero((got.view(U) != want["history"].view(U)).any(axis=(1, 2)))[:8]
                    assert same(gotd, want["depth_history"] if moments else DH)
                    assert work["valid"] == 1 and work["waves"] > 0 and {k: work[k] for k in ("probes", "restarted", "changed")} == want["work"]
                    assert np.all(th[P * 9:].cpu().numpy() == -7.0) and np.all(tdh[P * R * R:].cpu().numpy() == -7.0)
                    if listed:  # unlisted probes' history is untouched
                        skipped = np.setdiff1d(np.arange(P), PU.listed(words))
                        assert same(got[skipped], H[skipped]) and same(gotd[skipped], DH[skipped])
                    seen["restarted"] += want["work"]["restarted"]
                    seen["changed"] += want["work"]["changed"]
                    seen["kept"] += want["work"]["probes"] - want["work"]["restarted"] - want["work"]["changed"]
        assert min(seen.values()) >= 8, seen  # the condition on the inputs: every branch of rules U2 and U3 is taken
        # other parameters: h = 0 gives the new data; counting off changes no bit
        th[:P * 9].copy_(torch.from_numpy(H.reshape(-1, 4)))
        torch.cuda.synchronize()
        pt.blend_probes(hysteresis=0.0, fast_hysteresis=0.0)
        keep = H[:, 0, 3].view(U) != 0
        assert np.array_equal(pt.probe_history("coefficients")[keep], N[keep])
        with pytest.raises(srt.SrtError):
            pt.probe_blend_work()
    finally:
        pt.wait()
        pt.bind_probe_history("coefficients", None)
        pt.bind_probe_history("moments", None)
        pt.bind_probe_list(None)
        pt.bind_probe_grid_states(None)
        pt.bind_probe_previous_states(None)


def test_own_histories_restart_after_a_reset_and_then_blend(srt, lit):
    pt, objs, grid = lit
    P = grid.probes
    d = srt.light_probe_sphere(65)
    pos = PS.classify(grid, objs)["positions"]
    pt.reset_probe_history(P, 8)
    assert not pt.probe_history("coefficients").any() and not pt.probe_history("moments").any()
    frames = []
    H = np.zeros((P, 9, 4), F)
    DH = np.zeros((P, 64, 4), F)
    for f in range(1, 4):
        pt.trace_light_probes(pos, d, samples=1, bounces=3, seed=f)
        pt.trace_probe_depth(resolution=8, sharpness=3, max_distance=4.0 + f)
        N, DN = pt.light_probe_coefficients(), pt.probe_depth_output("moments")
        want = PU.blend(H, N, DH, DN, hysteresis=F(0.8), fast_hysteresis=F(0.8), depth_hysteresis=F(0.5))
        pt.blend_probes(hysteresis=0.8, fast_hysteresis=0.8, depth_hysteresis=0.5, moments=True, count_work=True)
        H, DH = pt.probe_history("coefficients"), pt.probe_history("moments")
        assert same(H, want["history"]) and same(DH, want["depth_history"])
        assert pt.probe_blend_work()["restarted"] == (P if f == 1 else 0)
        frames.append(N)
    assert frames[2][:, 0, :3].any() and not same(H, frames[2])  # (light reaches the probes, and the history is not just the last frame)
    # the history is what the shading binds: a reset of the coefficients alone leaves the moments
    pt.reset_probe_history(P, which="coefficients")
    assert not pt.probe_history("coefficients").any() and same(pt.probe_history("moments"), DH)
    # the new data must be the last trace's, for the history's probe count
    pt.trace_light_probes(pos[:P - 1], d, samples=1, bounces=1)
    with pytest.raises(srt.SrtError):
        pt.blend_probes()
    pt.trace_light_probes(pos, d, samples=1, bounces=1, coefficients=False, radiance=True)
    with pytest.raises(srt.SrtError):
        pt.blend_probes()
    pt.trace_light_probes(pos, d, samples=1, bounces=1)
    pt.trace_probe_depth(resolution=4)
    with pytest.raises(srt.SrtError):
        pt.blend_probes(moments=True)  # another R than the history's
    pt.blend_probes()
    assert same(pt.probe_history("coefficients"), pt.light_probe_coefficients())


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_errors_come_in_order_and_touch_nothing(srt, oracle):
    c = srt.capi
    objs = PS.synthetic_room()
    oarr, n = oracle.make_objects(objs)
    pt = srt.PathTracer(24, 20)
    L = pt.L
    nan, inf = float("nan"), float("inf")

    def lst(**kw):
        p = c.ProbeListParams()
        assert L.srt_probe_list_params_default(C.byref(p)) == c.OK
        for k, v in kw.items():
            if k == "reserved":
                p.reserved[:] = v
            else:
                setattr(p, k, v)
        return L.srt_list_probes(pt._h, C.byref(p))

    def blend(**kw):
        p = c.ProbeBlendParams()
        assert L.srt_probe_blend_params_default(C.byref(p)) == c.OK
        for k, v in kw.items():
            setattr(p, k, v)
        return L.srt_blend_probes(pt._h, C.byref(p))

    def why():
        return L.srt_last_error(pt._h)

    try:
        assert lst(flags=2) == c.ERR_STATE and b"srt_set_scene" in why()
        assert blend(flags=16) == c.ERR_STATE and b"srt_set_scene" in why()
        pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
        for kw in (dict(flags=2), dict(flags=0x80000000), dict(skip_mask=16), dict(skip_mask=0xFFFFFFFF), dict(reserved=(1, 0)), dict(reserved=(0, 1))):
            assert lst(**kw) == c.ERR_INVALID_ARG, kw
        assert lst() == c.ERR_STATE and b"no states" in why()
        words = np.empty(64, U)
        assert L.srt_read_probe_list_output(pt._h, words.ctypes.data_as(C.POINTER(C.c_uint32))) == c.ERR_STATE
        w = c.ProbeListWork()
        assert L.srt_get_probe_list_work(pt._h, C.byref(w)) == c.ERR_STATE
        for kw in (dict(flags=16), dict(hysteresis=1.0), dict(hysteresis=-0.1), dict(hysteresis=nan), dict(fast_hysteresis=1.0), dict(fast_hysteresis=nan),
                   dict(depth_hysteresis=1.5), dict(depth_hysteresis=-inf), dict(change_threshold=-1.0), dict(change_threshold=nan), dict(change_threshold=inf),
                   dict(reserved=1)):
            assert blend(**kw) == c.ERR_INVALID_ARG, kw
        assert blend() == c.ERR_STATE and b"no coefficient history" in why()
        assert L.srt_reset_probe_history(pt._h, 0, 60, 8) == c.ERR_INVALID_ARG and L.srt_reset_probe_history(pt._h, 4, 60, 8) == c.ERR_INVALID_ARG
        assert L.srt_reset_probe_history(pt._h, 1, 0, 0) == c.ERR_INVALID_ARG and L.srt_reset_probe_history(pt._h, 3, 60, 5) == c.ERR_INVALID_ARG
        buf = np.empty((60 * 256, 4), F)
        fp = buf.ctypes.data_as(C.POINTER(C.c_float))
        assert L.srt_read_probe_history(pt._h, 1, fp) == c.ERR_STATE and L.srt_read_probe_history(pt._h, 3, fp) == c.ERR_INVALID_ARG
        assert L.srt_bind_probe_history(pt._h, 3, None) == c.ERR_INVALID_ARG and L.srt_bind_probe_history(pt._h, 0, None) == c.ERR_INVALID_ARG
        assert L.srt_reset_probe_history(pt._h, 1, 60, 0) == c.OK
        assert blend() == c.ERR_STATE and b"COEFFICIENTS" in why()
        assert blend(hysteresis=nan) == c.ERR_INVALID_ARG  # the arguments before the inputs
        assert L.srt_read_probe_history(pt._h, 1, fp) == c.OK and not buf[:540].any()
        assert L.srt_read_probe_history(pt._h, 2, fp) == c.ERR_STATE
        # the list inputs
        assert L.srt_bind_probe_list(pt._h, None, 5) == c.ERR_INVALID_ARG and L.srt_write_probe_list(pt._h, None, 5) == c.ERR_INVALID_ARG
        wp = words.ctypes.data_as(C.POINTER(C.c_uint32))
        assert L.srt_write_probe_list(pt._h, wp, 4) == c.ERR_INVALID_ARG and L.srt_write_probe_list(pt._h, wp, 0) == c.ERR_INVALID_ARG
        grid = PS.room_grid(0.9, (4, 3, 5))
        pos = PS.classify(grid, objs)["positions"]
        # the listed traces: the parent's checks first, then the list
        with pytest.raises(srt.SrtError) as e:
            pt.trace_light_probes(pos, 64, samples=0, listed=True)
        assert e.value.code == c.ERR_INVALID_ARG and "srt_trace_light_probes_listed" in str(e.value)
        with pytest.raises(srt.SrtError) as e:
            pt.trace_light_probes(samples=1, listed=True)
        assert e.value.code == c.ERR_STATE and "no list" in str(e.value)
        with pytest.raises(srt.SrtError) as e:
            pt.trace_probe_depth(listed=True)
        assert e.value.code == c.ERR_STATE and "no list" in str(e.value)
        pt.bind_probe_list(PU.probe_list(PU.records_of(np.zeros(59, U))))
        for call in (lambda: pt.trace_light_probes(samples=1, listed=True), lambda: pt.trace_probe_depth(listed=True)):
            with pytest.raises(srt.SrtError) as e:
                call()
            assert e.value.code == c.ERR_STATE and "capacity" in str(e.value)
        with pytest.raises(srt.SrtError):
            pt.light_probe_coefficients(60)  # nothing was traced
        pt.trace_light_probes(samples=1, bounces=1)
        assert blend(flags=c.PROBE_BLEND_LISTED) == c.ERR_STATE and b"capacity" in why()
        assert blend(flags=c.PROBE_BLEND_PREVIOUS_STATES) == c.ERR_STATE and b"no states" in why()
        assert blend(flags=c.PROBE_BLEND_MOMENTS) == c.ERR_STATE and b"no moment history" in why()
        assert blend() == c.OK
        assert L.srt_blend_probes(pt._h, None) == c.ERR_INVALID_ARG and L.srt_list_probes(pt._h, None) == c.ERR_INVALID_ARG
        pt.wait()
    finally:
        pt.close()
