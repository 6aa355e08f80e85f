"""Adaptive sampling (srt_render_adaptive and the sample-count / sample-budget buffers, ABI 7) on the MI355X.  Every comparison is
bit for bit (NaN compares as its bits) with no pixel left out.  The reference for "pixel p after n_p samples" is the CPU oracle
(POW_SHARED) rendered cumulatively, one sample per call, and picked per pixel; srt_render is used alongside it the same way.
24 x 20 makes nine 8 x 8 tiles, the bottom row of tiles four rows high; budgets above 64 cross the kernel's chunk of 64 samples.
Accumulator and framebuffer are bound to torch tensors so that sentinels can be written into both."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path
from test_gpu_radiance import SCENES, Scene, moved_camera, srt_camera
from test_gpu_visibility import closed_room, scene1

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
W, H = 24, 20
N = W * H
SENT_ACC = 0x7FC0BEEF  # a NaN pattern no arithmetic produces
SENT_FB = 0x12345678
LIMIT = 2147483646


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def differing(a, b):
    d = bits(a) != bits(b)
    return int((d.any(axis=-1) if d.ndim == 3 else d).sum())


class Bound:
    """The tracer's accumulator and framebuffer bound to torch tensors."""

    def __init__(self, pt, w, h):
        import torch

        self.torch, self.pt = torch, pt
        dev = "cuda:%d" % pt.device
        self.acc = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
        self.fb = torch.zeros((h, w), dtype=torch.int32, device=dev)
        self.bind()

    def bind(self):
        self.pt.bind_output(self.fb.data_ptr(), self.acc.data_ptr())

    def unbind(self):
        self.pt.bind_output()

    def sentinel(self):
        self.pt.wait()
        self.acc.view(self.torch.int32).fill_(SENT_ACC)
        self.fb.fill_(SENT_FB)
        self.torch.cuda.synchronize()

    def write(self, fb, acc):
        self.pt.wait()
        self.acc.copy_(self.torch.from_numpy(np.ascontiguousarray(acc)))
        self.fb.copy_(self.torch.from_numpy(np.ascontiguousarray(fb).view(np.int32)))
        self.torch.cuda.synchronize()

    def read(self):
        """(framebuffer (h, w) uint32, memory rows; accumulator (h, w, 4) float32, scene rows)"""
        self.pt.wait()
        return self.fb.cpu().numpy().view(np.uint32), self.acc.cpu().numpy()


def sentinels(w=W, h=H):
    acc = np.full((h, w, 4), SENT_ACC, np.uint32).view(np.float32)
    return np.full((h, w), SENT_FB, np.uint32), acc


class Ref:
    """The oracle rendered cumulatively: acc[n], fb[n] after n = 1 .. samples of (camera, bounces, seed)."""

    def __init__(self, s, ocam, bounces, seed):
        self.s, self.ocam, self.bounces, self.seed = s, ocam, bounces, seed
        self.acc, self.fb = [None], [None]

    def upto(self, nmax):
        s = self.s
        while len(self.acc) <= nmax:
            f = len(self.acc)
            fb, acc, _ = s.oracle.render(s.oarr, s.n, s.env, self.ocam, s.w, s.h, spp=1, bounces=self.bounces, seed=self.seed, first_sample=f,
                                         reset=f == 1, accumulator=self.acc[-1], pow_mode=s.oracle.POW_SHARED,
                                         meshes=s.om[:2] if s.om else None, threads=1)
            self.acc.append(acc)
            self.fb.append(fb)

    def at(self, counts, fb0, acc0):
        """(fb, acc): per pixel the oracle after counts[p] samples; where `counts` is 0, (fb0, acc0)."""
        counts = np.asarray(counts)
        self.upto(int(counts.max()))
        fb, acc = fb0.copy(), acc0.copy()
        for n in np.unique(counts):
            if n == 0:
                continue
            m = counts == n  # scene rows; the framebuffer's memory row is H - 1 - y
            acc[m] = self.acc[n][m]
            fb[m[::-1]] = self.fb[n][m[::-1]]
        return fb, acc


def render_at(s, bound, counts, bounces, seed, fb0, acc0):
    """Ref.at with srt_render(1 .. n, RESET) into the tracer's own buffers as the reference."""
    bound.unbind()
    try:
        fb, acc = fb0.copy(), acc0.copy()
        for n in np.unique(counts):
            if n == 0:
                continue
            s.pt.render(spp=int(n), bounces=bounces, seed=seed)
            m = counts == n
            acc[m] = s.pt.accumulator()[m]
            fb[m[::-1]] = s.pt.framebuffer()[m[::-1]]
        return fb, acc
    finally:
        bound.bind()


def check(got, want, what):
    (gfb, gacc), (wfb, wacc) = got, want
    assert same(gacc, wacc), "%s: %d accumulator elements differ" % (what, differing(gacc, wacc))
    assert same(gfb, wfb), "%s: %d framebuffer pixels differ" % (what, differing(gfb, wfb))


def mixed_map(w=W, h=H):
    """Tile (0, 0) cycles through the budgets around the chunk of 64, tile (1, 0) is all zero, the other tiles hold 0..3."""
    b = ((np.arange(w)[None, :] + 2 * np.arange(h)[:, None]) % 4).astype(np.uint32)
    b[0:8, 0:8] = np.resize(np.array([0, 1, 2, 63, 64, 65, 130], np.uint32), 64).reshape(8, 8)
    b[0:8, 8:16] = 0
    return b


@pytest.fixture(scope="module", params=list(SCENES))
def sc(request, srt, oracle):
    s = Scene(srt, oracle, SCENES[request.param](oracle))
    s.name = request.param
    s.bound = Bound(s.pt, W, H)
    yield s
    s.close()


@pytest.fixture(scope="module")
def sc1(srt, oracle):
    s = Scene(srt, oracle, scene1(oracle))
    s.bound = Bound(s.pt, W, H)
    s.ocam = moved_camera(oracle)
    s.pt.set_camera(srt_camera(srt, s.ocam))
    s.refs = {}
    yield s
    s.close()


def ref_of(s, bounces, seed):
    key = (bounces, seed)
    if key not in s.refs:
        s.refs[key] = Ref(s, s.ocam, bounces, seed)
    return s.refs[key]


def start(s, counts, budget, sentinel=True):
    """The state in front of an adaptive call: counts and budget written, sentinels in accumulator and framebuffer."""
    s.pt.write_sample_counts(np.broadcast_to(np.uint32(counts), (s.h, s.w)) if np.isscalar(counts) else counts)
    s.pt.write_sample_budget(np.broadcast_to(np.uint32(budget), (s.h, s.w)) if np.isscalar(budget) else budget)
    if sentinel:
        s.bound.sentinel()


# ---- 1. a uniform budget from n = 0 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,bounces", [(5, 0), (5, 1), (70, 8)])
def test_a_uniform_budget_from_zero_equals_srt_render_and_the_oracle(sc, oracle, srt, k, bounces):
    for ocam, seed in ((oracle.default_camera(), 0), (moved_camera(oracle), 11)):
        sc.pt.set_camera(srt_camera(srt, ocam))
        ofb, oacc, rays = oracle.render(sc.oarr, sc.n, sc.env, ocam, W, H, spp=k, bounces=bounces, seed=seed, pow_mode=oracle.POW_SHARED,
                                        meshes=sc.om[:2] if sc.om else None)
        start(sc, 0, k)
        sc.pt.render_adaptive(bounces=bounces, seed=seed, count_work=True)
        got, work = sc.bound.read(), sc.pt.adaptive_work()
        print("%s k=%d B=%d seed=%d: oracle rays %d, work %s" % (sc.name, k, bounces, seed, rays, work))
        check(got, (ofb, oacc), "against the oracle")
        check(got, render_at(sc, sc.bound, np.full((H, W), k), bounces, seed, *sentinels()), "against srt_render")
        assert (sc.pt.sample_counts() == k).all() and (sc.pt.sample_budget_map() == k).all()
        assert work["valid"] == 1 and work["pixels"] == N and work["samples"] == N * k and work["closest_calls"] == rays
        assert work["wave_calls"] >= 9  # one primary invocation per tile
        if sc.name == "empty" or bounces == 0:
            assert work["wave_calls"] == 9
        # without the work record: the same bits
        start(sc, 0, k)
        sc.pt.render_adaptive(bounces=bounces, seed=seed)
        check(sc.bound.read(), (ofb, oacc), "without COUNT_WORK")


# ---- 2. a mixed map -------------------------------------------------------------------------------------------------------------
def test_a_mixed_map_gives_every_pixel_its_own_count_and_leaves_zero_budgets_alone(sc, oracle, srt):
    ocam, seed, bounces = moved_camera(oracle), 3, 8
    sc.pt.set_camera(srt_camera(srt, ocam))
    b = mixed_map()
    start(sc, 0, b)
    sc.pt.render_adaptive(bounces=bounces, seed=seed, count_work=True)
    got, work = sc.bound.read(), sc.pt.adaptive_work()
    check(got, Ref(sc, ocam, bounces, seed).at(b, *sentinels()), "against the oracle")
    check(got, render_at(sc, sc.bound, b, bounces, seed, *sentinels()), "against srt_render")
    zero = b == 0
    assert (bits(got[1])[zero] == SENT_ACC).all() and (got[0][zero[::-1]] == SENT_FB).all() and zero.sum() >= 64 + 9
    assert np.array_equal(sc.pt.sample_counts(), b) and np.array_equal(sc.pt.sample_budget_map(), b)
    assert work["pixels"] == int((b > 0).sum()) and work["samples"] == int(b.sum())


# ---- 3. continuation ------------------------------------------------------------------------------------------------------------
def test_two_calls_equal_one_call_with_the_sum(sc1):
    b1 = mixed_map()
    b2 = ((3 * np.arange(W)[None, :] + np.arange(H)[:, None]) % 5).astype(np.uint32)
    b2[0:8, 0:8] = 70 - np.minimum(b1[0:8, 0:8], 70)  # (130 + 0, the others up to 70: chunks that start inside a chunk)
    start(sc1, 0, b1)
    sc1.pt.render_adaptive(bounces=8, seed=5)
    sc1.pt.write_sample_budget(b2)
    sc1.pt.render_adaptive(bounces=8, seed=5)
    two = sc1.bound.read()
    assert np.array_equal(sc1.pt.sample_counts(), b1 + b2)
    start(sc1, 0, b1 + b2)
    sc1.pt.render_adaptive(bounces=8, seed=5)
    check(two, sc1.bound.read(), "two calls against one")
    check(two, ref_of(sc1, 8, 5).at(b1 + b2, *sentinels()), "against the oracle")


def test_a_uniform_srt_render_continues_through_set_sample_counts(sc1):
    b = mixed_map()
    sc1.bound.sentinel()
    sc1.pt.render(spp=7, bounces=8, seed=5)
    base = sc1.bound.read()
    check(base, ref_of(sc1, 8, 5).at(np.full((H, W), 7), *sentinels()), "srt_render(1..7)")
    sc1.pt.set_sample_counts(7)
    sc1.pt.write_sample_budget(b)
    sc1.pt.render_adaptive(bounces=8, seed=5)
    check(sc1.bound.read(), ref_of(sc1, 8, 5).at(7 + b, *sentinels()), "7 + b_p")
    assert np.array_equal(sc1.pt.sample_counts(), 7 + b)


# ---- 4. max_samples, KEEP_COUNTS, two accumulators ------------------------------------------------------------------------------
def test_max_samples_clamps_and_keep_counts_only_reads_the_counts(sc1):
    start(sc1, 0, 100)
    sc1.pt.render_adaptive(bounces=4, seed=2, max_samples=9)
    want = ref_of(sc1, 4, 2).at(np.full((H, W), 9), *sentinels())
    check(sc1.bound.read(), want, "budget 100, max_samples 9")
    assert (sc1.pt.sample_counts() == 9).all() and (sc1.pt.sample_budget_map() == 100).all()
    start(sc1, 0, 9)
    sc1.pt.render_adaptive(bounces=4, seed=2, keep_counts=True)
    check(sc1.bound.read(), want, "KEEP_COUNTS")
    assert (sc1.pt.sample_counts() == 0).all()


def test_two_accumulators_advanced_in_turn_each_equal_their_own_srt_render(sc1):
    import torch

    pt, b = sc1.pt, mixed_map()
    other_acc, other_fb = torch.zeros_like(sc1.bound.acc), torch.zeros_like(sc1.bound.fb)
    want = {}
    for seed in (21, 22):
        want[seed] = render_at(sc1, sc1.bound, 4 + b, 4, seed, *sentinels())
    try:
        # the uniform seed of both halves, then one adaptive round: A with KEEP_COUNTS, then B
        pt.render(spp=4, bounces=4, seed=21)
        pt.bind_output(other_fb.data_ptr(), other_acc.data_ptr())
        pt.render(spp=4, bounces=4, seed=22)
        pt.set_sample_counts(4)
        pt.write_sample_budget(b)
        sc1.bound.bind()
        pt.render_adaptive(bounces=4, seed=21, keep_counts=True)
        pt.bind_output(other_fb.data_ptr(), other_acc.data_ptr())
        pt.render_adaptive(bounces=4, seed=22)
        pt.wait()
        check(sc1.bound.read(), want[21], "half A")
        check((other_fb.cpu().numpy().view(np.uint32), other_acc.cpu().numpy()), want[22], "half B")
        assert not same(want[21][1], want[22][1])
        assert np.array_equal(pt.sample_counts(), 4 + b)
    finally:
        sc1.bound.bind()


# ---- 5. saturation --------------------------------------------------------------------------------------------------------------
def test_the_last_frames_are_2147483645_and_2147483646(sc1):
    pt = sc1.pt
    sc1.bound.sentinel()
    pt.render(spp=3, bounces=4, seed=8)
    fb0, acc0 = sc1.bound.read()
    n = np.full((H, W), LIMIT - 2, np.uint32)
    n[5] = LIMIT
    n[6] = 0xFFFFFFFF
    start(sc1, n, 5, sentinel=False)
    pt.render_adaptive(bounces=4, seed=8)
    got = sc1.bound.read()
    after = pt.sample_counts()
    sc1.bound.write(fb0, acc0)
    pt.render(spp=2, bounces=4, seed=8, first_sample=LIMIT - 1, reset=False)
    wfb, wacc = sc1.bound.read()
    for y in (5, 6):  # full already: untouched
        wacc[y], wfb[H - 1 - y] = acc0[y], fb0[H - 1 - y]
    check(got, (wfb, wacc), "frames 2147483645 and 2147483646")
    assert not same(got[1], acc0)
    n[n == LIMIT - 2] = LIMIT
    assert np.array_equal(after, n)


# ---- 6. a band ------------------------------------------------------------------------------------------------------------------
def test_a_band_writes_only_its_scene_rows(sc1):
    rows = (3, 14)  # memory rows: scene rows [H - 14, H - 3), eleven of them
    inside = np.zeros((H, W), bool)
    inside[H - rows[1]:H - rows[0]] = True
    n0 = np.full((H, W), 0, np.uint32)
    start(sc1, n0, 3)
    sc1.pt.render_adaptive(bounces=8, seed=5, rows=rows)
    check(sc1.bound.read(), ref_of(sc1, 8, 5).at(np.where(inside, 3, 0), *sentinels()), "the band")
    assert np.array_equal(sc1.pt.sample_counts(), np.where(inside, 3, 0))


# ---- 7. other frame sizes -------------------------------------------------------------------------------------------------------
def test_partial_tile_columns_and_rows(srt, oracle):
    s = Scene(srt, oracle, scene1(oracle), 21, 13)
    try:
        s.bound, s.ocam = Bound(s.pt, 21, 13), moved_camera(oracle)
        s.pt.set_camera(srt_camera(srt, s.ocam))
        b = ((np.arange(21)[None, :] * 5 + np.arange(13)[:, None]) % 7).astype(np.uint32)
        b[12, 20], b[0, 0] = 66, 65
        start(s, 0, b)
        s.pt.render_adaptive(bounces=8, seed=4)
        check(s.bound.read(), Ref(s, s.ocam, 8, 4).at(b, *sentinels(21, 13)), "21 x 13")
        assert np.array_equal(s.pt.sample_counts(), b)
    finally:
        s.close()


def test_64_tiles_are_dealt_by_the_ticket_and_repeat_bit_for_bit(srt, oracle):
    s = Scene(srt, oracle, scene1(oracle), 64, 64)
    try:
        s.bound, s.ocam = Bound(s.pt, 64, 64), moved_camera(oracle)
        s.pt.set_camera(srt_camera(srt, s.ocam))
        ty, tx = np.mgrid[0:64, 0:64] // 8
        b = np.where((tx + ty) % 2 == 0, 0, 3).astype(np.uint32)
        b[24:32, 32:40] = 40  # (tile (4, 3): odd)
        runs = []
        for _ in range(2):
            start(s, 0, b)
            s.pt.render_adaptive(bounces=8, seed=6, count_work=True)
            runs.append(s.bound.read())
            assert np.array_equal(s.pt.sample_counts(), b)
        check(runs[0], Ref(s, s.ocam, 8, 6).at(b, *sentinels(64, 64)), "64 x 64")
        check(runs[1], runs[0], "the call repeated")
        work = s.pt.adaptive_work()
        assert work["pixels"] == 32 * 64 and work["samples"] == int(b.sum())
    finally:
        s.close()


# ---- 8. packing -----------------------------------------------------------------------------------------------------------------
def test_one_pixel_of_200_samples_is_packed_and_an_all_zero_map_costs_nothing(srt, oracle):
    """The closed room: every path runs all B bounces.  A lane-per-pixel kernel would need 1 + 200 * 8 invocations."""
    s = Scene(srt, oracle, closed_room(oracle))
    try:
        s.bound = Bound(s.pt, W, H)
        ocam = oracle.default_camera()
        s.pt.set_camera(srt_camera(srt, ocam))
        x, y = 12, 10
        want, rays = s.oracle_acc(ocam, 200, 8, rows=(H - 1 - y, H - y), cols=(x, x + 1))
        assert rays == 200 * 9
        b = np.zeros((H, W), np.uint32)
        b[y, x] = 200
        start(s, 0, b)
        s.pt.render_adaptive(bounces=8, seed=0, count_work=True)
        (fb, acc), work = s.bound.read(), s.pt.adaptive_work()
        print(work)
        assert same(acc[y, x], want.reshape(H, W, 4)[y, x])
        acc[y, x], fb[H - 1 - y, x] = sentinels()[1][y, x], SENT_FB
        check((fb, acc), sentinels(), "the other pixels")
        assert work["samples"] == 200 and work["pixels"] == 1 and work["closest_calls"] == 200 * 9
        assert work["wave_calls"] <= 1 + -(-200 // 64) * 8
        start(s, 7, 0)
        s.pt.render_adaptive(bounces=8, seed=0, count_work=True)
        check(s.bound.read(), sentinels(), "an all-zero map")
        work = s.pt.adaptive_work()
        assert work["wave_calls"] == 0 and work["samples"] == 0 and work["pixels"] == 0 and work["closest_calls"] == 0
        assert (s.pt.sample_counts() == 7).all()
    finally:
        s.close()


# ---- 9. bound counts and budget -------------------------------------------------------------------------------------------------
def test_bound_tensors_for_counts_and_budget_keep_their_sentinels(sc1):
    import torch

    pt, b = sc1.pt, mixed_map()
    dev = sc1.bound.acc.device
    tn = torch.full((N + 64,), -7, dtype=torch.int32, device=dev)
    tb = torch.full((N + 64,), -7, dtype=torch.int32, device=dev)
    tn[:N] = 2
    tb[:N] = torch.from_numpy(b.astype(np.int32).reshape(-1)).to(dev)
    torch.cuda.synchronize()
    sc1.bound.sentinel()
    pt.render(spp=2, bounces=8, seed=5)
    pt.bind_sample_counts(tn[:N].view(H, W))
    pt.bind_sample_budget(tb[:N].view(H, W))
    try:
        pt.render_adaptive(bounces=8, seed=5)
        check(sc1.bound.read(), ref_of(sc1, 8, 5).at(2 + b, *sentinels()), "bound counts and budget")
        assert np.array_equal(pt.sample_counts(), 2 + b) and np.array_equal(pt.sample_budget_map(), b)
        hn, hb = tn.cpu().numpy(), tb.cpu().numpy()
        assert np.array_equal(hn[:N].reshape(H, W), (2 + b).astype(np.int32)) and (hn[N:] == -7).all()
        assert np.array_equal(hb[:N].reshape(H, W), b.astype(np.int32)) and (hb[N:] == -7).all()
        with pytest.raises(ValueError):
            pt.bind_sample_counts(tn[:N - 1])
        with pytest.raises(TypeError):
            pt.bind_sample_budget(torch.zeros((H, W), dtype=torch.float32, device=dev))
    finally:
        pt.bind_sample_counts(None)
        pt.bind_sample_budget(None)


# ---- 10. side effects -----------------------------------------------------------------------------------------------------------
def test_an_adaptive_render_leaves_the_other_outputs_alone(sc1, srt, oracle):
    from test_gpu_radiance import camera_rays

    pt = sc1.pt
    o, d = camera_rays(oracle, sc1.ocam)
    sc1.bound.unbind()
    try:
        pt.render(spp=3, bounces=4, seed=9)
        first = pt.accumulator(), pt.framebuffer()
        pt.render_gbuffer()
        pt.write_rays(o, d)
        pt.trace_rays()
        pt.trace_radiance(samples=2, bounces=2, seed=1)

        def snapshot():
            st = srt.capi.Stats()
            assert pt.L.srt_get_stats(pt._h, C.byref(st)) == 0
            return dict(stats=bytes(st), rad=pt.radiance(), **{"g_" + k: pt.gbuffer(k) for k in srt.capi.GBUFFERS},
                        **{"r_" + k: pt.ray_output(k) for k in srt.capi.RAY_OUTPUTS})

        before = snapshot()
        pt.set_sample_counts(3)
        pt.write_sample_budget(mixed_map())
        pt.render_adaptive(bounces=4, seed=9, count_work=True)
        pt.wait()
        after = snapshot()
        for k in before:
            a, b = before[k], after[k]
            assert (a == b) if isinstance(a, bytes) else np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
        assert not same(pt.accumulator(), first[0])
        pt.render(spp=3, bounces=4, seed=9)  # the next srt_render
        assert same(pt.accumulator(), first[0]) and np.array_equal(pt.framebuffer(), first[1])
    finally:
        sc1.bound.bind()


# ---- 11. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_untouched(srt, oracle):
    c = srt.capi
    pt = srt.PathTracer(W, H)
    try:
        L = pt.L

        def rc(**kw):
            p = c.AdaptiveParams()
            L.srt_adaptive_params_default(C.byref(p))
            p.row_begin, p.row_end = 0, H
            for k, v in kw.items():
                setattr(p, k, v)
            return L.srt_render_adaptive(pt._h, C.byref(p))

        def brc(**kw):
            p = c.BudgetParams()
            L.srt_budget_params_default(C.byref(p))
            for k, v in kw.items():
                setattr(p, k, v)
            return L.srt_sample_budget(pt._h, C.byref(p))

        u = np.zeros((H, W), np.uint32)
        up = u.ctypes.data_as(C.POINTER(C.c_uint32))
        w, t = c.AdaptiveWork(), C.c_uint64(0)
        assert rc() == c.ERR_STATE  # before srt_set_scene
        assert L.srt_read_sample_counts(pt._h, up) == c.ERR_STATE and L.srt_read_sample_budget(pt._h, up) == c.ERR_STATE
        assert L.srt_get_adaptive_work(pt._h, C.byref(w)) == c.ERR_STATE and L.srt_get_budget_total(pt._h, C.byref(t)) == c.ERR_STATE
        oarr, n = oracle.make_objects(scene1(oracle)[0])
        pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
        assert rc() == c.ERR_STATE  # before srt_set_camera
        pt.set_camera(srt.default_camera())
        assert rc() == c.ERR_STATE  # neither counts nor budget
        assert rc(flags=4) == c.ERR_INVALID_ARG  # (the arguments before the buffers)
        pt.set_sample_counts(2)
        assert rc() == c.ERR_STATE  # no budget
        pt.write_sample_budget(np.full((H, W), 3, np.uint32))
        pt.render(spp=2, bounces=2, seed=1)
        acc, fb = pt.accumulator(), pt.framebuffer()
        for kw in (dict(row_begin=0, row_end=0), dict(row_begin=5, row_end=5), dict(row_begin=-1), dict(row_end=H + 1), dict(flags=4), dict(reserved=1),
                   dict(max_samples=0), dict(max_samples=4097), dict(max_bounces=-1)):
            assert rc(**kw) == c.ERR_INVALID_ARG, kw
        assert same(pt.accumulator(), acc) and np.array_equal(pt.framebuffer(), fb) and (pt.sample_counts() == 2).all()
        assert L.srt_get_adaptive_work(pt._h, C.byref(w)) == c.ERR_STATE
        # the budget pass: the arguments, then guide, variance, counts
        for kw in (dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan")), dict(floor=-0.5), dict(floor=float("nan")), dict(max_budget=0),
                   dict(max_budget=4097), dict(flags=2)):
            assert brc(**kw) == c.ERR_INVALID_ARG, kw
        assert brc() == c.ERR_STATE  # no guide
        pt.render_gbuffer()
        assert brc() == c.ERR_STATE  # no variance
        pt.half_ptr()
        pt.variance(albedo=False, merge=False, gbuffer=False)
        assert brc() == c.ERR_STATE and brc(flags=0) == c.OK  # the own variance was estimated without ALBEDO
        assert brc(flags=0, threshold=float("inf")) == c.OK and L.srt_get_budget_total(pt._h, C.byref(t)) == c.OK and t.value == 0
        assert (pt.sample_budget_map() == 0).all()
        assert same(pt.accumulator(), acc) and (pt.sample_counts() == 2).all()
        # a render that works, and its record
        pt.write_sample_budget(np.full((H, W), 3, np.uint32))
        assert rc(max_bounces=2, seed=1) == c.OK and L.srt_get_adaptive_work(pt._h, C.byref(w)) == c.ERR_STATE  # it did not count
        assert (pt.sample_counts() == 5).all()
        assert rc(max_bounces=2, seed=1, flags=c.ADAPTIVE_COUNT_WORK | c.ADAPTIVE_KEEP_COUNTS) == c.OK
        assert L.srt_get_adaptive_work(pt._h, C.byref(w)) == c.OK and (w.valid, w.pixels, w.samples) == (1, N, 3 * N)
        assert (pt.sample_counts() == 5).all()
    finally:
        pt.close()
    # a budget pass without counts
    pt = srt.PathTracer(W, H)
    try:
        pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
        pt.set_camera(srt.default_camera())
        pt.render(spp=2, bounces=2)
        pt.half_ptr()
        pt.variance(merge=False)
        with pytest.raises(srt.SrtError) as e:
            pt.sample_budget()
        assert e.value.code == c.ERR_STATE
        pt.set_sample_counts(2)
        pt.sample_budget()
        assert pt.budget_total() == int(pt.sample_budget_map().sum())
    finally:
        pt.close()


# ---- 12. the C++ host, host.py and the command line -----------------------------------------------------------------------------
def test_the_host_layers_and_the_cli_run_the_two_half_workflow(srt, tmp_path):
    w, h, spp = 32, 24, 4
    r = srt.host.Renderer(w, h)
    try:
        r.set_scene(srt.host.Scene(scene_path("Scene1")))
        r.settings(fov=55, max_bounces=2, seed=0)
        total, counts = r.render_adaptive_frame(spp, rounds=1, threshold=0.05, max_budget=8)
        r.render_gbuffer("object")
        miss = r.gbuffer("object") < 0
        acc = r.accumulator()
        # the pieces: the counts as they stand, and another round by hand
        assert np.array_equal(2 * r.sample_counts(), counts)
        more = r.sample_budget(threshold=0.05, max_budget=8)
        r.render_adaptive(bounces=2, seed=0)
        assert int(2 * r.sample_counts().astype(np.int64).sum()) == total + 2 * more
    finally:
        r.close()
    assert total == int(counts.astype(np.int64).sum()) and (counts >= spp).all() and (counts <= spp + 2 * 8).all() and (counts % 2 == 0).all()
    assert miss.any() and (counts[miss] == spp).all() and total > spp * w * h
    assert np.isfinite(acc[..., :3]).all()
    out, cfile = tmp_path / "frame.ppm", tmp_path / "counts.bin"
    p = subprocess.run([CLI, "--scene", scene_path("Scene1"), "--width", str(w), "--height", str(h), "--spp", str(spp), "--bounces", "2", "--adaptive", "1",
                        "--adaptive-max", "8", "--counts-out", str(cfile), "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    printed = int(re.search(r"total samples (\d+)", p.stderr).group(1))
    got = np.frombuffer(cfile.read_bytes(), np.uint32).reshape(h, w)
    assert printed == int(got.astype(np.int64).sum()) == total and np.array_equal(got, counts)
    assert out.read_bytes().startswith(b"P6\n%d %d\n255\n" % (w, h))
