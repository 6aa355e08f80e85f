"""The seam under srt_trace_radiance, srt_trace_light_probes (unlisted and listed) and srt_render_adaptive on the MI355X: the
wave-level sample pool the three kernels run (srt_sample_pool.hip.h; light_probe_kernel from a text of its own) — the hand-out,
the chunks of RAD_CHUNK = 64 samples, the fold of ROWS_IN_FLIGHT = 8 rows at a time — at the sizes where it changes path.  Every
comparison is bit for bit in all four lanes (NaN alphas compare as their bits).  Radiance and adaptive are compared with the CPU
oracle's accumulator (POW_SHARED), as tests/test_gpu_radiance.py and tests/test_gpu_adaptive.py do; the probes' RADIANCE with
srt_trace_radiance for the explicit rays and their COEFFICIENTS with tests/light_probe_reference.py applied to
srt_trace_radiance's output.  Frames are 9 x 9 (81 rays: a full block and one of 17 lanes; four tiles, three of them partial),
so a case costs the oracle well under a second."""
import ctypes as C

import numpy as np
import pytest

import light_probe_reference as R
from test_gpu_adaptive import SENT_ACC, SENT_FB, Bound, Ref, check, sentinels, start
from test_gpu_adaptive import bits as ubits
from test_gpu_light_probes import PROBES, explicit_rays
from test_gpu_radiance import Scene, camera_rays, differing, moved_camera, same, srt_camera
from test_gpu_visibility import closed_room, scene1

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
W = H = 9
N = W * H
# both sides of ROWS_IN_FLIGHT (8) and of RAD_CHUNK (64), and the first full fold of a second chunk (128) and the row behind it
SAMPLE_COUNTS = [1, 7, 8, 9, 63, 64, 65, 128, 129]
ROOMS = {"scene1": scene1, "closed_room": closed_room}


@pytest.fixture(scope="module", params=list(ROOMS))
def sc(request, srt, oracle):
    s = Scene(srt, oracle, ROOMS[request.param](oracle), W, H)
    s.name = request.param
    s.ocam = moved_camera(oracle) if request.param == "scene1" else oracle.default_camera()
    s.rays = camera_rays(oracle, s.ocam, W, H)
    s.wants = {}
    yield s
    s.close()


@pytest.fixture(scope="module")
def sc1(srt, oracle):
    s = Scene(srt, oracle, scene1(oracle), W, H)
    s.ocam = moved_camera(oracle)
    s.rays = camera_rays(oracle, s.ocam, W, H)
    s.wants = {}
    yield s
    s.close()


def want_of(s, n, bounces, seed):
    """The oracle's accumulator of the 9 x 9 frame, computed once per (n, bounces, seed)."""
    key = (n, bounces, seed)
    if key not in s.wants:
        s.wants[key] = s.oracle_acc(s.ocam, n, bounces, seed)
    return s.wants[key]


def prefix_rays(s, count, n, bounces, seed):
    """The oracle's ray count of the first `count` pixels (i = x + y * W): whole scene rows, and a run of the next one.  Scene
    row y is memory row H - 1 - y."""
    full, rest = divmod(count, W)
    rays = 0
    if full:
        rays += s.oracle_acc(s.ocam, n, bounces, seed, rows=(H - full, H))[1]
    if rest:
        rays += s.oracle_acc(s.ocam, n, bounces, seed, rows=(H - 1 - full, H - full), cols=(0, rest))[1]
    return rays


def check_radiance_work(work, count, n, rays):
    blocks = (count + 63) // 64
    assert work["valid"] == 1 and work["rays"] == count and work["samples"] == count * n
    assert work["closest_calls"] == rays
    assert 64 * work["wave_calls"] >= work["closest_calls"] - work["samples"]
    assert work["wave_calls"] >= blocks  # one primary invocation per block of 64 rays


# ---- radiance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SAMPLE_COUNTS)
def test_radiance_sample_counts_around_the_fold_and_the_chunk(sc1, n):
    o, d = sc1.rays
    want, rays = want_of(sc1, n, 8, 3)
    sc1.pt.trace_radiance(o, d, samples=n, bounces=8, seed=3, count_work=True)
    got, work = sc1.pt.radiance(), sc1.pt.radiance_work()
    assert same(got, want), "%d of %d rays differ from the oracle" % (differing(got, want), N)
    check_radiance_work(work, N, n, rays)
    sc1.pt.trace_radiance(samples=n, bounces=8, seed=3)  # without the work record: the same bits
    assert same(sc1.pt.radiance(), want)


@pytest.fixture(scope="module")
def rooms(srt, oracle):
    made = {}

    def get(name):
        if name not in made:
            s = Scene(srt, oracle, ROOMS[name](oracle), W, H)
            s.name = name
            s.ocam = moved_camera(oracle) if name == "scene1" else oracle.default_camera()
            s.rays = camera_rays(oracle, s.ocam, W, H)
            s.wants = {}
            made[name] = s
        return made[name]

    yield get
    for s in made.values():
        s.close()


@pytest.mark.parametrize("room,bounces", [("closed_room", 8), ("scene1", 1), ("scene1", 8)])
@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_radiance_ray_counts_around_the_block(rooms, count, room, bounces):
    sc = rooms(room)
    n, seed = 65, 7
    o, d = sc.rays
    want, _ = want_of(sc, n, bounces, seed)
    rays = prefix_rays(sc, count, n, bounces, seed)
    if sc.name == "closed_room":
        assert rays > count * n * bounces  # all but a few paths run their full length (a few leave through the room's seams)
    sc.pt.trace_radiance(o[:count], d[:count], samples=n, bounces=bounces, seed=seed, count_work=True)
    got, work = sc.pt.radiance(), sc.pt.radiance_work()
    assert got.shape == (count, 4) and same(got, want[:count]), "%d of %d rays differ from the oracle" % (differing(got, want[:count]), count)
    check_radiance_work(work, count, n, rays)
    sc.pt.trace_radiance(samples=n, bounces=bounces, seed=seed)
    assert same(sc.pt.radiance(), want[:count])


def test_a_block_of_misses_between_two_pooled_blocks(srt, oracle):
    """24 x 8 = 192 rays, i = x + y * 24: blocks 0 and 2 are the moved camera's, block 1 looks at the sky from above the scene."""
    w, h, n, bounces, seed = 24, 8, 9, 8, 5
    s = Scene(srt, oracle, scene1(oracle), w, h)
    try:
        ocam, sky = moved_camera(oracle), oracle.default_camera()
        sky.position[:], sky.forward[:], sky.up[:] = (0.0, 50.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0)
        (o, d), (so, sd) = camera_rays(oracle, ocam, w, h), camera_rays(oracle, sky, w, h)
        o[64:128], d[64:128] = so[64:128], sd[64:128]
        nn, pp, t = (C.c_float * 3)(), (C.c_float * 3)(), C.c_float(0)
        hit = np.array([oracle.lib().srt_oracle_closest(s.oarr, s.n, (C.c_float * 3)(*o[i, :3]), (C.c_float * 3)(*d[i, :3]), nn, pp, C.byref(t)) >= 0
                        for i in range(w * h)])
        assert not hit[64:128].any() and hit[:64].any() and hit[128:].any()  # the precondition, from the oracle
        (wa, _), (ws, _) = s.oracle_acc(ocam, n, bounces, seed), s.oracle_acc(sky, n, bounces, seed)
        want = wa.copy()
        want[64:128] = ws[64:128]
        for count_work in (True, False):
            s.pt.trace_radiance(o, d, samples=n, bounces=bounces, seed=seed, count_work=count_work)
            got = s.pt.radiance()
            assert same(got, want), "%d of 192 rays differ from the oracle" % differing(got, want)
        assert not same(wa[64:128], ws[64:128])
    finally:
        s.close()


def test_radiance_continues_at_sample_65(sc1):
    o, d = sc1.rays
    want, _ = want_of(sc1, 129, 8, 3)
    sc1.pt.trace_radiance(o, d, samples=64, bounces=8, seed=3)
    assert same(sc1.pt.radiance(), want_of(sc1, 64, 8, 3)[0])
    sc1.pt.trace_radiance(samples=65, bounces=8, seed=3, first_sample=65, reset=False)
    got = sc1.pt.radiance()
    assert same(got, want), "%d of %d rays differ from one call of 129 samples" % (differing(got, want), N)


# ---- light probes, unlisted and listed -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("listed", [False, True])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 129])
def test_light_probes_direction_and_sample_counts(sc1, srt, k, listed):
    pt = sc1.pt
    d = srt.light_probe_sphere(k)
    P = PROBES.shape[0]
    # listed: probes 2 and 0, and between them a word out of range
    words = np.array([3, P, 0, 0, 2, P + 4, 0], U)
    idx = np.array([0, 2]) if listed else np.arange(P)
    skipped = np.setdiff1d(np.arange(P), idx)
    o, dd = explicit_rays(PROBES, d)
    try:
        if listed:
            pt.bind_probe_list(words)
        for n in (1, 9, 64, 65):
            kw = dict(samples=n, bounces=8, seed=11, id_base=1000)
            closest = 0  # of the probes the call traces, probe by probe
            for p in idx:
                pt.trace_radiance(o[p * k:(p + 1) * k], dd[p * k:(p + 1) * k], count_work=True, **dict(kw, id_base=1000 + p * k))
                closest += pt.radiance_work()["closest_calls"]
            pt.trace_radiance(o, dd, **kw)
            want = pt.radiance().reshape(P, k, 4)
            want_c = R.project(want, d)
            other = dict(kw, seed=12)
            pt.trace_light_probes(PROBES, d, radiance=True, **other)  # what an unlisted probe keeps
            keep_r, keep_c = pt.light_probe_radiance(), pt.light_probe_coefficients()
            pt.trace_light_probes(radiance=True, count_work=True, listed=listed, **kw)
            got, coeff, work = pt.light_probe_radiance(), pt.light_probe_coefficients(), pt.light_probe_work()
            assert same(got[idx], want[idx]), "K=%d n=%d: %d rays differ from srt_trace_radiance" % (k, n, differing(got[idx], want[idx]))
            assert same(coeff[idx], want_c[idx]), "K=%d n=%d: %d coefficients differ from the reference" % (k, n, differing(coeff[idx], want_c[idx]))
            assert same(got[skipped], keep_r[skipped]) and same(coeff[skipped], keep_c[skipped])
            j = (k + 63) // 64
            assert work["valid"] == 1 and work["probes"] == len(idx) and work["rays"] == len(idx) * k and work["samples"] == len(idx) * k * n
            assert work["closest_calls"] == closest
            assert work["wave_calls"] >= len(idx) * j and 64 * work["wave_calls"] >= work["closest_calls"] - work["samples"]
            # without the work record and without the RADIANCE output: the same coefficients
            if listed:
                pt.trace_light_probes(**other)
            pt.trace_light_probes(listed=listed, **kw)
            coeff2 = pt.light_probe_coefficients()
            assert same(coeff2[idx], want_c[idx]) and same(coeff2[skipped], keep_c[skipped])
    finally:
        pt.wait()
        pt.bind_probe_list(None)


# ---- adaptive ------------------------------------------------------------------------------------------------------------------
def pool_map():
    """Tile (0, 0) cycles through budgets on both sides of the fold's 8 rows and of the chunk, so that its slots run out in
    different chunks; column 8 and row 8 (the partial tiles) hold 0 .. 3."""
    b = ((np.arange(W)[None, :] + 2 * np.arange(H)[:, None]) % 4).astype(U)
    b[0:8, 0:8] = np.resize(np.array([0, 1, 7, 8, 9, 63, 64, 65, 129], U), 64).reshape(8, 8)
    return b


def test_adaptive_budgets_that_run_out_in_different_chunks(sc, srt, oracle):
    pt, bounces, seed = sc.pt, 8, 5
    pt.set_camera(srt_camera(srt, sc.ocam))
    sc.bound = Bound(pt, W, H)
    try:
        b = pool_map()
        n0 = np.where((np.arange(W)[None, :] + np.arange(H)[:, None]) % 3 == 0, 5, 0).astype(U)  # some pixels hold 5 samples
        assert ((n0 == 0) & (b > 0)).any() and ((n0 == 5) & (b > 0)).any() and ((n0 == 5) & (b == 0)).any() and (b[0:8, 0:8] == 129).any()
        ref = Ref(sc, sc.ocam, bounces, seed)
        pt.render(spp=5, bounces=bounces, seed=seed)
        fb5, acc5 = sc.bound.read()
        check((fb5, acc5), ref.at(np.full((H, W), 5), *sentinels(W, H)), "srt_render(1..5)")
        # the state in front of the call: the 5-sample mean where it continues, the sentinel everywhere else
        fb0, acc0 = sentinels(W, H)
        go = (n0 == 5) & (b > 0)
        acc0[go], fb0[go[::-1]] = acc5[go], fb5[go[::-1]]
        want = ref.at(np.where(b > 0, n0 + b, 0), *sentinels(W, H))
        # the oracle's rays, pixel by pixel: frames n0 + 1 .. n0 + b of that pixel alone
        rays = 0
        for y, x in zip(*np.nonzero(b)):
            rays += sc.oracle_acc(sc.ocam, int(b[y, x]), bounces, seed, first_sample=int(n0[y, x]) + 1, rows=(H - 1 - y, H - y), cols=(x, x + 1))[1]
        for count_work in (True, False):
            sc.bound.write(fb0, acc0)
            start(sc, n0, b, sentinel=False)
            pt.render_adaptive(bounces=bounces, seed=seed, count_work=count_work)
            got = sc.bound.read()
            check(got, want, "count_work %d against the oracle" % count_work)
            zero = b == 0
            assert (ubits(got[1])[zero] == SENT_ACC).all() and (got[0][zero[::-1]] == SENT_FB).all()
            assert np.array_equal(pt.sample_counts(), n0 + b)
            if count_work:
                work = pt.adaptive_work()
                assert work["valid"] == 1 and work["pixels"] == int((b > 0).sum()) and work["samples"] == int(b.sum())
                assert work["closest_calls"] == rays
                assert work["wave_calls"] >= 4 and 64 * work["wave_calls"] >= work["closest_calls"] - work["samples"]  # one primary invocation per tile
    finally:
        sc.bound.unbind()
