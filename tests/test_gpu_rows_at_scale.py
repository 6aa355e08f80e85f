"""The rows path-trace kernels (k_lds_rows6, k_lds_rows, t_lds_rows in srt_capi.hip: sample colours go through rows of the sample
buffer, srt::fold_from_rows) at the frame sizes that ship them, against the oracle bit for bit: framebuffer and all four accumulator
lanes, NaNs compared as NaNs.

tests/test_gpu_sample_rows.py and tests/test_gpu_six_waves.py compare these kernels with the oracle on a 40 x 24 frame at 2..15
samples: six workgroups.  From 16 samples on the shape rule keeps full tiles, and with them the rows path, only on launches of at
least 15 blocks of 16 x 16 pixels per CU (3840 on 256 CUs), so the folds of 16..63 rows per slot, five or six workgroups resident
on a CU, rows that have left L1 before the fold reads them back, cost-ordered dispatch (256 blocks and more) and row offsets
beyond 2^31 bytes all need frames of the size of the real ones.  The oracle renders only windows of those frames (rows x cols of the
real frame, 64 columns by 16..48 rows each, whole tiles): the first block, the last block row and column, the other two corners, the
big ball's silhouette and the horizon (tiles with fewer than 64 traced slots), and two windows inside the ball (all 64 traced).  What
each window holds is asserted from the oracle's primary hits.  One comparison in case (a) extends the check from the windows to every
pixel: the same frame rendered as eight bands, which take the small-tile kernel (no rows, another hand-out).

Which kernel a launch reaches is not reported by the library (no ABI change).  Every case asks the rule itself
(tests/native/rows_rule_check.cpp --ask, with the device's CU count and the scene's LDS bytes from six_wave_rule_check.cpp) and
asserts the answer, and asserts tile_rows == 8 and sample_chunks == 1 from the launch's stats; frame sizes that sit on a threshold
are computed from the CU count.  Nothing skips where the rule disagrees.

Oracle cost (16 threads, measured on the CPU): 2.4 M path-samples/s in a window on Scene1's ball at 8 bounces, 0.8 M/s in
Scene_indirect; the windows of one launch are 11 k pixels, 0.35 M path-samples at 32 spp: about 0.3 s per compared launch.
"""
import ctypes as C
import math

import numpy as np
import pytest

import rows_rule
from conftest import scene_path
from test_gpu_paths import _caller_accumulator
from test_gpu_sample_rows import nansmooth_sphere
from test_gpu_six_waves import _objects, threshold_counts

THREADS = 16
_ORACLE = {}


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    return rows_rule.rows_rule_exe(tmp_path_factory)


@pytest.fixture(scope="module")
def six_exe(tmp_path_factory):
    return rows_rule.six_wave_rule_exe(tmp_path_factory)


@pytest.fixture(scope="module")
def cu_count():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _load(oracle, name):
    return oracle.make_objects(oracle.load_scene_json_py(scene_path(name)))


def _lds_bytes(six_exe, name):
    return rows_rule.grow(six_exe, scene_path(name), [])[0][1]


def _tracer(srt, sc, w, h):
    pt = srt.PathTracer(w, h)
    pt.set_scene(C.cast(sc[0], C.POINTER(srt.Object)), sc[1])
    pt.set_camera(srt.default_camera())
    return pt


def _windows(w, h, band=None):
    """[(what it holds, cols, rows)] for Scene1's default view on a w x h frame: memory rows (row 0 is the image's top), aligned to
    the band's blocks of 16 rows.  "none": sky, no slot traced; "all": every slot traced; "mixed": tiles with 1..63 traced slots."""
    rb, re = band if band is not None else (0, h)
    f = (h / 2) / math.tan(math.radians(55 / 2))  # pixels per unit of tan: the default camera's vertical field of view is 55 degrees
    cx, cy, R = w / 2, h / 2, f * math.tan(math.asin(1 / 5))  # the big ball: radius 1 at (0, 0, 5)
    row16 = lambda y: rb + (int(y) - rb) // 16 * 16
    col16 = lambda x: int(x) // 16 * 16
    top, bottom = (rb, rb + 16), (row16(re - 1) - 16, re)  # (the last block row may be partial: the block row above it comes along)
    left, right = (0, 64), (w - 64, w)
    hcol = col16(w / 8)
    # the floor is a sphere of radius 1000 whose top is 1.2 below the camera: its horizon lies acos(1000 / 1001.2) below the horizontal
    hrow = row16(cy + math.sin(math.acos(1000 / 1001.2)) * f * math.hypot(1.0, (hcol + 32 - cx) / f))
    ball_cols = (col16(cx) - 32, col16(cx) + 32)
    return [("none", left, top), ("none", right, top), ("all", left, bottom), ("all", right, bottom),
            ("mixed", (col16(cx - R) - 32, col16(cx - R) + 32), (row16(cy) - 16, row16(cy) + 16)),
            ("mixed", (hcol, hcol + 64), (hrow - 16, hrow + 32)),
            ("all", ball_cols, (row16(cy - R / 2), row16(cy - R / 2) + 16)), ("all", ball_cols, (row16(cy + R / 2), row16(cy + R / 2) + 16))]


def _check_what_windows_hold(oracle, sc, w, h, wins):
    """the oracle's primary hits (one sample without a bounce: black where the ray hit something that does not shine) per 8 x 8 tile"""
    for what, cols, rows in wins:
        assert 0 <= cols[0] < cols[1] <= w and 0 <= rows[0] < rows[1] <= h and 48 <= cols[1] - cols[0] <= 64 and rows[1] - rows[0] >= 16, (cols, rows)
        _, acc, _ = oracle.render(sc[0], sc[1], oracle.default_environment(), oracle.default_camera(), w, h, spp=1, bounces=0, rows=rows, cols=cols,
                                  threads=THREADS)
        hit = (acc[h - rows[1]:h - rows[0], cols[0]:cols[1], :3] == 0).all(-1)[::-1]
        nr, nc = hit.shape[0] // 8, hit.shape[1] // 8
        per_tile = hit[:nr * 8, :nc * 8].reshape(nr, 8, nc, 8).sum((1, 3))
        if what == "none":
            assert not hit.any(), (cols, rows)
        elif what == "all":
            assert hit.all(), (cols, rows)
        else:
            assert ((per_tile > 0) & (per_tile < 64)).any(), (cols, rows, per_tile.tolist())


def _compare(pt, oracle, key, sc, w, h, wins, band=None, acc_in=None, **call):
    """the launch just rendered with **call == the oracle on every window; the oracle's windows of a request that starts a frame
    are computed once.  Returns the oracle's accumulator windows."""
    band = band if band is not None else (0, h)
    fb, acc = pt.framebuffer(rows=band), pt.accumulator()
    out = []
    for _, cols, rows in wins:
        assert band[0] <= rows[0] < rows[1] <= band[1]
        k = (key, w, h, cols, rows, tuple(sorted(call.items())))
        if acc_in is not None or k not in _ORACLE:
            ofb, oacc, _ = oracle.render(sc[0], sc[1], oracle.default_environment(), oracle.default_camera(), w, h, rows=rows, cols=cols,
                                         threads=THREADS, accumulator=acc_in, **call)
            ys = slice(h - rows[1], h - rows[0])
            ref = (ofb[rows[0]:rows[1], cols[0]:cols[1]].copy(), oacc[ys, cols[0]:cols[1]].copy())
            if acc_in is None:
                _ORACLE[k] = ref
        else:
            ref = _ORACLE[k]
        ofb, oacc = ref
        g = acc[h - rows[1]:h - rows[0], cols[0]:cols[1]]
        nan = np.isnan(oacc)
        assert np.array_equal(np.isnan(g), nan), (cols, rows)
        bad = ~nan & (g.view(np.uint32) != oacc.view(np.uint32))
        assert not bad.any(), (cols, rows, int(bad.sum()), np.argwhere(bad)[:8].tolist())
        assert np.array_equal(fb[rows[0] - band[0]:rows[1] - band[0], cols[0]:cols[1]], ofb), (cols, rows)
        out.append(oacc)
    return out


def _reached(pt, rule, label, want_rows, want_six, **request):
    """prints the launch's shape and the rule's answer; asserts full tiles in one chunk and the answer the case expects"""
    st, a = pt.stats(), rows_rule.ask(rule, [request])[0]
    print("%s: tile_rows %d sample_chunks %d shape_source %d; rule: tile_h %d chunks %d blocks %d rows %d six %d rows_bytes %d" %
          (label, st.tile_rows, st.sample_chunks, st.shape_source, a.tile_h, a.chunks, a.wg8, a.rows, a.six, a.rows_bytes))
    assert (st.tile_rows, st.sample_chunks) == (8, 1), label
    assert (a.tile_h, a.chunks) == (8, 1), label
    assert a.rows == want_rows and (want_six is None or a.six == want_six), (label, a)
    return a


def _same_bits(a, b):
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and not (~nan & (a.view(np.uint32) != b.view(np.uint32))).any()


@pytest.mark.gpu
def test_config_2_in_estimated_and_recorded_order_and_counting(srt, oracle, rule, six_exe, cu_count):
    """(a) Scene1, 1920 x 1080, 32 spp, 8 bounces, seed 0: 8160 workgroups, 1.0 GiB of rows, a fold of four groups of eight rows.
    The first launch runs in estimated cost order and records, the second in recorded order, the third counts (t_lds_rows).  Then
    every pixel against the same frame in eight bands, which take small tiles."""
    w, h = 1920, 1080
    call = dict(spp=32, bounces=8, seed=0)
    sc = _load(oracle, "Scene1")
    wins = _windows(w, h)
    _check_what_windows_hold(oracle, sc, w, h, wins)
    req = dict(w=w, rows=h, spp=32, cu_count=cu_count, lds_bytes=_lds_bytes(six_exe, "Scene1"))
    pt = _tracer(srt, sc, w, h)
    for label in ("estimated order", "recorded order"):
        pt.render(**call)
        _reached(pt, rule, "config 2, " + label, 1, 1, **req)
        _compare(pt, oracle, "Scene1", sc, w, h, wins, **call)
    fb, acc = pt.framebuffer(), pt.accumulator()
    pt.render(count_rays=True, count_work=True, **call)
    _reached(pt, rule, "config 2, counting", 1, None, **req)
    c = pt.work_counts().as_dict()
    print("config 2, counting:", c)
    assert c["valid"] == 1 and c["waves"] > 0 and c["closest_hit_calls"] == c["pool_steps"] + c["waves"]
    assert pt.stats().path_samples == w * h * 32
    _compare(pt, oracle, "Scene1", sc, w, h, wins, **call)
    assert np.array_equal(pt.framebuffer(), fb) and _same_bits(pt.accumulator(), acc)
    pt.close()
    bands = _tracer(srt, sc, w, h)
    for rb in range(0, h, 135):
        bands.render(rows=(rb, rb + 135), **call)
        st = bands.stats()
        print("config 2, band (%d, %d): tile_rows %d sample_chunks %d" % (rb, rb + 135, st.tile_rows, st.sample_chunks))
        assert st.tile_rows < 8 and st.sample_chunks == 1, rb
    assert np.array_equal(bands.framebuffer(), fb)
    assert _same_bits(bands.accumulator(), acc)
    bands.close()


def _threshold_frame(cu_count):
    """the smallest frame that keeps full tiles from 16 samples on: 16 a x 16 b pixels with a b = 15 x cu_count blocks, about 5 : 3"""
    n = 15 * cu_count
    b = min((d for d in range(1, n + 1) if n % d == 0), key=lambda d: abs(d - math.sqrt(n * 0.6)))
    return 16 * (n // b), 16 * b


@pytest.mark.gpu
@pytest.mark.parametrize("name,spp", [("Scene_indirect", 16), ("Scene1", 63)])
def test_both_ends_of_the_sample_window_on_the_smallest_frame(srt, oracle, rule, six_exe, cu_count, name, spp):
    """(b) 16 samples (two groups of eight rows; Scene_indirect: every slot traced, long paths) and 63 (seven groups and a
    remainder of seven, the last count before sample chunks) on the frame of exactly 15 blocks per CU: 1280 x 768 on 256 CUs"""
    w, h = _threshold_frame(cu_count)
    assert (w // 16) * (h // 16) == 15 * cu_count
    call = dict(spp=spp, bounces=8, seed=3)
    sc = _load(oracle, name)
    wins = _windows(w, h)
    if name == "Scene1":
        _check_what_windows_hold(oracle, sc, w, h, wins)
    pt = _tracer(srt, sc, w, h)
    pt.render(**call)
    _reached(pt, rule, "%s %d x %d %d spp" % (name, w, h, spp), 1, 1, w=w, rows=h, spp=spp, cu_count=cu_count, lds_bytes=_lds_bytes(six_exe, name))
    _compare(pt, oracle, name, sc, w, h, wins, **call)
    pt.close()


@pytest.mark.gpu
def test_one_block_row_below_the_smallest_frame_takes_small_tiles(srt, oracle, rule, six_exe, cu_count):
    """(b) ... and one block row fewer at 16 samples: the rule answers small tiles, so the frame above sits on the threshold"""
    w, h = _threshold_frame(cu_count)
    h -= 16
    call = dict(spp=16, bounces=8, seed=3)
    sc = _load(oracle, "Scene_indirect")
    a = rows_rule.ask(rule, [dict(w=w, rows=h, spp=16, cu_count=cu_count, lds_bytes=_lds_bytes(six_exe, "Scene_indirect"))])[0]
    pt = _tracer(srt, sc, w, h)
    pt.render(**call)
    st = pt.stats()
    print("Scene_indirect %d x %d 16 spp: tile_rows %d sample_chunks %d; rule: tile_h %d rows %d six %d" % (w, h, st.tile_rows, st.sample_chunks, a.tile_h, a.rows, a.six))
    assert a.tile_h < 8 and a.rows == 0 and st.tile_rows == a.tile_h and st.sample_chunks == 1
    _compare(pt, oracle, "Scene_indirect", sc, w, h, _windows(w, h), **call)
    pt.close()


@pytest.mark.gpu
def test_resumed_on_a_callers_accumulator(srt, oracle, rule, six_exe, cu_count):
    """(c) 1080p: 20 samples (two groups and a remainder of four), then 17 more (two groups and one) on the ragged band (3, 1075)
    onto a caller's accumulator (negatives, -0, 1e-38, a non-zero alpha); and the same band from first_sample = 2^24 - 10, where the
    running mean's weight goes from the float to the double divide at the eleventh sample, inside the second group of rows"""
    w, h, band = 1920, 1080, (3, 1075)
    sc = _load(oracle, "Scene1")
    lds = _lds_bytes(six_exe, "Scene1")
    pt = _tracer(srt, sc, w, h)
    pt.render(spp=20, bounces=8, seed=4)
    _reached(pt, rule, "1080p 20 spp", 1, 1, w=w, rows=h, spp=20, cu_count=cu_count, lds_bytes=lds)
    _compare(pt, oracle, "Scene1", sc, w, h, _windows(w, h), spp=20, bounces=8, seed=4)
    wins = _windows(w, h, band)
    _check_what_windows_hold(oracle, sc, w, h, wins)
    caller = _caller_accumulator(h, w, 1234)
    for first_sample in (21, 2**24 - 10):
        pt.write_accumulator(caller)
        call = dict(spp=17, bounces=8, seed=4, first_sample=first_sample, reset=False, rows=band)
        pt.render(**call)
        a = _reached(pt, rule, "band (3, 1075) 17 spp from sample %d" % first_sample, 1, 1, w=w, rows=band[1] - band[0], spp=17, cu_count=cu_count, lds_bytes=lds)
        assert a.wg8 >= 15 * cu_count
        call.pop("rows")
        got = _compare(pt, oracle, "Scene1", sc, w, h, wins, band=band, acc_in=caller, **call)
        assert any(not _same_bits(o, caller[h - r[1]:h - r[0], c[0]:c[1]]) for o, (_, c, r) in zip(got, wins))
        acc = pt.accumulator()  # rows outside the band keep the caller's bits
        assert _same_bits(acc[:h - band[1]], caller[:h - band[1]]) and _same_bits(acc[h - band[0]:], caller[h - band[0]:])
    pt.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nan", [False, True], ids=["plain", "nan-alpha"])
def test_five_wave_rows_kernel_at_occupancy(srt, oracle, rule, six_exe, cu_count, nan):
    """(d) Scene1 plus test_gpu_six_waves's `over` count of small spheres: six workgroups' LDS no longer fit into a CU, the launch
    takes k_lds_rows, five waves per SIMD.  1080p, 32 spp.  nan-alpha: with test_gpu_sample_rows's sphere of NaN smoothness ahead
    of the grid, so that a NaN alpha (bit 31 of the row entry's tag word) goes through rows at 32 samples."""
    w, h = 1920, 1080
    first = [nansmooth_sphere(oracle)] if nan else []
    counts = threshold_counts(six_exe, [tuple(o["position"]) + (o["radius"],) for o in first])
    n = counts["over"]
    sc = _objects(oracle, n, first)
    call = dict(spp=32, bounces=8, seed=6)
    wins = _windows(w, h)
    if nan:  # across the sphere's upper edge (it spans about +-207 pixels around column 1064, row 505)
        wins = wins + [("mixed", (1040, 1104), (288, 320))]
    pt = _tracer(srt, sc, w, h)
    pt.render(**call)
    _reached(pt, rule, "Scene1 + %d spheres%s, 1080p 32 spp" % (n, " + NaN smoothness" if nan else ""), 1, 0, w=w, rows=h, spp=32, cu_count=cu_count,
             lds_bytes=counts["bytes"][n])
    got = _compare(pt, oracle, ("over", nan), sc, w, h, wins, **call)
    alpha_nan = [np.isnan(o[..., 3]) for o in got]
    assert any(a.any() for a in alpha_nan) == nan and not all(a.all() for a in alpha_nan)
    pt.close()


@pytest.mark.gpu
def test_row_offsets_beyond_two_gibibytes(srt, oracle, rule, six_exe, cu_count):
    """(e) Scene1, 3840 x 2160, 4 bounces: 32 samples are 129600 tiles x 32 KiB = 3.96 GiB of rows — float4 indices beyond 2^27, byte
    offsets beyond 2^31 — and 33 go over ROWS_MAX_BYTES, so that launch keeps the ring kernel (k_lds) on this frame; then 32 again, into
    the buffer that holds the other frames' leftovers.  A tile's rows lie at tile x samples KiB, tiles numbered block by block, four to
    a block: the windows at the frame's four corners and at both heights inside the ball read tiles from the first MiB, between 2 and 3
    GiB and the last MiB, whichever way the blocks are numbered."""
    w, h = 3840, 2160
    sc = _load(oracle, "Scene1")
    lds = _lds_bytes(six_exe, "Scene1")
    wins = _windows(w, h)
    _check_what_windows_hold(oracle, sc, w, h, wins)
    heights = sorted((r[0] + r[1]) / 2 / h for _, _, r in wins)
    gib = [x * 129600 * 32 / 2**20 for x in heights] + [(1 - x) * 129600 * 32 / 2**20 for x in heights]
    assert sum(2 < g < 3 for g in gib[:len(heights)]) >= 1 and sum(2 < g < 3 for g in gib[len(heights):]) >= 1, gib
    with _tracer(srt, sc, w, h) as pt:  # (4 GiB of rows: closed before the next test, whatever happens)
        for seed, spp in enumerate((32, 33, 32)):
            call = dict(spp=spp, bounces=4, seed=seed)
            pt.render(**call)
            a = _reached(pt, rule, "4K %d spp" % spp, 1 if spp == 32 else 0, 1, w=w, rows=h, spp=spp, cu_count=cu_count, lds_bytes=lds)
            assert a.rows_bytes == (129600 * 32 * 1024 if spp == 32 else 0)
            _compare(pt, oracle, "Scene1", sc, w, h, wins, **call)


def test_rule_answers(rule):
    """rows_rule_check --ask (a stand-alone program under ASan + UBSan) on the requests of the cases above, for 256 CUs and for parts
    with other counts: the threshold frame has exactly 15 blocks per CU and sits on the threshold; a line that does not parse is an
    error"""
    import subprocess

    ask = lambda **q: rows_rule.ask(rule, [dict(dict(cu_count=256, lds_bytes=23776), **q)])[0]
    assert ask(w=1920, rows=1080, spp=32) == (8, 1, 8160, 1, 1, 8160 * 4 * 32 * 1024)
    assert ask(w=1920, rows=1072, spp=17)[:4] == (8, 1, 8040, 1)
    assert ask(w=1920, rows=135, spp=32)[0] < 8 and ask(w=1920, rows=135, spp=32).rows == 0
    assert ask(w=3840, rows=2160, spp=32) == (8, 1, 32400, 1, 1, 129600 * 32 * 1024)
    assert ask(w=3840, rows=2160, spp=33) == (8, 1, 32400, 0, 1, 0)
    assert ask(w=1920, rows=1080, spp=32, lds_bytes=27040)[3:5] == (1, 0)
    assert ask(w=1920, rows=1080, spp=64).chunks >= 2 and ask(w=1920, rows=1080, spp=64).rows == 0
    for q in (dict(mesh=True), dict(preview=True), dict(steps=2), dict(block_grid=True), dict(scene_in_lds=False), dict(spp=1)):
        assert ask(**dict(dict(w=1920, rows=1080, spp=8), **q)).rows == 0, q
    assert _threshold_frame(256) == (1280, 768)
    for cu in (64, 104, 256, 304):
        w, h = _threshold_frame(cu)
        assert (w // 16) * (h // 16) == 15 * cu and w % 16 == 0 and h % 16 == 0 and w >= 128 and h >= 128, (cu, w, h)
        for spp in (16, 63):
            assert ask(w=w, rows=h, spp=spp, cu_count=cu)[:4] == (8, 1, 15 * cu, 1), (cu, spp)
        assert ask(w=w, rows=h - 16, spp=16, cu_count=cu)[0] < 8 and ask(w=w, rows=h - 16, spp=16, cu_count=cu).rows == 0
    for text in ("1920 1080 32 256 0 0 1 0 1\n", "1920 1080 x\n", "0 1080 32 256 0 0 1 0 1 0\n"):
        assert subprocess.run([rule, "--ask"], input=text, capture_output=True, text=True).returncode == 2, text
    assert subprocess.run([rule, "--ask"], input="", capture_output=True, text=True).stdout == ""
