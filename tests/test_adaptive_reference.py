"""Hand-computed cases for tests/adaptive_reference.py (the numpy restatement of srt_render_adaptive rule 1 and of srt_sample_budget
that test_gpu_budget.py compares the GPU with, bit for bit), and its binary32 prefilter against variance_reference's float64 one
where float64 is exact.  No GPU."""
import numpy as np

import adaptive_reference as ar
import variance_reference as vr

F = np.float32


def test_effective_budget_by_hand():
    b = [0, 5, 5000, 100, 5, 5, 7]
    n = [3, 0, 0, 10, 2147483644, 2147483646, 0xFFFFFFFF]
    assert ar.effective_budget(b, n, 4096).tolist() == [0, 5, 4096, 100, 2, 0, 0]
    assert ar.effective_budget([100], [0], 9).tolist() == [9]
    assert ar.effective_budget([1], [2147483645], 4096).tolist() == [1]


def _flat(h=3, w=3, v=0.0, n=4, c=(1.0, 1.0, 1.0)):
    acc = np.zeros((h, w, 4), F)
    acc[..., :3] = c
    # (every pixel its own object: g = v)
    return dict(acc=acc, var=np.full((h, w), v, F), counts=np.full((h, w), n, np.uint32), obj=np.arange(h * w, dtype=np.int32).reshape(h, w),
                alb=np.ones((h, w, 4), F))


def test_budget_of_a_flat_frame_by_hand():
    # lum(1, 1, 1) = (0.2126f + 0.7152f) + 0.0722f = 1 (in binary32); floor 0, threshold 0.5 -> T = 0.25; v = 1 everywhere ->
    # g = 1, r = 4, e = 4 * 4 - 4 = 12
    k = _flat(v=1.0)
    assert ar.lum(k["acc"][..., :3])[0, 0] == F(1.0)
    b, total = ar.sample_budget(threshold=0.5, floor=0.0, max_budget=64, albedo=False, **k)
    assert b.dtype == np.uint32 and (b == 12).all() and total == 9 * 12
    # the cap: !(e < max) takes max_budget, equality included
    assert (ar.sample_budget(threshold=0.5, floor=0.0, max_budget=12, albedo=False, **k)[0] == 12).all()
    assert (ar.sample_budget(threshold=0.5, floor=0.0, max_budget=11, albedo=False, **k)[0] == 11).all()
    # g == T exactly: no budget; one ulp above: r rounds to 1 + 2^-23, e = 4 * 2^-23 -> ceil = 1
    k = _flat(v=0.25)
    assert (ar.sample_budget(threshold=0.5, floor=0.0, max_budget=64, albedo=False, **k)[0] == 0).all()
    k = _flat(v=float(np.nextafter(F(0.25), F(1))))
    assert (ar.sample_budget(threshold=0.5, floor=0.0, max_budget=64, albedo=False, **k)[0] == 1).all()
    # the floor: l + floor = 2 -> T = 1 -> v = 1 is converged
    k = _flat(v=1.0)
    assert (ar.sample_budget(threshold=0.5, floor=1.0, max_budget=64, albedo=False, **k)[0] == 0).all()
    # demodulation: albedo 0.5 doubles the luminance (T = 1); an albedo below 1e-3 divides by 1 (T = 0.25)
    k["alb"][...] = 0.5
    assert (ar.sample_budget(threshold=0.5, floor=0.0, max_budget=64, albedo=True, **k)[0] == 0).all()
    k["alb"][...] = 1e-4
    assert (ar.sample_budget(threshold=0.5, floor=0.0, max_budget=64, albedo=True, **k)[0] == 12).all()


def test_misses_empty_pixels_and_special_values_by_hand():
    k = _flat(h=1, w=8, v=1.0)
    k["obj"][0, 1] = -1
    k["counts"][0] = [4, 4, 0, 1, 4, 4, 4, 2**31]
    k["var"][0] = [1.0, 1.0, 1.0, 1.0, np.inf, np.nan, 0.0, 0.5]
    b, total = ar.sample_budget(threshold=0.5, floor=0.0, max_budget=4096, albedo=False, **k)
    # hit n=4: 12 | miss: 0 | n = 0: 0 | n = 1: 1 * 4 - 1 = 3 | +inf: the cap | NaN: 0 | 0: 0 | n = 2^31, r = 2: e = 2^31 -> the cap
    assert b[0].tolist() == [12, 0, 0, 3, 4096, 0, 0, 4096] and total == 12 + 3 + 2 * 4096
    # a T that underflows to 0 (threshold 1e-30: t = 1e-30, t * t = 0): every positive variance takes the cap, a zero one nothing
    b, _ = ar.sample_budget(threshold=1e-30, floor=0.0, max_budget=77, albedo=False, **k)
    assert b[0].tolist() == [77, 0, 0, 77, 77, 0, 0, 77]
    # threshold +inf: T = +inf, nothing exceeds it (inf > inf is false)
    b, _ = ar.sample_budget(threshold=np.inf, floor=0.0, max_budget=77, albedo=False, **k)
    assert not b.any()


def test_two_objects_in_a_window_by_hand():
    # a 1 x 3 row, objects 0 0 1, variances 1 3 100: g_0 = (2/4 * 1 + 1/4 * 3) / (3/4) = 5/3 (the tap on object 1 is skipped),
    # g_1 = (1/4 * 1 + 2/4 * 3) / (3/4) = 7/3, g_2 = 100
    obj = np.array([[0, 0, 1]], np.int32)
    v = np.array([[1, 3, 100]], F)
    g = ar.prefilter32(v, obj)
    want = [F(F(1.25) / F(0.75)), F(F(1.75) / F(0.75)), F(100)]
    assert g[0].tolist() == [float(x) for x in want]
    # a miss has no working variance and is no tap
    obj[0, 1] = -1
    assert ar.prefilter32(v, obj)[0].tolist() == [1.0, 0.0, 100.0]


def test_the_binary32_prefilter_equals_variance_reference_where_float64_is_exact():
    rng = np.random.default_rng(5)
    obj = rng.integers(-1, 3, size=(13, 21)).astype(np.int32)
    v = rng.integers(0, 1 << 12, size=obj.shape).astype(F)  # small integers: every product and partial sum is exact in both
    g64 = vr.prefilter(np.where(obj >= 0, v, 0).astype(np.float64), obj)
    g32 = ar.prefilter32(v, obj)
    hit = obj >= 0
    assert np.array_equal(g32[hit], g64[hit].astype(F))  # (one division, rounded once: float64 -> float32 is innocuous here)
