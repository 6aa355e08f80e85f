"""srt_sample_budget (ABI 7) on the MI355X against tests/adaptive_reference.py, bit for bit (the budget is an integer map; every
pixel is compared) on crafted inputs written through the write and bind calls: variances 0, subnormal, huge, +inf and NaN; counts
0, 1 and 2^31; misses; two objects meeting inside a 3 x 3 window; a prefiltered variance exactly equal to T and one ulp above; a T
that underflows to 0 and one that is +inf; both ALBEDO settings.  24 x 20 is whole tiles and a half row of them, 21 x 13 has partial
tile columns and rows and two workgroups whose prefilter tiles meet."""
import numpy as np
import pytest

import adaptive_reference as ar

pytestmark = pytest.mark.gpu

F = np.float32
PARAMS = [(0.5, 0.0, 64), (0.05, 0.01, 4096), (1e-30, 0.0, 77), (float("inf"), 0.0, 5), (0.2, 0.5, 1)]


def crafted(w, h):
    """The inputs of the pass, scene rows."""
    rng = np.random.default_rng(w * 1000 + h)
    ys, xs = np.mgrid[0:h, 0:w]
    obj = np.where(xs + ys // 3 < w // 2, 0, 1).astype(np.int32)  # two objects along a stepped edge
    obj[rng.random((h, w)) < 0.06] = -1                              # misses, some on the edge
    var = (rng.random((h, w)) ** 4 * 0.05).astype(F)
    counts = rng.integers(1, 40, size=(h, w)).astype(np.uint32)
    acc = np.zeros((h, w, 4), F)
    acc[..., :3] = rng.random((h, w, 3)) * 2
    acc[..., 3] = rng.random((h, w))
    alb = np.zeros((h, w, 4), F)
    alb[..., :3] = 0.2 + 0.8 * rng.random((h, w, 3))
    alb[rng.random((h, w)) < 0.05, 1] = 5e-4  # below 1e-3: that channel is not divided
    # special values inside the two objects: they reach their neighbours' windows too
    for k, v in enumerate((0.0, 1e-42, 1e38, np.inf, np.nan, 3e-39)):
        var[2 + 2 * (k % 3), 3 + 6 * (k // 3)] = v
        var[h - 2 - (k % 3), w - 2 - 4 * (k // 3)] = v
    counts[1, 1:4] = (0, 1, 2**31)
    counts[h - 1, w - 3:w] = (2**31, 1, 0)
    acc[3, 1, :3] = 0.0  # a black pixel: only the floor keeps T above 0
    # a row of pixels that are each their own object, white with albedo 1: g = v and l = 1 exactly, whichever the ALBEDO setting
    y = h // 2
    own = slice(2, 12)
    obj[y, own] = 100 + np.arange(10)
    acc[y, own, :3] = 1.0
    alb[y, own, :3] = 1.0
    counts[y, own] = (4, 4, 4, 1, 0, 2**31, 4, 4, 7, 4)
    var[y, own] = (0.25, np.nextafter(F(0.25), F(1)), 1.0, 1.0, 1.0, 0.5, np.inf, np.nan, 0.0, np.nextafter(F(0.25), F(0)))
    return dict(acc=acc, var=var, counts=counts, obj=obj, alb=alb)


@pytest.fixture(scope="module", params=[(24, 20), (21, 13)])
def frame(request, srt):
    import torch

    w, h = request.param
    k = crafted(w, h)
    pt = srt.PathTracer(w, h)
    dev = "cuda:%d" % pt.device
    t = dict(var=torch.from_numpy(k["var"]).to(dev), obj=torch.from_numpy(k["obj"]).to(dev), alb=torch.from_numpy(k["alb"]).to(dev))
    torch.cuda.synchronize()
    pt.bind_variance(t["var"])
    pt.bind_gbuffer("object", t["obj"])
    pt.bind_gbuffer("albedo", t["alb"])
    pt.write_accumulator(k["acc"])
    pt.write_sample_counts(k["counts"])
    yield pt, k, t
    pt.close()


def test_the_reference_sees_every_case(frame):
    """The crafted inputs do what the docstring says, by the reference's own intermediate values."""
    _, k, _ = frame
    h, w = k["obj"].shape
    y = h // 2
    b, _ = ar.sample_budget(threshold=0.5, floor=0.0, max_budget=64, albedo=True, **k)
    # g == T: 0 | one ulp above: 1 | 4 * 4 - 4 | 1 * 4 - 1 | n = 0 | n = 2^31: the cap | +inf: the cap | NaN | 0 | one ulp below
    assert b[y, 2:12].tolist() == [0, 1, 12, 3, 0, 64, 64, 0, 0, 0]
    g = ar.prefilter32(k["var"], k["obj"])
    hit = k["obj"] >= 0
    assert np.isnan(g[hit]).any() and np.isinf(g[hit]).any() and (g[hit] == 0).any() and (g[hit] > 1e37).any()
    edge = hit & (np.roll(k["obj"], 1, axis=1) != k["obj"]) & (np.roll(k["obj"], 1, axis=1) >= 0)
    assert edge.sum() >= h // 2 and (k["obj"] < 0).sum() >= 5


@pytest.mark.parametrize("albedo", [True, False])
@pytest.mark.parametrize("threshold,floor,max_budget", PARAMS)
def test_the_budget_equals_the_reference_bit_for_bit(frame, threshold, floor, max_budget, albedo):
    pt, k, t = frame
    want, total = ar.sample_budget(threshold=threshold, floor=floor, max_budget=max_budget, albedo=albedo, **k)
    pt.sample_budget(threshold=threshold, floor=floor, max_budget=max_budget, albedo=albedo)
    got = pt.sample_budget_map()
    print("%dx%d tau=%g floor=%g max=%d albedo=%d: total %d, %d pixels with a budget, %d at the cap" %
          (pt.width, pt.height, threshold, floor, max_budget, albedo, total, int((want > 0).sum()), int((want == max_budget).sum())))
    assert got.dtype == np.uint32 and np.array_equal(got, want), "%d pixels differ" % int((got != want).sum())
    assert pt.budget_total() == total
    if threshold == float("inf"):
        assert total == 0
    elif threshold == 1e-30:
        assert set(np.unique(want)) == {0, max_budget}
    else:
        assert 0 < (want > 0).sum() < want.size
    # the inputs are as they were
    assert np.array_equal(t["var"].cpu().numpy().view(np.uint32), k["var"].view(np.uint32))
    assert np.array_equal(pt.sample_counts(), k["counts"]) and np.array_equal(pt.accumulator().view(np.uint32), k["acc"].view(np.uint32))


def test_a_bound_budget_tensor_receives_the_map_and_keeps_its_sentinel(frame):
    import torch

    pt, k, t = frame
    h, w = k["obj"].shape
    tb = torch.full((h * w + 64,), -7, dtype=torch.int32, device=t["var"].device)
    torch.cuda.synchronize()
    pt.bind_sample_budget(tb[:h * w].view(h, w))
    try:
        pt.sample_budget(threshold=0.05, floor=0.01, max_budget=64, albedo=True)
        want, total = ar.sample_budget(threshold=0.05, floor=0.01, max_budget=64, albedo=True, **k)
        assert pt.budget_total() == total
        host = tb.cpu().numpy()
        assert np.array_equal(host[:h * w].reshape(h, w).view(np.uint32), want) and (host[h * w:] == -7).all()
    finally:
        pt.bind_sample_budget(None)
