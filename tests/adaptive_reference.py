"""The definitions of srt_render_adaptive rule 1 and of srt_sample_budget (include/srt_pathtrace.h) restated in numpy, written from
the header text.  srt_sample_budget is binary32 without FMA and the GPU test compares bits, so everything here is float32 arithmetic,
one rounding per operation; `lum` is variance_reference's (it keeps the dtype it is given) and `prefilter32` is variance_reference's
prefilter in binary32 and in the header's order (dy outer, dx inner) — test_adaptive_reference.py holds the two against each other
where float64 is exact.  Inputs are the arrays the pass reads (scene rows): accumulator (H, W, 4) float32, variance (H, W) float32,
counts (H, W) uint32, object (H, W) int32, albedo (H, W, 4) float32."""
import numpy as np

from variance_reference import K3, lum

FRAME_LIMIT = 2147483646
F = np.float32


def effective_budget(budget, counts, max_samples):
    """Rule 1: e_p = min(b_p, max_samples, 2147483646 - n_p), 0 when n_p >= 2147483646."""
    b, n = np.asarray(budget, np.int64), np.asarray(counts, np.int64)
    return np.where(n >= FRAME_LIMIT, 0, np.minimum(np.minimum(b, int(max_samples)), FRAME_LIMIT - n)).astype(np.uint32)


def prefilter32(v, obj):
    """g_p of srt_denoise_variance rule A at level 0 in binary32: taps dy outer, dx inner, over the taps inside the frame with
    o_q == o_p (the centre always); the working variance is v on hit pixels.  Defined on hit pixels; 0 elsewhere."""
    H, W = obj.shape
    v = np.where(obj >= 0, v, F(0)).astype(F)
    ys, xs = np.mgrid[0:H, 0:W]
    sk, sg = np.zeros((H, W), F), np.zeros((H, W), F)
    with np.errstate(all="ignore"):
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                qy, qx = ys + dy, xs + dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                take = inside & (obj[qy, qx] == obj) if (dx or dy) else inside
                k = F(K3[dx + 1]) * F(K3[dy + 1])
                sk = np.where(take, sk + k, sk).astype(F)
                sg = np.where(take, sg + k * v[qy, qx], sg).astype(F)
        g = (sg / sk).astype(F)
    return np.where(obj >= 0, g, F(0)).astype(F)


def demod32(alb, albedo):
    """srt_variance rule 2: per channel m = a >= 1e-3 ? a : 1 with the flag."""
    a = alb[..., :3].astype(F)
    return np.where(a >= F(1e-3), a, F(1)).astype(F)


def sample_budget(acc, var, counts, obj, alb, threshold, floor, max_budget, albedo):
    """srt_sample_budget: (b (H, W) uint32, total)."""
    threshold, floor = F(threshold), F(floor)
    n = np.asarray(counts, np.uint32)
    with np.errstate(all="ignore"):
        g = prefilter32(np.asarray(var, F), obj)
        c = acc[..., :3].astype(F)
        if albedo:
            c = (c / demod32(alb, True)).astype(F)
        l = lum(c).astype(F)
        assert l.dtype == F
        t = (threshold * (l + floor).astype(F)).astype(F)
        T = (t * t).astype(F)
        r = (g / T).astype(F)
        nf = n.astype(F)
        e = ((nf * r).astype(F) - nf).astype(F)
        mb = F(max_budget)
        capped = ~(e < mb)
        b = np.where(capped, np.uint32(max_budget), np.maximum(1, np.ceil(np.where(capped, F(0), e)).astype(np.int64))).astype(np.uint32)
        b = np.where(g > T, b, 0)
    b = np.where((obj < 0) | (n == 0), 0, b).astype(np.uint32)
    return b, int(b.astype(np.uint64).sum())
