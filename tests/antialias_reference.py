"""The anti-aliasing resolve (srt_antialias) restated in float64 numpy from the text of include/srt_pathtrace.h, not from the
kernel.  Shared by tests/test_antialias_abi.py (hand-worked cases, no GPU) and tests/test_gpu_antialias.py."""
import math

import numpy as np


def offsets(k):
    """Step 1: the k sub-sample offsets of an axis, (float)(2i - (k-1)) / (float)(2k) in binary32."""
    return np.array([np.float32(2 * i - (k - 1)) / np.float32(2 * k) for i in range(k)], np.float32)


def _shifted(a, ax, ay, fill):
    """a[y + ay, x + ax] per pixel (x, y), `fill` outside the frame, and the mask of pixels whose tap lies inside."""
    h, w = a.shape[:2]
    out = np.full(a.shape, fill, a.dtype)
    inside = np.zeros((h, w), bool)
    ys, yd = slice(max(ay, 0), h + min(ay, 0)), slice(max(-ay, 0), h - max(ay, 0))
    xs, xd = slice(max(ax, 0), w + min(ax, 0)), slice(max(-ax, 0), w - max(ax, 0))
    out[yd, xd] = a[ys, xs]
    inside[yd, xd] = True
    return out, inside


def resolve(c, obj, sub):
    """c (H, W, 4) float32, obj (H, W) int32, sub (K, H, W) int32.  Returns the result (H, W, 4) float64, the mask of pixels
    with a foreign sub-sample, and the mask of pixels some C_s of which came from taps (the others keep their input bits)."""
    K, h, w = sub.shape
    k = math.isqrt(K)
    assert k * k == K and obj.shape == (h, w) and c.shape == (h, w, 4)
    off = offsets(k).astype(np.float64)
    c3 = c[..., :3].astype(np.float64)
    total = np.zeros((h, w, 3))
    foreign_any = np.zeros((h, w), bool)
    changed = np.zeros((h, w), bool)
    for s in range(K):
        dx, dy = off[s % k], off[s // k]
        foreign = sub[s] != obj
        foreign_any |= foreign
        sw = np.zeros((h, w))
        sc = np.zeros((h, w, 3))
        for ay in (-1, 0, 1):          # fixed order: ay outer, ax inner
            for ax in (-1, 0, 1):
                wq = max(0.0, 1.0 - abs(ax - dx)) * max(0.0, 1.0 - abs(ay - dy))
                if wq == 0.0:
                    continue
                oq, inside = _shifted(obj, ax, ay, 0)
                cq, _ = _shifted(c3, ax, ay, np.nan)
                counts = foreign & inside & (oq == sub[s])
                sw += np.where(counts, wq, 0.0)
                sc += np.where(counts[..., None], wq * np.where(counts[..., None], cq, 0.0), 0.0)  # skipped taps are never read
        solved = sw > 0
        with np.errstate(all="ignore"):
            cs = np.where(solved[..., None], sc / np.where(solved, sw, 1.0)[..., None], c3)
        changed |= solved
        total += cs
    out = c.astype(np.float64).copy()
    out[..., :3] = np.where(changed[..., None], total / K, c3)
    return out, foreign_any, changed
