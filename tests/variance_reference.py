"""The definitions of srt_variance and srt_denoise_variance (include/srt_pathtrace.h) restated in float64 numpy, written from the
header text.  Inputs are the float32 arrays the passes read (scene rows): halves / accumulator (H, W, 4), object (H, W) int32,
normal_depth, position, albedo (H, W, 4), variance (H, W)."""
import numpy as np

H5 = np.array([1, 4, 6, 4, 1], np.float64) / 16
K3 = np.array([1, 2, 1], np.float64) / 4
FLT_MAX = float(np.finfo(np.float32).max)
EPS = float(np.float32(1e-10))
LUM = tuple(float(np.float32(v)) for v in (0.2126, 0.7152, 0.0722))


def lum(c):
    """(0.2126 r + 0.7152 g) + 0.0722 b with the binary32 constants."""
    return (LUM[0] * c[..., 0] + LUM[1] * c[..., 1]) + LUM[2] * c[..., 2]


def demod(alb, albedo):
    """Rule 2 of srt_denoise: per channel m = a >= 1e-3 ? a : 1 with the flag, else 1."""
    if not albedo:
        return np.ones(alb.shape[:2] + (3,))
    a = alb[..., :3]
    return np.where(a >= np.float32(1e-3), a.astype(np.float64), 1.0)


def variance(a, b, obj, alb, albedo):
    """srt_variance: (v, mean) — v (H, W) float64, 0 on misses; mean (H, W, 3) the merged rgb of every pixel."""
    m = demod(alb, albedo)
    a3, b3 = a[..., :3].astype(np.float64), b[..., :3].astype(np.float64)
    with np.errstate(all="ignore"):
        d = 0.5 * lum(a3 / m) - 0.5 * lum(b3 / m)
        v = np.where(obj >= 0, d * d, 0.0)
        mean = 0.5 * a3 + 0.5 * b3
    return v, mean


def prefilter(v, obj):
    """g_p: the 3 x 3 [1,2,1] x [1,2,1] / 16 mean of v over the taps inside the frame with o_q == o_p (the centre always)."""
    H, W = obj.shape
    ys, xs = np.mgrid[0:H, 0:W]
    sk, sg = np.zeros((H, W)), np.zeros((H, W))
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            qy, qx = ys + dy, xs + dx
            inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
            qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
            take = inside & (obj[qy, qx] == obj) if (dx or dy) else inside
            k = K3[dx + 1] * K3[dy + 1]
            sk += np.where(take, k, 0.0)
            with np.errstate(all="ignore"):
                kv = k * np.where(take, v[qy, qx], 0.0)
                # The header's rule for the products: one at or below 2^-150, half the smallest subnormal, is 0.  Only that
                # flush to zero is modelled; a product between 2^-150 and 2^-126 stays unrounded here while binary32 rounds
                # it to a subnormal: a change of g_p of less than 2^-149 per tap, far below what any weight can show.
                sg += np.where(take & (kv > 2.0 ** -150), kv, 0.0)
    with np.errstate(all="ignore"):
        return sg / sk


def denoise_variance(acc, var, obj, nd, pos, alb, iterations, sigma_luminance, sigma_normal, sigma_plane, albedo, levels_out=None):
    """srt_denoise_variance: the (H, W, 4) result.  levels_out, a list, receives every level's working variance."""
    H, W = obj.shape
    hit = obj >= 0
    m = demod(alb, albedo)
    with np.errstate(all="ignore"):
        c = acc[..., :3].astype(np.float64) / m
    v = np.where(hit, var.astype(np.float64), 0.0)
    n = nd[..., :3].astype(np.float64)
    d = nd[..., 3].astype(np.float64)
    x = pos[..., :3].astype(np.float64)
    sl = min(float(sigma_luminance), FLT_MAX)  # one above FLT_MAX counts as FLT_MAX
    ys, xs = np.mgrid[0:H, 0:W]
    for i in range(iterations):
        s = 1 << i
        if sl > 0:
            with np.errstate(all="ignore"):
                scale = 1.0 / (sl * np.sqrt(prefilter(v, obj)) + EPS)
            lc = lum(c)
        sw = np.zeros((H, W))
        sc = np.zeros((H, W, 3))
        sv = np.zeros((H, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + s * dy, xs + s * dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                w = np.full((H, W), H5[dx + 2] * H5[dy + 2])
                cq, vq = c[qy, qx], v[qy, qx]
                if dx or dy:
                    take = inside & hit & (obj[qy, qx] == obj)
                    with np.errstate(all="ignore"):
                        if sigma_normal > 0:
                            w = w * np.maximum(0.0, np.sum(n * n[qy, qx], axis=2)) ** sigma_normal
                        if sigma_plane > 0:
                            w = w * np.exp(-np.abs(np.sum(n * (x[qy, qx] - x), axis=2)) / (sigma_plane * d))
                        if sl > 0:
                            dl = np.abs(lc - lc[qy, qx])
                            w = w * np.where(dl == 0, 1.0, np.exp(-dl * scale))  # an exact tie keeps its weight 1
                else:
                    take = inside
                w = np.where(take, w, 0.0)
                sw += w
                sc += np.where(take[..., None], w[..., None] * np.where(take[..., None], cq, 0.0), 0.0)
                with np.errstate(all="ignore"):
                    sv += np.where(take, w * w * np.where(take, vq, 0.0), 0.0)
        with np.errstate(all="ignore"):
            c = np.where(hit[..., None], sc / sw[..., None], c)
            v = np.where(hit, sv / (sw * sw), v)
        if levels_out is not None:
            levels_out.append(v.copy())
    out = np.empty((H, W, 4))
    out[..., :3] = c * m
    out[..., 3] = acc[..., 3]
    out[~hit] = acc[~hit]
    return out
