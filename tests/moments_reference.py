"""The float64 definition of the luminance moments of the temporal history (srt_moments_output: the records
srt_temporal_accumulate keeps) and of srt_temporal_variance, restated from include/srt_pathtrace.h.  Used by
tests/test_moments_abi.py (against cases worked by hand) and tests/test_gpu_moments.py (against the kernels)."""
import math

import numpy as np

LUM = tuple(float(np.float32(v)) for v in (0.2126, 0.7152, 0.0722))


def lum(rgb):
    """(0.2126f r + 0.7152f g) + 0.0722f b with the float32 coefficients, in float64."""
    rgb = np.asarray(rgb, np.float64)
    return (LUM[0] * rgb[..., 0] + LUM[1] * rgb[..., 1]) + LUM[2] * rgb[..., 2]


def frame_luminance(acc, albedo=None):
    """mu_p = lum(c_p / m_p): m_p = the albedo per channel where it is >= 1e-3, else 1; albedo None: no demodulation."""
    c = np.asarray(acc, np.float64)[..., :3]
    if albedo is not None:
        a = np.asarray(albedo, np.float64)[..., :3]
        c = c / np.where(a >= float(np.float32(1e-3)), a, 1.0)
    return lum(c)


def ray_basis(cam, w, h):
    """The float32 columns right * rd, up * ld, forward * clip that srt_render folds from a camera, as float64."""
    f32 = np.float32
    clip = f32(0.01)
    aspect = f32(w) / f32(h)
    hfov = f32(cam.fov_degrees * 3.14159265358979323846 / 180.0)
    t = f32(math.tan(float(hfov / f32(2))))
    rd, ld = (clip * t) * aspect, clip * t
    r = np.array(cam.right[:], f32) * rd
    u = np.array(cam.up[:], f32) * ld
    f = np.array(cam.forward[:], f32) * clip
    return np.stack([r, u, f], 1).astype(np.float64)


def taps(obj, nd, pos, prev, sigma_t, thr):
    """The temporal tap rule (srt_temporal_accumulate rules 2-3) without object motion.  prev: dict(cam, obj, nd, pos) of the
    previous call.  For the four taps of every pixel: lists of (weight w_q (0 where the tap does not count), row, column), and
    `edge`, the smallest relative distance of any decision of the pixel from its threshold (the projection window, the floor
    of u and v, the plane and the normal test); a pixel with edge > 1e-3 has an unambiguous tap set."""
    H, W = obj.shape
    hit = obj >= 0
    Bi = np.linalg.inv(ray_basis(prev["cam"], W, H)).astype(np.float32).astype(np.float64)
    rel = pos[..., :3].astype(np.float64) - np.array(prev["cam"].position[:], np.float32).astype(np.float64)
    abg = rel @ Bi.T
    a, b, g = abg[..., 0], abg[..., 1], abg[..., 2]
    with np.errstate(all="ignore"):
        u = (a / g + 1) * W / 2
        v = (b / g + 1) * H / 2
    ok = hit & (g > 0) & (u > -1) & (u < W) & (v > -1) & (v < H)
    edge = np.where(hit, np.abs(g) / np.maximum(np.linalg.norm(rel, axis=2), 1e-30), np.inf)
    uu, vv = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
    x0, y0 = np.floor(uu).astype(np.int64), np.floor(vv).astype(np.int64)
    fx, fy = uu - x0, vv - y0
    edge = np.minimum(edge, np.where(ok, np.minimum(np.minimum(fx, 1 - fx), np.minimum(fy, 1 - fy)), np.inf))
    n_p, d_p, x_p = nd[..., :3].astype(np.float64), nd[..., 3].astype(np.float64), pos[..., :3].astype(np.float64)
    tol = sigma_t * d_p
    out = []
    for k in range(4):
        qx, qy = x0 + (k & 1), y0 + (k >> 1)
        wq = np.where(k & 1, fx, 1 - fx) * np.where(k >> 1, fy, 1 - fy)
        inside = ok & (wq > 0) & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
        cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
        same = inside & (prev["obj"][cy, cx] == obj)
        dist = np.abs(np.sum(n_p * (prev["pos"][cy, cx, :3].astype(np.float64) - x_p), axis=2))
        with np.errstate(all="ignore"):
            edge = np.minimum(edge, np.where(same, np.abs(dist - tol) / tol, np.inf))
        counted = same & (dist <= tol)
        if thr > -1:
            dot = np.sum(n_p * prev["nd"][cy, cx, :3].astype(np.float64), axis=2)
            edge = np.minimum(edge, np.where(counted, np.abs(dot - thr) / max(abs(thr), 1e-3), np.inf))
            counted &= dot >= thr
        out.append((np.where(counted, wq, 0.0), cy, cx))
    return out, edge


def blend(mu, obj, tap_list, mom_prev, n, max_samples):
    """The records (H, W, 3) = (M1, M2, Lm) of one call.  mu: this frame's luminance; tap_list: taps()[0], or None when the
    colour history is invalid; mom_prev: the previous records (H, W, >= 3), or None when the moments history is invalid."""
    hit = obj >= 0
    mu = np.asarray(mu, np.float64)
    out = np.stack([mu, mu * mu, np.full(obj.shape, float(n))], -1)
    if tap_list is not None and mom_prev is not None:
        mp = np.asarray(mom_prev, np.float64)
        sw = np.zeros(obj.shape)
        s = np.zeros(obj.shape + (3,))
        for w, cy, cx in tap_list:
            sw += w
            s += w[..., None] * np.where((w > 0)[..., None], mp[cy, cx, :3], 0.0)
        with np.errstate(all="ignore"):
            Lm = np.minimum(s[..., 2] / sw + n, max_samples)
            a = n / Lm
            m1 = (1 - a) * (s[..., 0] / sw) + a * mu
            m2 = (1 - a) * (s[..., 1] / sw) + a * (mu * mu)
        out = np.where((sw > 0)[..., None], np.stack([m1, m2, Lm], -1), out)
    return np.where(hit[..., None], out, 0.0)


def temporal_variance(mom, obj, n, min_frames, radius):
    """srt_temporal_variance: (variance (H, W), young (H, W) bool).  mom: (H, W, >= 3) records (M1, M2, Lm)."""
    H, W = obj.shape
    m = np.asarray(mom, np.float64)
    old = float(np.float32(min_frames) * np.float32(n))
    v = np.zeros((H, W))
    young = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            o = obj[y, x]
            if o < 0:
                continue
            m1, m2, lm = m[y, x, :3]
            if not lm >= old:
                young[y, x] = True
                a1 = a2 = 0.0
                cnt = 0
                for dy in range(-radius, radius + 1):
                    for dx in range(-radius, radius + 1):
                        qx, qy = x + dx, y + dy
                        if qx < 0 or qx >= W or qy < 0 or qy >= H or obj[qy, qx] != o:
                            continue
                        a1 += m[qy, qx, 0]
                        a2 += m[qy, qx, 1]
                        cnt += 1
                m1, m2 = a1 / cnt, a2 / cnt
            with np.errstate(all="ignore"):
                s = m2 - m1 * m1
                v[y, x] = (s if s > 0 else 0.0) * (n / lm)  # (fmaxf(0, NaN) = 0)
    return v, young
