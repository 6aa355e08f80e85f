"""Inputs shared by tests/test_gpu_pass_edges.py (the kernels on the MI355X) and tests/test_pass_references.py (the float64
definitions alone, on the CPU): the frame shapes, synthetic guides that exist at every shape, guides with exact ties for the
upsampler's parameter extremes, object maps with borders on the tile and workgroup seams, piecewise-constant colours, and the
moving-object frames.  Everything here is numpy; nothing touches a GPU."""
import numpy as np

import test_gpu_motion as mo
import test_gpu_temporal as tp
from test_gpu_filter_edges import SHAPES as FILTER_SHAPES

# (33, 18): three workgroups across with a partial last one, two down
SHAPES = list(FILTER_SHAPES) + [(33, 18)]
INF = float("inf")
F32_MAX = float(np.finfo(np.float32).max)


def f32(v):
    return float(np.float32(v))


# ---- guides that exist at every shape -------------------------------------------------------------------------------------
def guides(w, h, seed):
    """(acc, obj, nd, pos, alb) in the style of test_gpu_upsample.synthetic and test_gpu_denoise.synthetic, at any shape down to
    one pixel: blobs of smoothly varying normals (one object's stay within an acute angle), points and depths, scattered misses
    and a block of them, a one-pixel-wide column and row object where the frame has room, positive noisy colours, alphas of
    0, 1 and 0.5, and some albedo channels below 1e-3.  Pixel (0, 0) is always a hit."""
    rng = np.random.default_rng(seed)
    n = min(5, max(1, w * h // 4))
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy = rng.uniform(0, w, n), rng.uniform(0, h, n)
    obj = np.argmin(np.stack([np.hypot(xs - cx[k], ys - cy[k]) for k in range(n)]), axis=0).astype(np.int32)
    obj[rng.random((h, w)) < 0.04] = -1
    if w >= 5 and h >= 5:
        obj[(xs < w * 0.2) & (ys > h * 0.6)] = -1
    if w >= 4:
        obj[:, w // 2 + 1] = n
    if h >= 4:
        obj[h // 3 + 1, :] = n + 1
    if obj[0, 0] < 0:
        obj[0, 0] = 0
    k = np.maximum(obj, 0)
    base_n = rng.normal(size=(n + 2, 3))
    base_n *= 2.0 / np.linalg.norm(base_n, axis=1, keepdims=True)
    nrm = base_n[k] + 0.25 * np.stack([np.sin(xs / 7.0), np.cos(ys / 5.0), np.sin((xs + ys) / 11.0)], -1)
    nrm += 0.02 * rng.normal(size=nrm.shape)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    depth = 2.0 + 3.0 * rng.random(n + 2)[k] + 0.01 * xs
    pnt = np.stack([xs * 0.01, ys * 0.01, depth], -1) + 0.002 * rng.normal(size=(h, w, 3))
    nd = np.concatenate([nrm, depth[..., None]], -1).astype(np.float32)
    pos = np.concatenate([pnt, np.ones((h, w, 1))], -1).astype(np.float32)
    alb = np.concatenate([rng.uniform(0.05, 0.9, (n + 2, 3))[k] * (1 + 0.2 * rng.random((h, w, 3))), np.zeros((h, w, 1))], -1).astype(np.float32)
    small = rng.random((h, w, 3)) < 0.1
    alb[..., :3] = np.where(small, rng.choice(np.array([0.0, 5e-4, 9.99e-4, 1e-3], np.float32), size=(h, w, 3)), alb[..., :3])
    acc = np.concatenate([alb[..., :3] * rng.uniform(0.2, 4.0, (h, w, 3)) + rng.uniform(0.05, 0.3, (h, w, 3)),
                          rng.choice(np.array([0.0, 1.0, 0.5], np.float32), size=(h, w, 1))], -1).astype(np.float32)
    miss = obj < 0
    nd[miss] = np.array([0, 0, 0, np.inf], np.float32)
    pos[miss] = 0
    alb[miss] = 0
    return acc, obj, nd, pos, alb


def shape_seed(w, h):
    return 1000 + 31 * w + h


UPSAMPLE_STEPS = [1, 2, 3, 8, 512, 32768]
UPSAMPLE_SIGMAS = [(32.0, 0.02), (0.0, 0.0)]


def upsample_stripes(w):
    return [0, 1, 2, 5, w, w + 3]


# ---- the upsampler's parameter extremes on exact ties ---------------------------------------------------------------------
TIE_SIGMA_NORMAL = [f32(1e-30), 128.0, F32_MAX, INF]
TIE_SIGMA_PLANE = [f32(1e-38), f32(1e-30), f32(1e30), F32_MAX, INF]
TIE_W, TIE_H, TIE_STEPS, TIE_STRIPE = 37, 21, 3, 17
# object -> (unit normal, the coordinate all its points share, d_p)
TIE_OBJECTS = [((0.0, 1.0, 0.0), 1, 2.5), ((1.0, 0.0, 0.0), 0, 0.0), ((0.0, 0.0, -1.0), 2, -2.0), ((0.0, -1.0, 0.0), 1, f32(1e-38)),
               ((-1.0, 0.0, 0.0), 0, INF)]
TIE_PERP = len(TIE_OBJECTS)  # the object whose anchors' normals are perpendicular to its other pixels'


def upsample_tie_guides(seed=7):
    """(acc, obj, nd, pos) on TIE_W x TIE_H: vertical bands of the TIE_OBJECTS — one constant unit axis normal per object, every
    point of an object with the same coordinate along that axis bit for bit, so that n_p.n_q == 1 and n_p.(x_q - x_p) == 0
    exactly and each weight is b_q in binary32 and in float64 — with d_p of 2.5, 0, -2, 1e-38 and inf, a band of misses, and one
    more object whose anchor pixels (for TIE_STEPS, TIE_STRIPE) have the normal (1, 0, 0) and whose other pixels (0, 1, 0),
    all its points sharing x and y: its weights are exactly 0."""
    from test_gpu_upsample import around

    w, h = TIE_W, TIE_H
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    obj = np.minimum(xs // 5, TIE_PERP + 1).astype(np.int32)
    obj[obj == TIE_PERP + 1] = -1
    obj[h // 2, :] = np.where(obj[h // 2, :] >= 0, (obj[h // 2, :] + 1) % TIE_PERP, -1)  # a row that shifts the bands
    free = rng.uniform(-3.0, 3.0, (h, w, 3)).astype(np.float32)
    nd = np.zeros((h, w, 4), np.float32)
    pos = np.concatenate([free, np.ones((h, w, 1), np.float32)], -1)
    for k, (nrm, axis, d) in enumerate(TIE_OBJECTS):
        on = obj == k
        nd[on] = np.array(nrm + (d,), np.float32)
        pos[..., axis][on] = np.float32(0.375 + k)
    x0, _, _ = around(w, TIE_STEPS, TIE_STRIPE)
    y0, _, _ = around(h, TIE_STEPS, 0)
    anchor = (np.arange(h) == y0)[:, None] & (np.arange(w) == x0)[None, :]
    on = obj == TIE_PERP
    nd[on & anchor] = np.array([1.0, 0.0, 0.0, 3.0], np.float32)
    nd[on & ~anchor] = np.array([0.0, 1.0, 0.0, 3.0], np.float32)
    pos[..., 0][on] = np.float32(-1.25)
    pos[..., 1][on] = np.float32(0.5)
    miss = obj < 0
    nd[miss] = np.array([0, 0, 0, np.inf], np.float32)
    pos[miss] = 0
    acc = np.concatenate([rng.uniform(0.05, 4.0, (h, w, 3)), rng.choice(np.array([0.0, 1.0, 0.5], np.float32), size=(h, w, 1))],
                         -1).astype(np.float32)
    return acc, obj, nd, pos


# ---- anti-aliasing ----------------------------------------------------------------------------------------------------------
def antialias_inputs(w, h, k):
    """(c, obj, sub, other): colours and objects of guides(), sub-sample planes drawn by test_gpu_antialias.draw_subsamples, and
    what the source that is not chosen holds."""
    from test_gpu_antialias import draw_subsamples

    c, obj, _, _, _ = guides(w, h, shape_seed(w, h))
    sub = draw_subsamples(obj, k, seed=shape_seed(w, h) + k)
    other = np.random.default_rng(5).uniform(0.05, 4.0, c.shape).astype(np.float32)
    return c, obj, sub, other


# ---- variance ---------------------------------------------------------------------------------------------------------------
def halves(w, h, seed, alb):
    """Two positive half renders around one mean with differing alphas (test_gpu_variance._halves)."""
    rng = np.random.default_rng(seed)
    mean = alb[..., :3] * rng.uniform(0.2, 4.0, (h, w, 3)) + rng.uniform(0.01, 0.2, (h, w, 3))
    a = np.concatenate([mean * rng.uniform(0.5, 1.5, (h, w, 3)), rng.choice([0.0, 1.0, 7.5], size=(h, w, 1))], -1).astype(np.float32)
    b = np.concatenate([mean * rng.uniform(0.5, 1.5, (h, w, 3)), rng.choice([0.0, 2.0], size=(h, w, 1))], -1).astype(np.float32)
    return a, b


def variance_field(w, h, seed):
    return np.random.default_rng(seed).uniform(0.02, 0.5, (h, w)).astype(np.float32)


FILTER_LEVELS = [1, 2, 8]
FILTER_SIGMAS = [0.0, 4.0, INF]

# ---- the apron at the seams -------------------------------------------------------------------------------------------------
SEAM_SHAPES = [(48, 40), (33, 18), (17, 15)]
SEAM_MAPS = ["vertical", "horizontal", "checker1", "checker8", "seam misses"]
_SEAMS = np.array([0, 8, 16, 17, 24, 32, 40])  # borders at 7|8, 15|16, 16|17 and on the later tile seams


def seam_objects(w, h, kind):
    ys, xs = np.mgrid[0:h, 0:w]
    band_x, band_y = np.searchsorted(_SEAMS, xs, side="right") - 1, np.searchsorted(_SEAMS, ys, side="right") - 1
    if kind == "vertical":
        obj = band_x
    elif kind == "horizontal":
        obj = band_y
    elif kind == "checker1":
        obj = (xs + ys) % 2
    elif kind == "checker8":
        obj = (xs // 8 + ys // 8) % 2
    else:  # misses on both sides of every tile seam, one object per cell between them
        obj = band_x + 8 * band_y
        on_seam = np.isin(xs, [7, 8, 15, 16, 17, 23, 24, 31, 32]) | np.isin(ys, [7, 8, 15, 16, 17, 23, 24, 31, 32])
        obj = np.where(on_seam & ((xs + ys) % 3 != 0), -1, obj)
    return obj.astype(np.int32)


def seam_inputs(w, h, kind, seed=3):
    """(acc, var, obj, nd, pos, alb): smooth normals and points that do not depend on the object map, noisy colours, and a
    variance that is a per-pixel random field over six decades (1e-5 .. 10)."""
    rng = np.random.default_rng(seed + w)
    obj = seam_objects(w, h, kind)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    nrm = np.stack([0.3 * np.sin(xs / 7.0), 0.3 * np.cos(ys / 5.0), np.ones((h, w))], -1) + 0.02 * rng.normal(size=(h, w, 3))
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    depth = 3.0 + 0.01 * xs
    pnt = np.stack([xs * 0.01, ys * 0.01, depth], -1) + 0.002 * rng.normal(size=(h, w, 3))
    nd = np.concatenate([nrm, depth[..., None]], -1).astype(np.float32)
    pos = np.concatenate([pnt, np.ones((h, w, 1))], -1).astype(np.float32)
    alb = np.concatenate([rng.uniform(0.1, 0.9, (h, w, 3)), np.zeros((h, w, 1))], -1).astype(np.float32)
    acc = np.concatenate([rng.uniform(0.1, 3.0, (h, w, 3)), rng.choice(np.array([0.0, 1.0], np.float32), size=(h, w, 1))], -1).astype(np.float32)
    var = (10.0 ** rng.uniform(-5.0, 1.0, (h, w))).astype(np.float32)
    miss = obj < 0
    nd[miss] = np.array([0, 0, 0, np.inf], np.float32)
    pos[miss] = 0
    alb[miss] = 0
    return acc, var, obj, nd, pos, alb


# ---- variance and sigma_luminance extremes ----------------------------------------------------------------------------------
EXT_W, EXT_H = 37, 21
EXT_VARIANCES = [0.0, f32(1e-45), f32(1e-38), 1.0, f32(1e30), F32_MAX, INF]
EXT_SIGMAS = [f32(1e-45), f32(1e-30), 1.0, F32_MAX, INF]
EXT_LEVELS = [1, 3]


def extreme_inputs():
    """(acc, obj, nd, pos, alb) on EXT_W x EXT_H: four vertical objects and a column of misses; the colour is piecewise constant
    (cells of 3 x 2 pixels from a palette whose luminances differ by at least 0.05), so that exact luminance ties lie next
    to distinct values inside every object."""
    w, h = EXT_W, EXT_H
    ys, xs = np.mgrid[0:h, 0:w]
    obj = (xs // 10).astype(np.int32)
    obj[:, 18] = -1
    obj[4, 5] = -1
    palette = np.array([[0.25, 0.5, 0.125], [1.0, 0.75, 2.0], [0.5, 1.5, 0.25], [2.0, 2.5, 1.0], [0.125, 0.25, 5.0]], np.float32)
    acc = np.concatenate([palette[(xs // 3 + 2 * (ys // 2)) % 5], np.where((xs + ys) % 2, 1.0, 0.5)[..., None]], -1).astype(np.float32)
    nd = np.broadcast_to(np.array([0, 0, -1, 3], np.float32), (h, w, 4)).copy()
    pos = np.stack([xs * 0.01, ys * 0.01, np.full((h, w), 3.0), np.ones((h, w))], -1).astype(np.float32)
    alb = np.broadcast_to(np.array([0.5, 0.5, 0.5, 0], np.float32), (h, w, 4)).copy()
    miss = obj < 0
    nd[miss] = np.array([0, 0, 0, np.inf], np.float32)
    pos[miss] = 0
    alb[miss] = 0
    return acc, obj, nd, pos, alb


def extreme_variances():
    """(name, (H, W) float32): every value of EXT_VARIANCES as a uniform buffer, and two per-object assignments."""
    _, obj, _, _, _ = extreme_inputs()
    out = [("uniform %g" % v, np.full((EXT_H, EXT_W), v, np.float32)) for v in EXT_VARIANCES]
    vals = np.array(EXT_VARIANCES, np.float32)
    out.append(("per object a", vals[np.maximum(obj, 0)]))
    out.append(("per object b", vals[3 + np.maximum(obj, 0)]))
    return out


def variance_opens(v, sigma):
    """Whether the kernel's reciprocal scale 1 / (sigma sqrt(v) + 1e-10), sigma above FLT_MAX counting as FLT_MAX, evaluated in
    binary32, is below 1e-30 (0, or a subnormal: the weight of every finite difference is then 1)."""
    with np.errstate(all="ignore"):
        s = np.float32(1) / (np.float32(min(sigma, F32_MAX)) * np.sqrt(np.float32(v)) + np.float32(1e-10))
    return float(s) < 1e-30


# ---- moving objects ---------------------------------------------------------------------------------------------------------
MOTION_PARAMS = [(1, 32.0, 0.02, 0.9), (2, 7.0, 0.05, -1.0)]
# (moves of the three spheres since the previous frame, camera): a start, a sideways move, a move in depth.  The camera moves a
# little in every frame: a still one reprojects the frame's border pixels exactly onto the window's edge, where the float64
# definition cannot say which taps binary32 takes (a fifth of a one-row frame)
MOTION_FRAMES = [
    ([], ((0.0, 0.0, 0.0), 0.0, 55)),
    ([[(0.15, 0.0, 0.0), (-0.1, 0.0, 0.0), (0.0, 0.08, 0.0)]], ((0.013, 0.004, 0.05), 0.7, 55)),
    ([[(0.0, 0.0, 0.3), (0.05, 0.0, -0.25), (0.0, 0.05, 0.2)]], ((0.04, 0.01, 0.12), 2.5, 55)),
]


# The frames of the 37 x 21 cases.  The camera steps sideways by 0.111 and up by 0.1 per frame and does not turn: a point at
# depth Z then lands t H / (2 Z tan(fov / 2)) = 20.2 t / Z pixels from its pixel, 0.35 to 0.7 of a pixel sideways and about as
# much upwards at the spheres' depths of 3.2 to 6.4.  A sphere of three pixels' radius turns its normal by about 19 degrees per
# pixel, so no tap of a sphere pixel has n_p.n'_q within 1e-3 of 1, the band in which the definition cannot decide a
# normal_threshold of 1 (tests/test_pass_references.py counts what is left out).
EDGE_W, EDGE_H = 37, 21
EDGE_FRAMES = [
    ([], ((0.0, 0.0, 0.0), 0.0, 55)),
    ([[(0.15, 0.0, 0.0), (-0.1, 0.0, 0.0), (0.0, 0.08, 0.0)]], ((0.111, 0.1, 0.0), 0.0, 55)),
    ([[(0.0, 0.0, 0.3), (0.05, 0.0, -0.25), (0.0, 0.05, 0.2)]], ((0.222, 0.2, 0.0), 0.0, 55)),
]
TEMPORAL_EXTREMES = [(1, INF, 0.02, 0.9), (3, INF, 0.05, -1.0), (1, 32.0, 0.02, -1.0), (1, 32.0, 0.02, 1.0), (1, 32.0, f32(1e-38), 0.9),
                     (1, 32.0, F32_MAX, 0.9)]
EDGE_PARAMS = (1, 32.0, 0.02, 0.9)
DISPLACEMENTS = [0.0, f32(1e-30), f32(1e30), INF]


def motion_sequence(srt, w, h, seed, frames=None):
    """Per frame of MOTION_FRAMES (or `frames`): (updates: the sphere lists to pass to srt_update_scene in turn, spheres, camera,
    guides (obj, nd, pos), acc)."""
    rng = np.random.default_rng(seed)
    spheres = mo.BASE
    out = []
    for updates, (p, yaw, fov) in (MOTION_FRAMES if frames is None else frames):
        lists = []
        for steps in updates:
            spheres = mo._moved(spheres, steps)
            lists.append(spheres)
        cam = tp.camera(srt, p, yaw, fov)
        g = mo._cast(cam, w, h, spheres)
        acc = np.concatenate([rng.uniform(0.02, 3.0, (h, w, 3)), rng.choice([0.0, 1.0], (h, w, 1))], -1).astype(np.float32)
        out.append((lists, spheres, cam, g, acc))
    return out


def sphere_table(prev, now):
    """(delta, keep) of the contract for the dummy list of test_gpu_motion._objects: the ground (never moved) and the spheres."""
    delta = np.zeros((1 + len(now), 3), np.float32)
    for k, ((c0, _), (c1, _)) in enumerate(zip(prev, now)):
        delta[k + 1] = np.array(c1, np.float32) - np.array(c0, np.float32)
    return delta, np.ones(1 + len(now), bool)


def relabel_beyond(obj, pos, count):
    """The OBJECT guide with the ground's pixels relabelled, by where their point lies in the world (so that a ground point keeps
    its label from frame to frame), to the indices count, count + 5 and 2^30, none of which the motion table has."""
    out = obj.copy()
    cell = np.floor(pos[..., 0].astype(np.float64) * 1.5).astype(np.int64) % 4
    for r, idx in ((1, count), (2, count + 5), (3, 2 ** 30)):
        out[(obj == 0) & (cell == r)] = idx
    return out


def displacement_frames(srt, step, seed=4):
    """Two frames of EDGE_FRAMES' first two cameras over spheres that stay where they are in the guides, while the LIST position
    of the first sphere (object 1, whose y is 0) changes by `step` (-0 for +0 when step is 0): (cameras, guides per frame, accs,
    the moved list)."""
    rng = np.random.default_rng(seed)
    w, h = EDGE_W, EDGE_H
    cams = [tp.camera(srt, p, yaw, fov) for _, (p, yaw, fov) in EDGE_FRAMES[:2]]
    guides = [mo._cast(cam, w, h, mo.BASE) for cam in cams]
    accs = [np.concatenate([rng.uniform(0.02, 3.0, (h, w, 3)), rng.choice([0.0, 1.0], (h, w, 1))], -1).astype(np.float32) for _ in cams]
    moved = [(list(c), r) for c, r in mo.BASE]
    assert moved[0][0][1] == 0.0
    moved[0][0][1] = -0.0 if step == 0.0 else step
    return cams, guides, accs, moved
