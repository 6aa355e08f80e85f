"""The float64 definition of srt_temporal_accumulate with the mirror history on (srt_mirror_history), restated from the
"mirror history" block of include/srt_pathtrace.h on top of tests/moments_reference.py's ray_basis and taps, and a generator of
synthetic guides for a flat mirror.  Used by tests/test_mirror_history_reference.py (properties of the definition alone) and
tests/test_gpu_mirror_history.py (against the kernels)."""
import ctypes as C
import json
import math

import numpy as np

import moments_reference as mr

TAG_SHIFT = 32768
MIRROR, PATCH, WALL0 = 7, 5, 1  # object indices of the generator: the mirror, the non-mirror patch on it, the wall's first stripe


# camera positions of tests/test_gpu_moments.py's SYNTH_MOVES: translations in the mirror plane's directions.  At the image's depth
# of 13 a step of 0.34 (0.16) is 0.53 (0.25) pixels of 37 x 21, on the plane itself 1.37 (0.65): no footprint lies near a pixel boundary
SYNTH_MOVES = [(0.0, 0.0), (0.34, 0.16), (0.68, 0.32), (0.34, 0.48), (0.0, 0.64)]


def camera(srt, pos, yaw_deg=0.0, basis=None):
    """A camera at pos, turned by yaw_deg about world up (or with the rows right, up, forward of `basis`), fov 55."""
    if basis is None:
        a = math.radians(yaw_deg)
        basis = [(math.cos(a), 0.0, -math.sin(a)), (0.0, 1.0, 0.0), (math.sin(a), 0.0, math.cos(a))]
    c = srt.Camera()
    c.position = (C.c_float * 3)(*[float(v) for v in pos])
    c.right = (C.c_float * 3)(*[float(v) for v in basis[0]])
    c.up = (C.c_float * 3)(*[float(v) for v in basis[1]])
    c.forward = (C.c_float * 3)(*[float(v) for v in basis[2]])
    c.fov_degrees = 55
    return c


def mirror_box_scene(path):
    """The mirror-box scene as a file of the scene format: the camera looks at a large mirror box; a red and a green diffuse
    sphere stand behind the camera, side by side, so that they are seen in the mirror only.  Objects: 0 the mirror, 1 red, 2 green."""
    def obj(pos, rend, color, smooth, spec):
        return {"Name": "", "Position": list(pos), "Renderer": rend,
                "Material": {"Color": list(color), "Emissive": [0.0, 0.0, 0.0], "Metalness": 0.0, "Smoothness": smooth, "SpecularAmount": spec,
                             "SpecularColor": [1.0, 1.0, 1.0]}}
    objs = [obj((0.0, 0.0, 4.0), {"Type": "Cube", "Size": [8.0, 6.0, 1.0]}, (0.9, 0.9, 0.9), 1.0, 1.0),
            obj((-1.6, 0.0, -2.0), {"Type": "Sphere", "Radius": 1.5}, (0.9, 0.1, 0.1), 0.5, 0.0),
            obj((1.6, 0.0, -2.0), {"Type": "Sphere", "Radius": 1.5}, (0.1, 0.9, 0.1), 0.5, 0.0)]
    with open(path, "w") as f:
        json.dump({"SceneName": "", "SceneObjects": objs}, f)
    return str(path)


def tag(bounces, first_object):
    """M1: 0 for J = 0, else J * 32768 + m."""
    bounces, first_object = np.asarray(bounces, np.int64), np.asarray(first_object, np.int64)
    return np.where(bounces >= 1, bounces * TAG_SHIFT + first_object, 0)


def untag(t):
    """(J, m) of a non-zero tag."""
    t = np.asarray(t, np.int64)
    return t // TAG_SHIFT, t % TAG_SHIFT


def rho(radius_pixels, fov_degrees, height):
    """(float)((double)radius_pixels * 2 * tan(fov_degrees * pi / 360) / H), as float64."""
    with np.errstate(all="ignore"):
        return float(np.float32(float(np.float32(radius_pixels)) * 2.0 * math.tan(float(np.float32(fov_degrees)) * math.pi / 360.0) / height))


def project(y, cam, w, h, exact=False):
    """Step 2 for the points y (..., 3) and the camera `cam` of the stored history: (u, v, ok, edge).  ok: g > 0 and (u, v) in
    the window (-1, W) x (-1, H); edge: the relative distance of g from 0.  exact: the float64 inverse of the basis instead of
    the float32 one the host passes to the kernel."""
    Bi = np.linalg.inv(mr.ray_basis(cam, w, h))
    if not exact:
        Bi = Bi.astype(np.float32).astype(np.float64)
    rel = np.asarray(y, np.float64) - np.array(cam.position[:], np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        abg = rel @ Bi.T
        a, b, g = abg[..., 0], abg[..., 1], abg[..., 2]
        u = (a / g + 1) * w / 2
        v = (b / g + 1) * h / 2
        ok = (g > 0) & (u > -1) & (u < w) & (v > -1) & (v < h)
        edge = np.abs(g) / np.maximum(np.linalg.norm(rel, axis=-1), 1e-30)
    return u, v, ok, np.where(np.isfinite(edge), edge, np.inf)


def _ball_taps(y, want, g, prev, r, thr):
    """M4 for one candidate y (H, W, 3) over the pixels `want`: the four taps as (weight, row, column) with weight 0 where the
    tap does not count, (u, v, ok) of the projection, and the smallest relative distance of any decision from its threshold."""
    H, W = want.shape
    u, v, ok, edge = project(y, prev["cam"], W, H)
    ok = ok & want
    edge = np.where(want, edge, np.inf)
    uu, vv = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
    x0, y0 = np.floor(uu).astype(np.int64), np.floor(vv).astype(np.int64)
    fx, fy = uu - x0, vv - y0
    edge = np.minimum(edge, np.where(ok, np.minimum(np.minimum(fx, 1 - fx), np.minimum(fy, 1 - fy)), np.inf))
    x_p, n_p = g["r_pos"][..., :3].astype(np.float64), g["r_nd"][..., :3].astype(np.float64)
    tg = tag(g["bounces"], g["obj"])
    out = []
    for k in range(4):
        qx, qy = x0 + (k & 1), y0 + (k >> 1)
        wq = np.where(k & 1, fx, 1 - fx) * np.where(k >> 1, fy, 1 - fy)
        inside = ok & (wq > 0) & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
        cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
        same = inside & (prev["obj"][cy, cx] == g["r_obj"]) & (prev["tag"][cy, cx] == tg)
        with np.errstate(all="ignore"):
            d = prev["pos"][cy, cx, :3].astype(np.float64) - x_p
            dist2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            counted = same & (dist2 <= r * r)  # (a NaN fails)
            finite = same & np.isfinite(r) & (r > 0)
            edge = np.minimum(edge, np.where(finite, np.abs(np.sqrt(dist2) - r) / np.where(finite, r, 1.0), np.inf))
            if thr > -1:
                dot = np.sum(n_p * prev["nrm"][cy, cx, :3].astype(np.float64), axis=2)
                edge = np.minimum(edge, np.where(counted, np.abs(dot - thr) / max(abs(thr), 1e-3), np.inf))
                counted = counted & (dot >= thr)
        out.append((np.where(counted, wq, 0.0), cy, cx))
    return out, u, v, ok, np.where(np.isnan(edge), 0.0, edge)


def accumulate(acc, g, prev, n, max_samples, sigma_t, thr, radius_pixels=2.0, displaced=False):
    """One srt_temporal_accumulate call with the mode on.
    acc: the accumulator (H, W, >= 3).  g: the current guides — cam, obj / nd / pos (first hits), r_obj / r_nd / r_pos / bounces
    (reflection outputs).  prev: the stored history of the previous call — cam, color (H, W, 4: rgb, L), obj, pos, nrm, tag — or
    None when there is none.  displaced: the call uses a displacement table (M5: mirror pixels have no history; the pixels with
    J = 0 are NOT modelled then, the caller compares them with the mode off).
    Returns a dict: out (H, W, 3), L, motion (H, W, 3: u - x, v - y, W), taps (the counted taps as moments_reference.blend takes
    them, None without a history), candidate (0: none, 1, 2; mirror pixels), edge, store (the history this call stores)."""
    H, W = g["obj"].shape
    c = np.asarray(acc, np.float64)[..., :3]
    obj, J = g["obj"], g["bounces"]
    hit = obj >= 0
    mirror = hit & (J >= 1)
    plain = hit & ~mirror
    tg = tag(np.where(mirror, J, 0), np.where(mirror, obj, 0))
    ys, xs = np.mgrid[0:H, 0:W]
    motion = np.zeros((H, W, 3))
    cand = np.zeros((H, W), np.int64)
    edge = np.full((H, W), np.inf)
    tl = None
    if prev is not None:
        # M2: today's rule from the G-buffer slots, and tag' == 0
        like = dict(cam=prev["cam"], obj=prev["obj"], nd=prev["nrm"], pos=prev["pos"])
        t0, e0 = mr.taps(obj, g["nd"], g["pos"], like, sigma_t, thr)
        t0 = [(np.where(plain & (prev["tag"][cy, cx] == 0), w, 0.0), cy, cx) for w, cy, cx in t0]
        u0, v0, ok0, _ = project(g["pos"][..., :3], prev["cam"], W, H)
        edge = np.where(plain, e0, edge)
        sel = plain & ok0
        motion[..., 0], motion[..., 1] = np.where(sel, u0 - xs, 0.0), np.where(sel, v0 - ys, 0.0)
        tl = t0
        # M4
        want = mirror & (g["r_obj"] >= 0) & (not displaced)
        if want.any():
            C = np.array(g["cam"].position[:], np.float32).astype(np.float64)
            x0p = g["pos"][..., :3].astype(np.float64)
            with np.errstate(all="ignore"):
                D, t0p = g["r_nd"][..., 3].astype(np.float64), g["nd"][..., 3].astype(np.float64)
                r = rho(radius_pixels, g["cam"].fov_degrees, H) * D
                y1 = C + (x0p - C) * (D / t0p)[..., None]
            t1, u1, v1, ok1, e1 = _ball_taps(y1, want, g, prev, r, thr)
            w1 = sum(t[0] for t in t1) > 0
            t2, u2, v2, ok2, e2 = _ball_taps(x0p, want & ~w1, g, prev, r, thr)
            w2 = sum(t[0] for t in t2) > 0
            cand = np.where(w1, 1, np.where(w2, 2, 0))
            edge = np.where(want, np.where(w1, e1, np.minimum(e1, e2)), edge)
            tl = [(np.where(w1, a[0], np.where(w2, b[0], k[0])), np.where(w1, a[1], np.where(w2, b[1], k[1])),
                   np.where(w1, a[2], np.where(w2, b[2], k[2]))) for a, b, k in zip(t1, t2, t0)]
            mu = np.where(w2, u2 - xs, np.where(ok1, u1 - xs, 0.0))
            mv = np.where(w2, v2 - ys, np.where(ok1, v1 - ys, 0.0))
            motion[..., 0], motion[..., 1] = np.where(want, mu, motion[..., 0]), np.where(want, mv, motion[..., 1])
    out = c.copy()
    L = np.where(hit, float(n), 0.0)
    if tl is not None:
        col = prev["color"].astype(np.float64)
        sw = np.zeros((H, W))
        s = np.zeros((H, W, 4))
        for w, cy, cx in tl:
            sw += w
            s += w[..., None] * np.where((w > 0)[..., None], col[cy, cx], 0.0)
        with np.errstate(all="ignore"):
            Lb = np.minimum(s[..., 3] / sw + n, max_samples)
            a = n / Lb
            blended = (1 - a)[..., None] * (s[..., :3] / sw[..., None]) + a[..., None] * c
        use = sw > 0
        out = np.where(use[..., None], blended, c)
        L = np.where(use, Lb, L)
        motion[..., 2] = sw
    store = dict(cam=g["cam"], color=np.concatenate([np.where(hit[..., None], out, 0.0), L[..., None]], -1),
                 obj=np.where(mirror, g["r_obj"], obj).astype(np.int32), pos=np.where(mirror[..., None], g["r_pos"], g["pos"]).astype(np.float32),
                 nrm=np.where(mirror[..., None], g["r_nd"][..., :3], g["nd"][..., :3]).astype(np.float32), tag=tg)
    for k in ("pos", "nrm"):
        store[k] = np.where(hit[..., None], store[k], 0).astype(np.float32)
    return dict(out=out, L=L, motion=motion, taps=tl, candidate=cand, edge=edge, store=store)


def store_of(g, color):
    """The history a call stores for the guides g, with the colour rows `color` (H, W, 4: result rgb, L) as read back."""
    z = np.zeros(g["obj"].shape + (3,))
    return dict(accumulate(z, g, None, 1, 1.0, 1.0, -1.0)["store"], color=np.asarray(color, np.float64))


# ---- synthetic guides: a flat mirror ------------------------------------------------------------------------------------------------
def flat_mirror_guides(cam, w, h, xs=None, ys=None, dtype=np.float32, features=True):
    """The G-buffer and reflection arrays of cam's primary rays, in float64, rounded to `dtype`: the mirror plane z = 5 faces a
    camera near the origin (object MIRROR, normal (0, 0, -1)); its reflections end on the wall z = -3 (normal (0, 0, 1)), which
    carries world-anchored stripes of three objects WALL0 .. WALL0 + 2 and bands where the chain leaves the scene; a
    world-anchored patch of the plane is a non-mirror object (PATCH, J = 0) and bands of it are first-hit misses.  Any translated
    or rotated camera sees the same world.  xs, ys: pixel coordinates (default: the frame's pixel grid).  features=False: the whole
    plane is the mirror and the whole wall one object (WALL0); the caller paints its own."""
    if xs is None:
        ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    B = mr.ray_basis(cam, w, h)
    d = (xs / w * 2 - 1)[..., None] * B[:, 0] + (ys / h * 2 - 1)[..., None] * B[:, 1] + B[:, 2]
    o = np.array(cam.position[:], np.float32).astype(np.float64)
    dl = np.linalg.norm(d, axis=-1)
    with np.errstate(all="ignore"):
        t = (5.0 - o[2]) / d[..., 2]
    p = o + t[..., None] * d
    p[..., 2] = 5.0
    miss = ~(d[..., 2] > 0) | (np.floor(p[..., 1] / 0.9 + 0.25).astype(np.int64) % 5 == 0)
    if not features:
        miss = ~(d[..., 2] > 0)
    patch = ~miss & (p[..., 0] > -1.9) & (p[..., 0] < -0.7) & features
    mirror = ~miss & ~patch
    t0 = t * dl
    # the reflected ray: (dx, dy, -dz) from p down to z = -3
    t1 = 8.0 / d[..., 2] * dl
    q = p + (8.0 / d[..., 2])[..., None] * (d * np.array([1.0, 1.0, -1.0]))
    q[..., 2] = -3.0
    sky = mirror & (np.floor(q[..., 1] / 2.6 + 0.4).astype(np.int64) % 4 == 0) & features
    wall = (WALL0 + (np.floor(q[..., 0] / 2.3).astype(np.int64) % 3 if features else 0) + np.zeros(miss.shape, np.int64)).astype(np.int32)
    shape = miss.shape
    obj = np.where(miss, -1, np.where(patch, PATCH, MIRROR)).astype(np.int32)
    nd = np.zeros(shape + (4,))
    nd[..., 2] = np.where(miss, 0.0, -1.0)
    nd[..., 3] = np.where(miss, np.inf, t0)
    pos = np.zeros(shape + (4,))
    pos[..., :3] = np.where(miss[..., None], 0.0, p)
    pos[..., 3] = np.where(miss, 0.0, 1.0)
    ended = mirror & ~sky
    r_obj = np.where(mirror, np.where(sky, -1, wall), obj).astype(np.int32)
    r_nd = nd.copy()
    r_nd[..., 2] = np.where(ended, 1.0, np.where(sky, 0.0, nd[..., 2]))
    r_nd[..., 3] = np.where(ended, t0 + t1, np.where(sky, np.inf, nd[..., 3]))
    r_pos = pos.copy()
    r_pos[..., :3] = np.where(ended[..., None], q, np.where(sky[..., None], 0.0, pos[..., :3]))
    r_pos[..., 3] = np.where(sky, 0.0, pos[..., 3])
    return dict(cam=cam, obj=obj, nd=nd.astype(dtype), pos=pos.astype(dtype), r_obj=r_obj, r_nd=r_nd.astype(dtype), r_pos=r_pos.astype(dtype),
                bounces=mirror.astype(np.int32))


def without_mirrors(g):
    """The same first hits with every J = 0: the reflection outputs equal the G-buffer's (the identity of the reflection pass)."""
    return dict(g, r_obj=g["obj"].copy(), r_nd=g["nd"].copy(), r_pos=g["pos"].copy(), bounces=np.zeros_like(g["bounces"]))
