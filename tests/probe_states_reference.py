"""Probe classification and relocation and the probe-grid shading that obeys the records, as the header defines them
(include/srt_pathtrace.h: rules S1-S7 of the classification block and rules 3s / 4s of the states-shading block), in numpy float32
with one rounding per operation, on top of tests/probe_grid_reference.py and tests/probe_depth_reference.py.  The reference never
culls: every candidate is measured against every primitive.  scene_distance64() and inside64() are the float64 yardsticks of the
CPU tests.  Not a test: tests/test_probe_states_reference.py, tests/test_probe_states_abi.py and the GPU tests import it."""
import numpy as np

import light_probe_reference as LP
import probe_depth_reference as PD
import probe_grid_reference as PG

F = np.float32
RECORDS, POSITIONS = 1, 2
RELOCATE, NORMALIZE, COUNT_WORK = 1, 2, 4
CLEAR, MOVED, BURIED, INSIDE, IDLE = 0, 1, 2, 4, 8
SPHERE, BOX, MESH = 1, 2, 3
DEFAULTS = dict(clearance=F(0.2), max_offset=F(0.45), steps=8)


def primitives(objs):
    """(spheres (Ns, 4) float32 = centre, |radius|; boxes (Nb, 2, 3) float32 = centre, half size; has_mesh) of a list of object
    dicts (type, position, radius, half_size) — the primitive table of the pass."""
    sph = [list(o["position"]) + [abs(F(o.get("radius", 0.0)))] for o in objs if o["type"] == SPHERE]
    box = [[list(o["position"]), list(o.get("half_size", (0.0, 0.0, 0.0)))] for o in objs if o["type"] == BOX]
    return (np.asarray(sph, dtype=F).reshape(-1, 4), np.asarray(box, dtype=F).reshape(-1, 2, 3), any(o["type"] == MESH for o in objs))


def scene_distance(prims, x):
    """Rule S1 on points x (..., 3) float32: S (...) float32."""
    sph, box, _ = prims
    x = np.asarray(x, dtype=F)
    S = np.full(x.shape[:-1], np.inf, dtype=F)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for s in sph:
            e = (x - s[:3]).astype(F)
            q = ((e[..., 0] * e[..., 0]).astype(F) + (e[..., 1] * e[..., 1]).astype(F)).astype(F)
            q = (q + (e[..., 2] * e[..., 2]).astype(F)).astype(F)
            sd = (np.sqrt(q).astype(F) - s[3]).astype(F)
            S = np.where(sd < S, sd, S)
        for c, h in box:
            q = (np.abs((x - c).astype(F)).astype(F) - h).astype(F)
            m = np.where(q > 0, q, F(0)).astype(F)
            o = ((m[..., 0] * m[..., 0]).astype(F) + (m[..., 1] * m[..., 1]).astype(F)).astype(F)
            o = np.sqrt((o + (m[..., 2] * m[..., 2]).astype(F)).astype(F)).astype(F)
            qxy = np.where(q[..., 0] > q[..., 1], q[..., 0], q[..., 1])
            qm = np.where(qxy > q[..., 2], qxy, q[..., 2])
            sd = (o + np.where(qm < 0, qm, F(0)).astype(F)).astype(F)
            S = np.where(sd < S, sd, S)
    return S.astype(F)


def scene_distance64(prims, x):
    """The same distance in float64 on the same float32 inputs."""
    sph, box, _ = prims
    x = np.asarray(x, dtype=np.float64)
    S = np.full(x.shape[:-1], np.inf)
    for s in sph.astype(np.float64):
        S = np.minimum(S, np.sqrt(((x - s[:3]) ** 2).sum(axis=-1)) - s[3])
    for c, h in box.astype(np.float64):
        q = np.abs(x - c) - h
        S = np.minimum(S, np.sqrt((np.maximum(q, 0.0) ** 2).sum(axis=-1)) + np.minimum(q.max(axis=-1), 0.0))
    return S


def inside64(prims, x):
    """The containment test of tools/probe_depth_leak.py in float64: strictly inside a box with a positive half size or a sphere."""
    sph, box, _ = prims
    x = np.asarray(x, dtype=np.float64)
    inside = np.zeros(x.shape[:-1], bool)
    for s in sph.astype(np.float64):
        if s[3] > 0:
            inside |= ((x - s[:3]) ** 2).sum(axis=-1) < s[3] * s[3]
    for c, h in box.astype(np.float64):
        if (h > 0).any():
            inside |= (np.abs(x - c) < h).all(axis=-1)
    return inside


def scales(grid, clearance, max_offset, steps):
    """Rule S2: (margin, reach, dt) float32."""
    s = grid.spacing
    smin = min(s[0], s[1], s[2])
    margin = F(F(clearance) * smin)
    reach = F(np.sqrt(F(F(F(s[0] * s[0]) + F(s[1] * s[1])) + F(s[2] * s[2]))))
    return margin, reach, F(F(max_offset) / F(steps))


def directions_as_used(directions, flags):
    d = np.asarray(directions, dtype=F).reshape(-1, 4)
    if flags & NORMALIZE:
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            x, y, z = d[:, 0], d[:, 1], d[:, 2]
            n = np.sqrt((((x * x).astype(F) + (y * y).astype(F)).astype(F) + (z * z).astype(F)).astype(F)).astype(F)
            return (d[:, :3] / n[:, None]).astype(F)
    return d[:, :3].copy()


def candidates(grid, g, d, t):
    """Rule S4's candidates of probes g (N, 3) for directions d (K, 3) at offset length t: (o (N, K, 3), x (N, K, 3))."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        o = ((d * F(t)).astype(F) * grid.spacing[None, :]).astype(F)  # (K, 3): the same for every probe
        x = (g[:, None, :] + o[None, :, :]).astype(F)
    return np.broadcast_to(o[None], x.shape), x


def classify(grid, objs, directions=None, flags=0, clearance=DEFAULTS["clearance"], max_offset=DEFAULTS["max_offset"], steps=DEFAULTS["steps"]):
    """srt_classify_probes: a dict of records (P, 4) float32 with the state bits in w, positions (P, 4), state (P,) uint32, s0 (P,),
    step (P,) the winning m of a MOVED probe (0 otherwise), and work, the counts of rule S7 without the waves."""
    prims = primitives(objs)
    g = PG.positions(grid)[:, :3]
    P = g.shape[0]
    margin, reach, dt = scales(grid, clearance, max_offset, steps)
    s0 = scene_distance(prims, g)
    inside = s0 < 0
    state = np.where(inside, BURIED | INSIDE, CLEAR).astype(np.uint32)
    off = np.zeros((P, 3), dtype=F)
    step = np.zeros(P, dtype=np.int64)
    cand = 0
    if flags & RELOCATE:
        d = directions_as_used(directions, flags)
        K = d.shape[0]
        todo = np.flatnonzero(s0 < margin)
        for m in range(1, int(steps) + 1):
            if len(todo) == 0:
                break
            t = F(F(m) * dt)
            o, x = candidates(grid, g[todo], d, t)
            S = scene_distance(prims, x)  # (N, K)
            cand += len(todo) * K
            with np.errstate(invalid="ignore"):
                ok = S >= margin
            key = np.where(ok, S, F(-np.inf))
            best = key.argmax(axis=1)  # (the first of equal values: the lowest k)
            found = ok.any(axis=1)
            w = todo[found]
            off[w] = o[found, best[found]]
            state[w] = MOVED | np.where(inside[w], INSIDE, 0).astype(np.uint32)
            step[w] = m
            todo = todo[~found]
    if not prims[2]:
        idle = (state == CLEAR) & (s0 > F(F(1.0625) * reach))
        state = np.where(idle, IDLE, state).astype(np.uint32)
    records = np.zeros((P, 4), dtype=F)
    records[:, :3] = off
    records[:, 3] = state.view(F)
    positions = np.zeros((P, 4), dtype=F)
    positions[:, :3] = (g + off).astype(F)
    work = dict(probes=P, inside=int(((state & INSIDE) != 0).sum()), moved=int(((state & MOVED) != 0).sum()), buried=int(((state & BURIED) != 0).sum()),
                idle=int(((state & IDLE) != 0).sum()), candidates=cand)
    return dict(records=records, positions=positions, state=state, s0=s0, step=step, work=work, margin=margin, reach=reach, dt=dt)


def state_bits(records):
    return np.ascontiguousarray(np.asarray(records, dtype=F).reshape(-1, 4)[:, 3]).view(np.uint32)


def corners(grid, records, x, n, flags=0):
    """PG.corners with rules 3s and 4s: the same dict, plus buried (N, 8): corners with weight > 0 that rule 3s skipped."""
    x = np.asarray(x, dtype=F).reshape(-1, 3)
    n = np.asarray(n, dtype=F).reshape(-1, 3)
    rec = np.asarray(records, dtype=F).reshape(-1, 4)
    bits = state_bits(rec)
    i, f = PG.cells(grid, x)
    N = x.shape[0]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        w = np.empty((N, 8, 3), dtype=F)
        for a in range(3):
            one_minus = (F(1.0) - f[:, a]).astype(F)
            w[:, :, a] = np.where(PG.CORNER_BITS[None, :, a] == 1, f[:, None, a], one_minus[:, None])
        t = ((w[:, :, 0] * w[:, :, 1]).astype(F) * w[:, :, 2]).astype(F)
        live = t > 0
        weighted = live.copy()
        idx = i[:, None, :] + PG.CORNER_BITS[None, :, :]
        nx, ny, nz = grid.counts
        k = [np.clip(idx[:, :, a], 0, grid.counts[a] - 1) for a in range(3)]
        probe = k[0] + nx * (k[1] + ny * k[2])
        buried = live & ((bits[probe] & BURIED) != 0)
        live = live & ~buried
        p = np.empty((N, 8, 3), dtype=F)
        for a in range(3):
            p[:, :, a] = ((grid.origin[a] + (idx[:, :, a].astype(F) * grid.spacing[a]).astype(F)).astype(F) + rec[probe, a]).astype(F)
        O = (x + (n * F(.00001)).astype(F)).astype(F)
        v = (p - O[:, None, :]).astype(F)
        q = ((v[..., 0] * v[..., 0]).astype(F) + (v[..., 1] * v[..., 1]).astype(F)).astype(F)
        q = (q + (v[..., 2] * v[..., 2]).astype(F)).astype(F)
        L = np.sqrt(q).astype(F)
        live = live & (L > 0)
        d = (v / L[..., None]).astype(F)
        if flags & PG.NORMAL_WEIGHT:
            dn = ((d[..., 0] * n[:, None, 0]).astype(F) + (d[..., 1] * n[:, None, 1]).astype(F)).astype(F)
            dn = (dn + (d[..., 2] * n[:, None, 2]).astype(F)).astype(F)
            h = ((dn + F(1.0)).astype(F) * F(0.5)).astype(F)
            t = (t * ((h * h).astype(F) + F(0.2)).astype(F)).astype(F)
    return dict(t=t, live=live, probe=probe, O=O, d=d, L=L, buried=buried, weight=w, weighted=weighted)


def shade(grid, coefficients, records, obj, nd, pos, albedo=None, flags=0, band_weight=PG.IRRADIANCE, depth=None, R=None, bias=0.0, min_variance=1e-4, rows=None):
    """srt_shade_probe_grid_states over a whole frame: ((H, W, 4) float32, counts).  depth: None (the parent is srt_shade_probe_grid)
    or the (P, R*R, 4) moments (the parent is srt_shade_probe_grid_depth).  counts: pixels, corners, segments, open, wave_trips of the
    band `rows` of MEMORY rows, and skipped (corners rule 3s dropped), all8 (hit pixels whose corners are all buried), and
    used, the probe indices of the corners that entered the sum."""
    assert not flags & PG.VISIBILITY
    obj = np.asarray(obj)
    H, W = obj.shape
    out = np.zeros(obj.shape + (4,), dtype=F)
    pix = np.flatnonzero(obj.reshape(-1) != -1)
    y0, y1 = (0, H) if rows is None else (H - rows[1], H - rows[0])
    hit = (obj != -1)[y0:y1]
    trips = sum((int(hit[ty:ty + 8, tx:tx + 8].sum()) + 7) // 8 for ty in range(0, y1 - y0, 8) for tx in range(0, W, 8))
    counts = dict(pixels=int(hit.sum()), corners=0, segments=0, open=0, wave_trips=trips, skipped=0, all8=0, used=np.zeros(0, np.int64))
    if len(pix) == 0:
        return out, counts
    x = np.asarray(pos, dtype=F).reshape(-1, 4)[pix, :3]
    n = np.asarray(nd, dtype=F).reshape(-1, 4)[pix, :3]
    c = corners(grid, records, x, n, flags)
    live, t = c["live"], c["t"]
    ok = live
    in_band = ((pix // W >= y0) & (pix // W < y1))[:, None]
    counts["corners"] = int((live & in_band).sum())
    if depth is not None:
        depth = np.asarray(depth, dtype=F).reshape(grid.probes, R * R, 4)
        tau = PD.encode(c["d"].reshape(-1, 3), R).reshape(live.shape)
        mo = depth[c["probe"], tau]
        t, _ = PD.chebyshev(t, c["L"], mo[..., 0], mo[..., 1], bias, min_variance)
        with np.errstate(invalid="ignore"):
            ok = live & (t > 0)
        counts["segments"] = counts["corners"]
        counts["open"] = int((ok & in_band).sum())
    counts["skipped"] = int((c["buried"] & in_band).sum())
    counts["all8"] = int(((c["buried"] | ~c["weighted"]).all(axis=1) & c["buried"].any(axis=1)).sum())  # (a corner of weight 0 does not exist)
    counts["used"] = np.unique(c["probe"][ok])
    e = PG.corner_irradiance(coefficients, c["probe"], n, band_weight)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        E = np.zeros((len(pix), 3), dtype=F)
        T = np.zeros(len(pix), dtype=F)
        for k in range(8):
            term = np.where(ok[:, k, None], (t[:, k, None] * e[:, k, :]).astype(F), F(0.0)).astype(F)
            E = (E + term).astype(F)
            T = (T + np.where(ok[:, k], t[:, k], F(0.0)).astype(F)).astype(F)
        good = T > 0
        rgba = np.zeros((len(pix), 4), dtype=F)
        rgba[good, :3] = (E[good] / T[good, None]).astype(F)
        rgba[good, 3] = T[good]
        if flags & PG.ALBEDO:
            a = np.asarray(albedo, dtype=F).reshape(-1, 4)[pix, :3]
            rgba[good, :3] = (rgba[good, :3] * a[good]).astype(F)
    out.reshape(-1, 4)[pix] = rgba
    return out, counts


def synthetic_room():
    """The classification tests' room: six wall boxes around [-3, 3] x [-1, 3] x [0, 6], a box of half size 1.2 that the grid's
    planes cut, a small sphere (radius 0.3) that swallows one probe and a big one (radius 1.5) that buries several."""
    wall = lambda p, h: dict(type=BOX, position=p, half_size=h, base=(0.6, 0.6, 0.6))
    return [wall((0.0, -1.25, 3.0), (3.5, 0.25, 3.5)), wall((0.0, 3.25, 3.0), (3.5, 0.25, 3.5)), wall((-3.25, 1.0, 3.0), (0.25, 2.5, 3.5)),
            wall((3.25, 1.0, 3.0), (0.25, 2.5, 3.5)), wall((0.0, 1.0, -0.25), (3.5, 2.5, 0.25)), wall((0.0, 1.0, 6.25), (3.5, 2.5, 0.25)),
            dict(type=BOX, position=(-1.3, 0.2, 3.6), half_size=(1.2, 1.2, 1.2), base=(0.7, 0.3, 0.2)),
            dict(type=SPHERE, position=(1.52, 2.04, 1.03), radius=0.3, base=(0.2, 0.4, 0.9)),
            dict(type=SPHERE, position=(1.4, 0.4, 4.1), radius=1.5, base=(0.3, 0.8, 0.3))]


def room_grid(spacing=0.5, counts=(9, 9, 9)):
    """A grid over the room whose lowest plane lies in the floor: origin (-2.05, -1.3, 0.4), off the objects' faces."""
    return PG.Grid((-2.05, -1.3, 0.4), (spacing, spacing, spacing), counts)


def sphere_directions(K):
    """K unit directions (K, 4) float32: light_probe_reference's spherical Fibonacci set where it exists, else the same formula."""
    if hasattr(LP, "sphere"):
        return np.asarray(LP.sphere(K), dtype=F).reshape(-1, 4)
    i = np.arange(K, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / K
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    out = np.zeros((K, 4), dtype=F)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = r * np.cos(phi), r * np.sin(phi), z, 4.0 * np.pi / K
    return out
