"""Inputs of the ray-query sweep (tests/test_gpu_query_fuzz.py): the random scene families of tests/test_gpu_fuzz.py — unit, far,
tiny, mixed, offset — and the 3400-sphere scene that does not fit in LDS, each with five families of rays, directions at the
edges of the contract of include/srt_pathtrace.h (srt_trace_rays' "Input domain") and the t_max sets of the any-hit query.
numpy and the oracle only, no device: tests/test_query_fuzz_inputs.py counts, on the CPU, what these inputs reach.

Ray families (all origins finite; every case concatenates them into ONE batch, so that the rays of two families share a wave):
  A  origins in front of the scene as the fuzz camera stands, aimed at points of the scene volume: primary-ray-like queries
  B  origins uniform in the scene volume, random directions: origins among the objects
  C  origins on surfaces — the oracle's hit points of A, lifted by normal * .00001f in binary32 as srt_render_visibility and the
     probe-grid pass lift them — half with random directions on the normal's side, half towards a second point p (another
     ray's hit point or a point of the volume) with d = unit(p - o) and t_max = |p - o|: the segments the visibility passes send
  D  origins inside spheres (in `mixed`: the 30x, 300x and negative-radius ones among them): the t_max <= 0 path
  E  origins on a shell 3 to 10 times the scene's extent (the largest radius included) from its middle, a third aimed at objects
     (every other one at the centre — of a triangle, for a mesh — the rest at a point 0.9 to 1.1 radii from it, where a cull is
     decided), a third tangential, a third outward: large |o|_1 against the object sizes, and misses where a sphere encloses all

Directions are numpy-binary32 normalized (test_gpu_rays._unit); per family a tenth are rescaled to d.d = 1 -+ 0.8e-6 (inside the
unit window), a tenth have one or two components exactly +0.0 or -0.0, two have a NaN component, and in scenes without triangles
a further tenth are rescaled to d.d = 1 -+ 1.5e-6 (outside the window) and six have length 0.5 or 3.  All-zero directions,
infinite components and origins beyond 1e29 are left out: the contract does not pin them."""
import numpy as np

from test_gpu_fuzz import _random_scene
from test_gpu_rays import _oracle, _rays, _unit

F = np.float32
KINDS = ["unit", "far", "tiny", "mixed", "offset"]
SEED_BASE = 7200  # (the render sweep draws from 1000 + seed, the blocks sweep from 5000 + seed, the environments from 9000 + seed)
DEFAULT_SEEDS = 20
LARGE = ("large", "large-mesh")
FAMILIES = "ABCDE"
SIZES = dict(A=397, B=384, C=419, D=320, E=390)  # 1910 rays; none but B a multiple of 64
PLAIN, WINDOW, ZERO, OUTSIDE, LENGTH, NAN = range(6)  # direction tags
TAG_NAMES = ["plain", "d.d=1-+0.8e-6", "zero component", "d.d=1-+1.5e-6", "length 0.5 / 3", "NaN component"]
FINITE_SETS = ("t", "above t", "below t", "0", "-0", "t/2", "uniform", "segment")


class Case:
    """A scene (oracle arrays), one batch of rays with t_max = +inf, the family and direction tag of every ray, the oracle's
    closest hits (index, normal, point, distance) and the t_max sets."""


def large_scene(oracle, with_mesh):
    """The recipe of test_gpu_fuzz.test_scene_larger_than_lds: 3400 spheres, 60 boxes and a floor sphere of radius 1000, whose
    scene image cannot sit in LDS."""
    rng = np.random.default_rng(77)
    objs = []
    for _ in range(3400):
        objs.append(dict(type=oracle.OBJ_SPHERE, position=tuple(float(v) for v in (rng.uniform(-6, 6), rng.uniform(-3, 3), rng.uniform(4, 16))),
                         radius=float(rng.uniform(0.03, 0.25)) * (8.0 if rng.uniform() < 0.01 else 1.0),
                         base=tuple(float(v) for v in rng.uniform(0, 1, 3)), emissive=tuple(float(v) for v in rng.uniform(0, 3, 3) * (rng.uniform() < 0.05)),
                         specular_amount=float(rng.uniform(0, 1)), smoothness=float(rng.uniform(0, 1))))
    for _ in range(60):
        objs.append(dict(type=oracle.OBJ_BOX, position=tuple(float(v) for v in (rng.uniform(-6, 6), rng.uniform(-3, 3), rng.uniform(4, 16))),
                         half_size=tuple(float(v) for v in rng.uniform(0.05, 0.5, 3)), base=tuple(float(v) for v in rng.uniform(0, 1, 3)),
                         specular_amount=float(rng.uniform(0, 1)), smoothness=float(rng.uniform(0, 1))))
    objs.append(dict(type=oracle.OBJ_SPHERE, position=(0.0, -1003.5, 8.0), radius=1000.0, base=(0.6, 0.6, 0.6)))
    meshes = []
    if with_mesh:
        meshes.append(oracle.uv_sphere(0.8, 12, 16))
        objs.append(dict(type=oracle.OBJ_MESH, position=(0.3, 0.2, 3.0), mesh=0, base=(0.9, 0.5, 0.2), smoothness=0.3))
    order = rng.permutation(len(objs))
    return [objs[i] for i in order], meshes, np.array([0.0, 0.0, 10.0]), 1.5  # (the volume off +- 4 * scale holds the spheres)


def scene(oracle, key):
    """(kind, objects, meshes, off, scale, generator) of case `key`: a seed of the cycle or one of LARGE."""
    if key in LARGE:
        rng = np.random.default_rng(SEED_BASE + 900 + LARGE.index(key))
        return ("large",) + large_scene(oracle, key == "large-mesh") + (rng,)
    rng = np.random.default_rng(SEED_BASE + key)
    kind = KINDS[key % 5]
    return (kind,) + _random_scene(oracle, rng, kind) + (rng,)


def _extent(oracle, objs, meshes, off, scale):
    """The radius about `off` of a ball that holds every object, enlarged spheres included."""
    ext = 4.0 * np.sqrt(3.0) * scale
    for o in objs:
        if o.get("type") in (None, oracle.OBJ_NONE):
            continue
        size = {oracle.OBJ_SPHERE: abs(o.get("radius", 0.0)), oracle.OBJ_BOX: float(np.linalg.norm(o.get("half_size", (0, 0, 0)))),
                oracle.OBJ_MESH: max([float(np.linalg.norm(np.where(np.isfinite(V), V, 0.0), axis=1).max()) for V, _ in meshes] + [0.0])}[o["type"]]
        if np.isfinite(size):
            ext = max(ext, float(np.linalg.norm(np.array(o["position"]) - off)) + size)
    return ext


def _rescaled(d, target):
    """d * s in binary32 with d.d = target, d.d taken in float64 from the binary32 components (two rounds: the components' own
    rounding moves d.d by up to 1.2e-7)."""
    d = np.asarray(d, F)
    for _ in range(2):
        dd = (d.astype(np.float64) ** 2).sum(axis=1)
        d = (d.astype(np.float64) * np.sqrt(target / dd)[:, None]).astype(F)
    return d


def dd64(d):
    return (np.asarray(d, F).astype(np.float64) ** 2).sum(axis=-1)


def _special_directions(rng, d, analytic):
    """The direction edges of one family: returns (directions, tags)."""
    n = len(d)
    d, tag = d.copy(), np.full(n, PLAIN, np.int32)
    perm, k = rng.permutation(n), n // 10
    window, zero, nan = perm[:k], perm[k:2 * k], perm[-2:]
    d[window] = _rescaled(d[window], 1.0 + 0.8e-6 * np.where(np.arange(k) % 2, 1.0, -1.0))
    tag[window] = WINDOW
    for i in zero:
        comps = rng.permutation(np.delete(np.arange(3), np.argmax(np.abs(d[i]))))[:int(rng.integers(1, 3))]  # (the largest stays)
        d[i, comps] = rng.choice(np.array([0.0, -0.0], F), len(comps))
    d[zero] = _unit(d[zero])
    tag[zero] = ZERO
    if analytic:
        outside, length = perm[2 * k:3 * k], perm[3 * k:3 * k + 6]
        d[outside] = _rescaled(d[outside], 1.0 + 1.5e-6 * np.where(np.arange(k) % 2, 1.0, -1.0))
        tag[outside] = OUTSIDE
        d[length] = d[length] * np.array([0.5, 3.0] * 3, F)[:, None]
        tag[length] = LENGTH
    for i in nan:
        d[i, int(rng.integers(0, 3))] = np.nan
    tag[nan] = NAN
    return d, tag


def _random_directions(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def build(oracle, key):
    """The case of `key` (a seed, or "large" / "large-mesh")."""
    kind, objs, meshes, off, scale, rng = scene(oracle, key)
    c = Case()
    c.key, c.kind, c.objs, c.meshes, c.off, c.scale = key, kind, objs, meshes, off, scale
    c.oarr, c.n = oracle.make_objects(objs)
    marr, mn, keep = oracle.make_meshes(meshes)
    c.marr, c.mn, c.om = marr, mn, ((marr, mn, keep) if mn else None)
    c.triangles = any(o.get("type") == oracle.OBJ_MESH for o in objs) and mn > 0
    c.broken_mesh = any((T >= len(V)).any() or not np.isfinite(V).all() for V, T in meshes)
    c.has_none = any(o.get("type", oracle.OBJ_NONE) == oracle.OBJ_NONE for o in objs)
    c.mesh_objects = np.array([i for i, o in enumerate(objs) if o.get("type") == oracle.OBJ_MESH], np.int32)
    spheres = [o for o in objs if o.get("type") == oracle.OBJ_SPHERE and np.isfinite(o["radius"]) and o["radius"] != 0]
    c.enlarged = np.array([i for i, o in enumerate(objs) if o.get("type") == oracle.OBJ_SPHERE and kind == "mixed" and abs(o["radius"]) > 0.6 * scale], np.int32)
    analytic = not c.triangles
    vol = lambda k: off + rng.uniform(-4, 4, (k, 3)) * scale
    fam = {}

    # A: in front of the scene, aimed into the volume
    oa = off - np.array([0.0, 0.0, 6.0]) * scale + rng.uniform(-1, 1, (SIZES["A"], 3)) * scale
    fam["A"] = (oa, _unit(vol(SIZES["A"]) - oa), None)
    # B: among the objects
    fam["B"] = (vol(SIZES["B"]), _random_directions(rng, SIZES["B"]), None)
    # D: inside spheres; in `mixed` half the picks are the enlarged and the negative-radius spheres
    if spheres:
        odd = [o for o in spheres if abs(o["radius"]) > 0.6 * scale or o["radius"] < 0]
        pick = [spheres[i] for i in rng.integers(0, len(spheres), SIZES["D"])]
        if kind == "mixed" and odd:
            pick[::2] = [odd[i] for i in rng.integers(0, len(odd), len(pick[::2]))]
        cen, rad = np.array([o["position"] for o in pick]), np.array([abs(o["radius"]) for o in pick])
        fam["D"] = (cen + rng.uniform(-0.5, 0.5, (SIZES["D"], 3)) * rad[:, None], _random_directions(rng, SIZES["D"]), None)
    # E: a shell well outside everything
    k = SIZES["E"]
    ext = _extent(oracle, objs, meshes, off, scale)
    radial = _random_directions(rng, k).astype(np.float64)
    oe = off + radial * (rng.uniform(3, 10, (k, 1)) * ext)
    centres, sizes = [], []
    for o in objs:  # (the centre of a mesh object, a triangle soup, is the middle of one of its triangles)
        if o.get("type") == oracle.OBJ_MESH:
            V, T = meshes[o["mesh"]]
            good = [t for t in T if (t < len(V)).all() and np.isfinite(V[t]).all()]
            centres += [np.array(o["position"]) + V[good[int(i)]].astype(np.float64).mean(axis=0) for i in rng.integers(0, len(good), 8)] if good else []
        elif o.get("type", oracle.OBJ_NONE) != oracle.OBJ_NONE:
            centres.append(np.array(o["position"], np.float64))
        size = abs(o.get("radius", 0.0)) if o.get("type") == oracle.OBJ_SPHERE else float(np.linalg.norm(o.get("half_size", (0, 0, 0)))) / np.sqrt(3.0)
        sizes += [size if np.isfinite(size) else 0.0] * (len(centres) - len(sizes))
    centres, sizes = np.array(centres or [off], np.float64), np.array(sizes or [0.0])
    de = np.empty((k, 3), F)
    third = np.arange(k) % 3
    # every other inward ray grazes its object: it is aimed at a point 0.9 to 1.1 radii from the centre, where a cull is decided
    at = rng.integers(0, len(centres), int((third == 0).sum()))
    graze = _random_directions(rng, len(at)) * (sizes[at] * rng.uniform(0.9, 1.1, len(at)) * (np.arange(len(at)) % 2))[:, None]
    de[third == 0] = _unit(centres[at] + graze - oe[third == 0])
    de[third == 1] = _unit(np.cross(radial[third == 1], rng.normal(size=(int((third == 1).sum()), 3))))
    de[third == 2] = _unit(radial[third == 2] + 0.5 * _random_directions(rng, int((third == 2).sum())))
    fam["E"] = (oe, de, None)

    # the direction edges, then A's hits for the origins of C
    done = {}
    for f in "ABDE":
        if f in fam:
            d, tag = _special_directions(rng, fam[f][1], analytic)
            done[f] = _rays(fam[f][0], d) + (tag, None)
    ref_a = _oracle(oracle, c.oarr, c.n, done["A"][0], done["A"][1], c.om)
    hits = np.flatnonzero((ref_a[0] >= 0) & np.isfinite(ref_a[1]).all(axis=1) & np.isfinite(ref_a[2]).all(axis=1))  # (a box can be hit by a NaN ray)
    c.p2p = np.zeros(0, bool)
    if len(hits):
        k = SIZES["C"]
        src = hits[rng.integers(0, len(hits), k)]
        p, nrm = ref_a[2][src], ref_a[1][src]
        oc = (p + nrm * F(.00001)).astype(F)  # binary32, no FMA: the bounce origin of the visibility passes
        dc = _random_directions(rng, k)
        flip = ((dc[:, 0] * nrm[:, 0] + dc[:, 1] * nrm[:, 1]) + dc[:, 2] * nrm[:, 2]) < 0
        dc[flip] *= F(-1)
        seg = (rng.uniform(0.5, 3.0, k) * scale).astype(F)  # the hemisphere half: an AO radius
        p2p = np.arange(k) % 2 == 1
        other = ref_a[2][hits[rng.integers(0, len(hits), k)]]
        to = np.where((rng.uniform(size=k) < 0.6)[:, None], other, vol(k).astype(F)).astype(F)
        v = (to - oc).astype(F)
        length = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        p2p &= np.isfinite(length) & (length > 0)
        dc[p2p], seg[p2p] = _unit(v[p2p]), length[p2p]
        d, tag = _special_directions(rng, dc, analytic)
        done["C"] = _rays(oc, d) + (tag, seg)
        c.p2p = p2p

    order = [f for f in FAMILIES if f in done]
    c.O4, c.D4 = np.concatenate([done[f][0] for f in order]), np.concatenate([done[f][1] for f in order])
    c.family = np.concatenate([np.full(len(done[f][0]), FAMILIES.index(f), np.int32) for f in order])
    c.tag = np.concatenate([done[f][2] for f in order])
    assert np.isfinite(c.O4).all() and np.abs(c.O4).max() < 1e29
    rest = c.family != 0  # (A comes first and has been answered)
    c.ref = tuple(np.concatenate([a, b]) for a, b in zip(ref_a, _oracle(oracle, c.oarr, c.n, c.O4[rest], c.D4[rest], c.om)))
    idx, _, _, t = c.ref
    hit = idx >= 0

    # t_max sets
    inf = F(np.inf)
    uniform = np.where(hit, rng.uniform(0, 2, len(t)) * np.abs(t.astype(np.float64)), rng.uniform(0, 12, len(t)) * scale).astype(F)
    c.tmax = {"+inf": np.full_like(t, inf), "t": t.copy(), "above t": np.nextafter(t, inf), "below t": np.nextafter(t, -inf),
              "0": np.zeros_like(t), "-0": np.full_like(t, -0.0), "t/2": (t / F(2)).astype(F), "NaN": np.full_like(t, np.nan),
              "-inf": np.full_like(t, -inf), "uniform": uniform}
    if "C" in done:
        seg = uniform.copy()  # (outside C the segment set repeats the uniform draw)
        seg[c.family == 2] = done["C"][3]
        c.tmax["segment"] = seg

    # SRT_RAYS_NORMALIZE: every third unit direction, scaled by 0.5 or 3 in binary32 (taken from the unit ones, so that the flag
    # returns them to the pinned domain in triangle scenes too), and what the oracle says for the pre-normalized batch
    rows = np.flatnonzero((c.tag == PLAIN) | (c.tag == ZERO))[::3]
    c.norm_rows = rows
    c.norm_O4, c.norm_D4 = c.O4[rows].copy(), c.D4[rows].copy()
    c.norm_D4[:, :3] = c.norm_D4[:, :3] * np.where(np.arange(len(rows)) % 2, F(3.0), F(0.5))[:, None]
    c.norm_D4[:, 3] = uniform[rows]
    c.norm_pre = c.norm_D4.copy()
    c.norm_pre[:, :3] = _unit(c.norm_D4[:, :3])
    c.norm_ref = _oracle(oracle, c.oarr, c.n, c.norm_O4, c.norm_pre, c.om)
    return c


_cases = {}


def case(oracle, key):
    """build(), once per session for the default cases: the CPU conditions and the GPU sweep share them and leave them unchanged
    (the seeds of a longer sweep are built, used once and dropped)."""
    if key in _cases:
        return _cases[key]
    c = build(oracle, key)
    if key in LARGE or key < DEFAULT_SEEDS:
        _cases[key] = c
    return c


def want(c, name):
    """`hit and t < t_max` in binary32 under t_max set `name`."""
    with np.errstate(invalid="ignore"):
        return ((c.ref[0] >= 0) & (c.ref[3] < c.tmax[name])).astype(np.int32)


def describe(c, rows):
    """The first ten of `rows` for a failure message: index, family, direction tag — enough to replay a ray through the oracle
    on the CPU from build(oracle, key)."""
    return ", ".join("%d (%s, %s)" % (i, FAMILIES[c.family[i]], TAG_NAMES[c.tag[i]]) for i in np.asarray(rows)[:10])
