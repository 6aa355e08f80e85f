"""Inputs of the probe sweep (tests/test_gpu_probe_fuzz.py): the random scene families of the ray-query sweep — unit, far, tiny,
mixed, offset, and the 3400-sphere scene that is read from memory, with and without a mesh — seen through a 26 x 16 frame, two probe
grids, five probe points and synthetic grid data, for the passes that start rays or take measurements away from the camera: the
reflection guides, the light probes and their depth maps, probe classification, the probe-grid shading calls, the probe tail and
adaptive rendering.  numpy and the oracle only, no device: tests/test_probe_fuzz_inputs.py counts, on the CPU, what these inputs
reach, and build(oracle, key) replays a failing case of the GPU sweep there.

A key is a seed or one of "large", "large-mesh"; its kind is key % 5 as in the query sweep, and its SCENE is the query sweep's:
query_fuzz_inputs.scene(oracle, SCENE_SHIFT + key), generator 7200 + SCENE_SHIFT + key, so both sweeps see the same families of
geometry.  SCENE_SHIFT = 375 is where the ten default seeds meet every condition of tests/test_probe_fuzz_inputs.py at once.
Everything this file draws on top of the scene comes from a generator of its own, SEED_BASE + key (8675 .. 8998 for the keys in
use; 8673 and 8674 for the large cases), apart from the render sweep's 1000, the blocks sweep's 5000, the query sweep's
7200 .. 8199 and the environments' 9000 (the environment of a case is test_gpu_fuzz._random_environment's number SCENE_SHIFT + key,
990 / 991 for the large cases, drawn by that function from its own generator).  CLAMP_KEYS are five more keys, one per kind, at
which hit points of the frame lie outside `grid`: the shading and the tail test of the GPU sweep run them besides the default keys.

A case holds
  the frame     26 x 16 (26 is no multiple of the 8-pixel tile); a camera in front of the scene, turned about the up axis and then
                about its right axis by the angles test_gpu_query_fuzz._camera draws (the rotation is Rodrigues' formula in float64,
                rounded once); test_gpu_fuzz._random_environment's environment; the camera rays; the oracle's G-buffer
                (visibility_reference.oracle_gbuffer) and the albedo guide (the base colour clamped at 0)
  the grids     `grid`: (5, 4, 6) probes over off +- 6 * scale, 1.5 times the volume the objects are drawn in, so the spacing
                differs per axis and outer probes can be IDLE in mesh-free scenes; `flat`: (7, 1, 3) over +- 2.5 * scale about
                off, one probe along y, so that hit points of every frame lie outside it and corners are skipped; in a scene with a
                negative-radius sphere (`mixed`) about the first such sphere's centre instead, where its middle probe then stands:
                that probe is INSIDE by the table's |radius| alone;
                65 directions (probe_states_reference.sphere_directions: one more than a wave) and the same directions scaled to
                length 0.5 and 3 in turn, for the NORMALIZE flags
  the probes    the camera position, two points of the volume, a point strictly inside a sphere (in `mixed` an enlarged or
                negative-radius one where there is one; the largest sphere that keeps the binary32 point inside otherwise; a
                volume point in a scene without spheres) and a surface point lifted by normal * .00001f in binary32 (the first
                hit pixel's; a volume point in a frame without a hit)
  grid data     from the case's generator, for both grids and for the two levels of the cascade (probe_cascade_reference.grids
                around the centroid of the hit points, base spacing = scale, counts (5, 5, 5), blend_cells 1, R = 4): coefficients
                of both signs, R = 4 depth moments with m1 of the size of a cell and six non-finite values, and state records of
                which about a quarter are BURIED and a third MOVED, both with non-zero offsets within 0.45 of the spacing
  parameters    seeds for the traces and the per-pixel sample counts of the adaptive call, drawn from {0, 1, 2, 3, 5, 9}

The references that the CPU conditions and the GPU sweep share are computed once per case and kept: reflection(), classified(),
grid_segments(), paths().

Inputs the header does not pin, and what this file does about them (nothing is masked after the fact):
  - directions outside the unit window in a scene with triangles (srt_trace_rays, "Input domain": "In a scene with triangles only
    unit-length directions are pinned"): the directions of length 0.5 and 3 are traced with the NORMALIZE flag, which returns them to
    the window, in every scene; without the flag they are traced in scenes without triangles only (c.scaled_unnormalized).  The
    camera's rays and the 65 unit directions are asserted to lie inside the window here.
  - all-zero directions (the same block: "outside what srt_render itself produces"): none is drawn.
  - a sun_direction that is not of unit length in a scene with triangles (srt_render_visibility, rule 4): no pass of this sweep
    sends a ray along the sun; the environment only colours misses, which srt_render pins for every sun_direction
    (tests/test_gpu_fuzz.py), so the environment is used as drawn."""
import numpy as np

import probe_cascade_reference as PC
import probe_grid_reference as PG
import probe_states_reference as PS
import probe_tail_reference as PT
import query_fuzz_inputs as q
import reflection_reference as RR
import visibility_reference as VR
from test_gpu_fuzz import _random_environment
from test_gpu_radiance import camera_rays
from test_gpu_rays import _oracle

F = np.float32
SEED_BASE = 8675
SCENE_SHIFT = 375
CLAMP_KEYS = (160, 126, 132, 323, 14)  # one per kind: see tests/test_probe_fuzz_inputs.py
DEFAULT_SEEDS = 10  # two per kind
LARGE = q.LARGE
KINDS = q.KINDS
W, H = 26, 16
COUNTS, FLAT_COUNTS, FLAT_HALF = (5, 4, 6), (7, 1, 3), 2.5
K, R = 65, 4
BUDGETS = np.array([0, 1, 2, 3, 5, 9], np.uint32)
PROBE_NAMES = ("camera", "volume", "volume 2", "inside a sphere", "lifted surface point")
THRESHOLDS = ((1.0, 1.0), (0.5, 0.5), (0.0, 0.0))
MAX_BOUNCES = 8


class Case:
    """See the module's docstring."""


def scene_key(key):
    """The key of the query sweep whose scene case `key` has."""
    return key if key in LARGE else int(key) + SCENE_SHIFT


def index_of(key):
    """The number of a key's environment: the number of its scene's seed, or 990 + its place in LARGE."""
    return 990 + LARGE.index(key) if key in LARGE else int(key) + SCENE_SHIFT


def generator_of(key):
    """The seed of the generator of everything build() draws: SEED_BASE + key, and the two below SEED_BASE for LARGE."""
    return SEED_BASE - 2 + LARGE.index(key) if key in LARGE else SEED_BASE + int(key)


def rotated(v, angle, axis):
    """Rodrigues' rotation of v about the unit vector `axis` in float64."""
    v, k = np.asarray(v, np.float64), np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    return v * np.cos(angle) + np.cross(k, v) * np.sin(angle) + k * np.dot(k, v) * (1.0 - np.cos(angle))


def camera(oracle, c, rng):
    cam = oracle.Camera()
    pos = c.off - np.array([0, 0, 6.0]) * c.scale + rng.uniform(-1, 1, 3) * c.scale
    basis = np.eye(3)
    a = float(rng.uniform(-0.5, 0.5))
    basis = np.array([rotated(b, a, (0, 1, 0)) for b in basis])
    a = float(rng.uniform(-0.3, 0.3))
    basis = np.array([rotated(b, a, basis[0]) for b in basis])
    cam.position = oracle.f3(pos)
    cam.right, cam.up, cam.forward = oracle.f3(basis[0]), oracle.f3(basis[1]), oracle.f3(basis[2])
    cam.fov_degrees = int(rng.integers(15, 104))
    return cam


def grid_data(rng, grid, scale):
    """(coefficients (P, 9, 4), moments (P, R*R, 4), records (P, 4)) of one grid."""
    P = grid.probes
    co = rng.uniform(-0.6, 1.4, (P, 9, 4)).astype(F)
    co[:, 0, :3] += F(1.0)  # (a mostly positive mean, with negative lobes)
    cell = float(np.linalg.norm(grid.spacing.astype(np.float64)))
    m1 = rng.uniform(0.05, 1.0, (P, R * R)) * cell
    mo = np.empty((P, R * R, 4), F)
    mo[..., 0] = m1
    mo[..., 1] = m1 * m1 + rng.uniform(0.0, 0.05, (P, R * R)) * cell * cell
    mo[..., 2:] = rng.uniform(0.0, 4.0, (P, R * R, 2))
    odd = [np.nan, np.inf, -np.inf]
    for j in range(6):  # a few values that are not finite, in the two lanes the shading reads
        mo[int(rng.integers(0, P)), int(rng.integers(0, R * R)), j % 2] = odd[j % 3]
    rec = np.zeros((P, 4), F)
    u = rng.uniform(size=P)
    buried, moved = u < 0.25, (u >= 0.25) & (u < 0.58)
    bits = np.zeros(P, np.uint32)
    bits[buried] = PS.BURIED | PS.INSIDE
    bits[moved] = PS.MOVED | np.where(rng.uniform(size=int(moved.sum())) < 0.3, PS.INSIDE, 0).astype(np.uint32)
    bits[(u >= 0.95)] = PS.IDLE
    shifted = moved | (buried & (rng.uniform(size=P) < 0.5))
    lo = np.where(np.array(grid.counts) > 1, 0.05, 0.0)  # (|offset| >= 0.05 spacing: never zero; the one-probe axis keeps its plane)
    off = rng.uniform(0.05, 0.45, (P, 3)) * rng.choice([-1.0, 1.0], (P, 3)) * grid.spacing.astype(np.float64)[None, :]
    rec[shifted, :3] = (off * (lo > 0)[None, :])[shifted]
    rec[:, 3] = bits.view(F)
    return co, mo, rec


def _inside_point(oracle, c, rng):
    """A binary32 point strictly inside a sphere of the scene, or None."""
    spheres = [o for o in c.objs if o.get("type") == oracle.OBJ_SPHERE and np.isfinite(o["radius"]) and o["radius"] != 0]
    odd = [o for o in spheres if abs(o["radius"]) > 0.6 * c.scale or o["radius"] < 0]
    order = sorted(spheres, key=lambda o: -abs(o["radius"]))
    if c.kind == "mixed" and odd:
        order = sorted(odd, key=lambda o: -abs(o["radius"])) + order
    d = q._random_directions(rng, 1)[0].astype(np.float64)
    for o in order:
        cen, r = np.array(o["position"], np.float64), abs(o["radius"])
        p = (cen + 0.3 * r * d).astype(F)
        if np.linalg.norm(p.astype(np.float64) - cen.astype(F).astype(np.float64)) < 0.9 * abs(float(F(r))):
            return p
    return None


def build(oracle, key):
    """The case of `key` (a seed, or "large" / "large-mesh")."""
    kind, objs, meshes, off, scale, _ = q.scene(oracle, scene_key(key))
    rng = np.random.default_rng(generator_of(key))
    c = Case()
    c.key, c.kind, c.objs, c.meshes, c.off, c.scale = key, kind, objs, meshes, np.asarray(off, np.float64), float(scale)
    c.oarr, c.n = oracle.make_objects(objs)
    marr, mn, keep = oracle.make_meshes(meshes)
    c.marr, c.mn, c.om = marr, mn, ((marr, mn, keep) if mn else None)
    c.triangles = any(o.get("type") == oracle.OBJ_MESH for o in objs) and mn > 0
    c.mesh_free = not any(o.get("type") == oracle.OBJ_MESH for o in objs)
    c.scaled_unnormalized = not c.triangles
    c.enlarged = [o for o in objs if o.get("type") == oracle.OBJ_SPHERE and abs(o["radius"]) > 100 * scale]

    # the frame
    c.cam = camera(oracle, c, rng)
    c.env, c.env_kind = _random_environment(oracle, index_of(key), c.cam, W, H)
    c.O4, c.D4 = camera_rays(oracle, c.cam, W, H)
    assert np.all(np.abs(q.dd64(c.D4[:, :3]) - 1) < 0.9e-6)  # (the camera's rays are inside the unit window)
    c.obj, c.nd, c.pos = VR.oracle_gbuffer(oracle, c.oarr, c.n, c.cam, W, H, c.om)
    c.hit = c.obj != -1
    c.hits = int(c.hit.sum())
    c.alb = np.zeros((H, W, 4), F)
    for i in np.unique(c.obj[c.hit]):
        c.alb[c.obj == i, :3] = [RR.c0(v) for v in c.oarr[int(i)].material.base_color]

    # the grids and the directions
    lo = (c.off - 6.0 * scale).astype(F)
    c.grid = PG.Grid(lo, [12.0 * scale / (n - 1) for n in COUNTS], COUNTS)
    c.negative = [o for o in objs if o.get("type") == oracle.OBJ_SPHERE and o["radius"] < 0]
    c.flat_centre = np.array(c.negative[0]["position"], np.float64) if c.negative else c.off  # (its middle probe: inside that sphere by |radius| alone)
    flo = (c.flat_centre - FLAT_HALF * scale).astype(F)
    c.flat = PG.Grid((flo[0], F(c.flat_centre[1]), flo[2]), [2.0 * FLAT_HALF * scale / (n - 1) if n > 1 else scale for n in FLAT_COUNTS], FLAT_COUNTS)
    c.dirs = PS.sphere_directions(K)
    assert np.all(np.abs(q.dd64(c.dirs[:, :3]) - 1) < 0.9e-6)
    c.scaled = c.dirs.copy()
    c.scaled[:, :3] = c.dirs[:, :3] * np.where(np.arange(K) % 2, F(3.0), F(0.5))[:, None]
    c.max_distance = float(F(1.5 * np.linalg.norm(c.grid.spacing.astype(np.float64))))  # 1.5 cell diagonals

    # the probe points
    vol = lambda: c.off + rng.uniform(-4, 4, 3) * scale
    inside = _inside_point(oracle, c, rng)
    c.has_inside = inside is not None
    c.has_lifted = c.hits > 0
    if c.has_lifted:
        first = int(np.flatnonzero(c.hit.reshape(-1))[rng.integers(0, c.hits)])
        p, nrm = c.pos.reshape(-1, 4)[first, :3], c.nd.reshape(-1, 4)[first, :3]
        lifted = (p + (nrm * F(.00001)).astype(F)).astype(F)
        c.has_lifted = bool(np.isfinite(lifted).all())
    c.probes = np.zeros((5, 4), F)
    c.probes[0, :3] = c.O4[0, :3]
    c.probes[1, :3], c.probes[2, :3] = vol(), vol()
    c.probes[3, :3] = inside if c.has_inside else vol()
    c.probes[4, :3] = lifted if c.has_lifted else vol()

    # synthetic grid data: the two grids and the cascade's levels
    c.co, c.mo, c.rec = grid_data(rng, c.grid, scale)
    c.flat_co, c.flat_mo, c.flat_rec = grid_data(rng, c.flat, scale)
    centre = c.pos[c.hit][:, :3].astype(np.float64).mean(axis=0) if c.hits else c.off
    c.cascade = PC.grids(centre if np.isfinite(centre).all() else c.off, (scale, scale, scale), (5, 5, 5), 2)
    c.cascade.resolution = R
    c.cas_co, c.cas_mo, c.cas_rec = (list(v) for v in zip(*[grid_data(rng, g, scale) for g in c.cascade.grids]))

    # parameters
    c.seeds = {k: int(rng.integers(0, 2**31)) for k in ("probes", "tail", "adaptive", "chain")}
    c.budget = BUDGETS[rng.integers(0, len(BUDGETS), (H, W))]
    c._kept = {}
    return c


_cases = {}


def case(oracle, key):
    """build(), once per session for the default cases and CLAMP_KEYS: the CPU conditions and the GPU sweep share them and leave
    them unchanged (the seeds of a longer sweep are built, used once and dropped)."""
    if key in _cases:
        return _cases[key]
    c = build(oracle, key)
    if key in LARGE or key < DEFAULT_SEEDS or key in CLAMP_KEYS:
        _cases[key] = c
    return c


def _keep(c, name, make):
    if name not in c._kept:
        c._kept[name] = make()
    return c._kept[name]


# ---- the references that the CPU conditions and the GPU sweep share ----------------------------------------------------------------
def reflection(oracle, c, thresholds):
    """reflection_reference.reference of the frame at (min_smoothness, min_specular) = thresholds, max_bounces 8."""
    return _keep(c, ("reflection", thresholds), lambda: RR.reference(oracle, c.oarr, c.n, c.cam, W, H, om=c.om, max_bounces=MAX_BOUNCES,
                                                                     min_smoothness=thresholds[0], min_specular=thresholds[1]))


WAYS = {"relocate": PS.RELOCATE, "rest": 0, "normalize": PS.RELOCATE | PS.NORMALIZE}


def classified(c, which, way):
    """probe_states_reference.classify of grid `which` ("grid" / "flat") one of three `way`s: with RELOCATE on the unit
    directions, without it, with RELOCATE | NORMALIZE on the scaled ones."""
    d = c.scaled if way == "normalize" else c.dirs
    return _keep(c, ("classified", which, way), lambda: PS.classify(getattr(c, which), c.objs, d, WAYS[way]))


def grid_segments(oracle, c, which="grid"):
    """(pix, corner, O4, D4, occluded) of probe_grid_reference.segments on the frame's guides, answered by the oracle."""
    def make():
        pix, corner, O4, D4 = PG.segments(getattr(c, which), c.obj, c.nd, c.pos)
        return pix, corner, O4, D4, VR.occluded_by_oracle(oracle, c.oarr, c.n, O4, D4, c.om)
    return _keep(c, ("segments", which), make)


def tail_scene(oracle, c):
    return _keep(c, "tail scene", lambda: PT.Scene(oracle, c.oarr, c.n, om=c.om[:2] if c.om else None, env=c.env))


def paths(oracle, c, bounces, samples, seed):
    """probe_tail_reference.trace of the frame's camera rays: (colours (N, samples, 4), terminals, ray-major)."""
    return _keep(c, ("paths", bounces, samples, seed), lambda: PT.trace(tail_scene(oracle, c), c.O4, c.D4, samples, bounces, seed=seed))


def closest(oracle, c, positions, directions):
    """The oracle's closest hit of the explicit P*K batch: (index (P, K), distance (P, K) with +inf on a miss)."""
    P, Kd = len(positions), len(directions)
    O4, D4 = np.repeat(positions, Kd, axis=0).astype(F), np.tile(directions, (P, 1)).astype(F)
    idx, _, _, t = _oracle(oracle, c.oarr, c.n, O4, D4, c.om)
    return idx.reshape(P, Kd), np.where(idx >= 0, t, F(np.inf)).astype(F).reshape(P, Kd)


def where(c):
    return "key %s (%s, environment %s)" % (c.key, c.kind, c.env_kind)
