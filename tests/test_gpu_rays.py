"""Ray queries (srt_trace_rays, ABI 7) on the MI355X: the closest hit of caller-supplied rays — object index, normal + distance,
point, albedo and OCCLUDED — bit for bit against the oracle's GetClosestObject (Raytracer.cpp:123-140) called per ray
(srt_oracle_closest / srt_oracle_closest_m): batch sizes around the 64-ray block, the edges srt_render itself produces, every
instantiation, SRT_RAYS_NORMALIZE, the output mask, binding, order against scene updates, what the call leaves alone, its
errors and the layers above the C calls."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path

pytestmark = pytest.mark.gpu

NAMES = ["object", "normal_depth", "position", "albedo", "occluded"]
CLI = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
MISS_ND = np.array([0, 0, 0, np.inf], np.float32).view(np.uint32)


def _tracer(srt, oracle, objs, meshes=None, w=16, h=16, refit=False):
    """A PathTracer with a scene and NO camera: a ray query needs none."""
    oarr, n = oracle.make_objects(objs)
    pt = srt.PathTracer(w, h)
    om = None
    if refit:
        pt.update_mode(True)
    if meshes:
        marr, mn, keep = oracle.make_meshes(meshes)
        pt.set_meshes(C.cast(marr, C.POINTER(srt.Mesh)), mn)
        om = (marr, mn, keep)
    pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
    return pt, oarr, n, om


def _same_bits(a, b):
    """Bit equality, NaNs compared as NaNs (their sign and payload are the processor's)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a) | np.isnan(b)
    return bool(np.all(np.where(nan, np.isnan(a) & np.isnan(b), a.view(np.uint32) == b.view(np.uint32))))


def _unit(v):
    """numpy-float32 normalization, the arithmetic of float3::Normalized: v / sqrt((x*x + y*y) + z*z)."""
    v = np.asarray(v, np.float32).reshape(-1, 3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return (v / np.sqrt((x * x + y * y) + z * z)[:, None]).astype(np.float32)


def _rays(o, d, tmax=np.inf):
    """(N, 3) origins and directions -> the two (N, 4) float32 arrays of srt_write_rays."""
    o, d = np.asarray(o, np.float32).reshape(-1, 3), np.asarray(d, np.float32).reshape(-1, 3)
    O4, D4 = np.zeros((len(o), 4), np.float32), np.zeros((len(o), 4), np.float32)
    O4[:, :3], O4[:, 3] = o, 7.5  # (w is ignored)
    D4[:, :3], D4[:, 3] = d, tmax
    return O4, D4


def _oracle(oracle, oarr, n, O4, D4, om=None):
    """srt_oracle_closest (with om = oracle meshes: srt_oracle_closest_m) per ray: index, normal, point, distance."""
    L = oracle.lib()
    nn, pp, t = (C.c_float * 3)(), (C.c_float * 3)(), C.c_float()
    k = len(O4)
    idx = np.empty(k, np.int32)
    nrm, pnt, dist = np.zeros((k, 3), np.float32), np.zeros((k, 3), np.float32), np.zeros(k, np.float32)
    for i in range(k):
        o, d = (C.c_float * 3)(*O4[i, :3]), (C.c_float * 3)(*D4[i, :3])
        if om:
            idx[i] = L.srt_oracle_closest_m(oarr, n, om[0], om[1], o, d, nn, pp, C.byref(t))
        else:
            idx[i] = L.srt_oracle_closest(oarr, n, o, d, nn, pp, C.byref(t))
        if idx[i] >= 0:
            nrm[i], pnt[i], dist[i] = nn[:], pp[:], t.value
    return idx, nrm, pnt, dist


def _check(g, ref, oarr, D4):
    """All five outputs of `g` (name -> array) against the oracle's results `ref`; returns (hits, misses)."""
    idx, nrm, pnt, dist = ref
    k = len(idx)
    obj, nd, pos, alb, occ = (np.asarray(g[name])[:k] for name in NAMES)
    assert np.array_equal(obj, idx), "object index differs at %d rays" % int((obj != idx).sum())
    hit, miss = idx >= 0, idx < 0
    assert _same_bits(nd[hit, :3], nrm[hit]) and _same_bits(nd[hit, 3], dist[hit]), "normal / distance bits differ"
    assert _same_bits(pos[hit, :3], pnt[hit]) and np.all(pos[hit, 3] == 1.0), "point bits differ"
    base = np.array([list(oarr[int(i)].material.base_color) for i in idx[hit]], np.float32).reshape(-1, 3)
    base = np.where(base < 0, np.float32(0), base)  # Color's clamping constructor (Common.hpp:253-262)
    assert _same_bits(alb[hit, :3], base) and np.all(alb[hit, 3].view(np.uint32) == 0), "albedo bits differ"
    assert np.all(nd[miss].view(np.uint32) == MISS_ND)
    assert np.all(pos[miss].view(np.uint32) == 0) and np.all(alb[miss].view(np.uint32) == 0)
    with np.errstate(invalid="ignore"):
        want = (hit & (dist < D4[:k, 3])).astype(np.int32)  # a binary32 <
    assert np.array_equal(occ, want), "occluded differs at %d rays" % int((occ != want).sum())
    return int(hit.sum()), int(miss.sum())


def _trace(pt, O4, D4, **kw):
    pt.write_rays(O4, D4)
    pt.trace_rays(**kw)
    return {k: pt.ray_output(k) for k in NAMES}


def _box_rays(rng, n, lo=(-5, -1, 0), hi=(5, 4, 10)):
    """Origins uniform in a box around Scene1, directions numpy-float32-normalized random vectors."""
    return _rays(rng.uniform(lo, hi, (n, 3)), _unit(rng.normal(size=(n, 3))))


def _scene1(oracle):
    return oracle.load_scene_json_py(scene_path("Scene1"))


def _sentinels(n):
    import torch

    t = {}
    for k in NAMES:
        t[k] = torch.full((n,) if k in ("object", "occluded") else (n, 4), -7 if k in ("object", "occluded") else 12345.0,
                          dtype=torch.int32 if k in ("object", "occluded") else torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    return t


def _unbind(pt):
    """Back to the handle's own output buffers, once everything enqueued has finished (the shared tracer outlives the tensors)."""
    pt.wait()
    for k in NAMES:
        pt.bind_ray_output(k, None)


def _untouched(t):
    a = t.cpu().numpy()
    return bool(np.all(a == (-7 if a.dtype == np.int32 else 12345.0)))


# ---- batch sizes ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene1(srt, oracle):
    """One tracer of Scene1 (64 clustered and 3 uniform spheres: the LDS instantiation) shared by the tests that only trace."""
    pt, oarr, n, _ = _tracer(srt, oracle, _scene1(oracle))
    yield pt, oarr, n
    pt.close()


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257, 4099])
def test_batch_sizes_match_the_oracle_and_write_nothing_past_the_batch(srt, oracle, scene1, count):
    pt, oarr, n = scene1
    # the seed is chosen on the CPU with the oracle so that hits and misses both occur (a single ray can only be one of them)
    for seed in range(100, 140):
        O4, D4 = _box_rays(np.random.default_rng(seed), count)
        D4[:, 3] = np.random.default_rng(seed + 1000).uniform(0.0, 12.0, count).astype(np.float32)  # t_max on both sides of the distances
        ref = _oracle(oracle, oarr, n, O4, D4)
        if count == 1 or ((ref[0] >= 0).any() and (ref[0] < 0).any()):
            break
    hits, misses = _check(_trace(pt, O4, D4), ref, oarr, D4)  # the handle's own output buffers
    assert hits + misses == count and (count == 1 or (hits > 0 and misses > 0))
    # bound buffers, longer than the batch and pre-filled: nothing past element count - 1 is written
    t = _sentinels(count + 70)
    try:
        for k in NAMES:
            pt.bind_ray_output(k, t[k])
        pt.trace_rays()
        pt.wait()
        got = {k: t[k].cpu().numpy() for k in NAMES}
        _check(got, ref, oarr, D4)
        for k in NAMES:
            assert _untouched(t[k][count:]), k
            assert np.array_equal(pt.ray_output(k).view(np.uint32), got[k][:count].view(np.uint32)), k  # the read follows the binding
    finally:
        _unbind(pt)
    # repeated calls give the same bits
    again = _trace(pt, O4, D4)
    assert all(np.array_equal(again[k].view(np.uint32), got[k][:count].view(np.uint32)) for k in NAMES)


# ---- camera rays ------------------------------------------------------------------------------------------------------------
def test_camera_rays_equal_the_gbuffer(srt, oracle):
    w, h = 64, 36
    pt, oarr, n, _ = _tracer(srt, oracle, _scene1(oracle), w=w, h=h)
    pt.set_camera(srt.default_camera())
    pt.render_gbuffer()
    cam = oracle.default_camera()
    L = oracle.lib()
    d = (C.c_float * 3)()
    D = np.zeros((h, w, 3), np.float32)
    for y in range(h):
        for x in range(w):
            L.srt_oracle_ray_direction(C.byref(cam), w, h, x, y, d)
            D[y, x] = d[:]
    O4, D4 = _rays(np.tile(np.array(cam.position[:], np.float32), (w * h, 1)), D.reshape(-1, 3))
    g = _trace(pt, O4, D4)
    for k in NAMES[:4]:
        assert np.array_equal(g[k].view(np.uint32).reshape(-1), pt.gbuffer(k).view(np.uint32).reshape(-1)), k
    assert (g["object"] >= 0).any() and (g["object"] < 0).any()
    pt.close()


# ---- edges srt_render itself produces ---------------------------------------------------------------------------------------
def _edge_scene(oracle, swap=False):
    """A sphere, a box, and two pairs of coincident objects (exact distance ties), the pairs in either list order."""
    pair_s = [dict(type=oracle.OBJ_SPHERE, position=(-3.0, 0.0, 5.0), radius=1.0, base=(0.9, 0.1, 0.1)),
              dict(type=oracle.OBJ_SPHERE, position=(-3.0, 0.0, 5.0), radius=1.0, base=(0.1, 0.9, 0.1))]
    pair_b = [dict(type=oracle.OBJ_BOX, position=(0.0, 3.0, 5.0), half_size=(1.0, 0.5, 1.0), base=(0.1, 0.1, 0.9)),
              dict(type=oracle.OBJ_BOX, position=(0.0, 3.0, 5.0), half_size=(1.0, 0.5, 1.0), base=(0.9, 0.9, 0.1))]
    if swap:
        pair_s.reverse(), pair_b.reverse()
    return ([dict(type=oracle.OBJ_SPHERE, position=(0.0, 0.0, 5.0), radius=1.0, base=(0.8, 0.8, 0.8)), pair_s[0],
             dict(type=oracle.OBJ_BOX, position=(3.0, 0.0, 5.0), half_size=(1.0, 1.0, 1.0), base=(0.2, 0.6, 0.7)), pair_b[0], pair_s[1], pair_b[1]])


@pytest.mark.parametrize("swap", [False, True])
def test_edge_rays_and_exact_ties_in_both_list_orders(srt, oracle, swap):
    objs = _edge_scene(oracle, swap)
    pt, oarr, n, _ = _tracer(srt, oracle, objs)
    rng = np.random.default_rng(5)
    o, d = [], []
    # directions with one and two zero or -0.0 components, from outside the objects
    z, mz = 0.0, -0.0
    for dirs in ([z, z, 1.0], [mz, z, 1.0], [z, mz, 1.0], [mz, mz, 1.0], [0.6, z, 0.8], [0.6, mz, 0.8], [z, -0.6, 0.8], [mz, 0.6, 0.8], [-0.6, z, 0.8]):
        for org in ([0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [-3.0, 0.0, 0.0], [0.0, 3.0, 0.0], [0.25, 0.5, -1.0], [3.5, -0.25, 1.0]):
            o.append(org), d.append(dirs)
    for dirs in ([1.0, z, z], [1.0, mz, z], [1.0, mz, mz], [-1.0, z, mz]):  # along x through the spheres and the box
        for org in ([-10.0, 0.0, 5.0], [10.0, 0.0, 5.0], [-10.0, 0.5, 5.25]):
            o.append(org), d.append(dirs)
    for dirs in ([z, 1.0, z], [mz, -1.0, z]):  # along y through the sphere and the coincident boxes
        for org in ([0.0, -10.0, 5.0], [0.0, 10.0, 5.0], [0.5, 10.0, 4.5]):
            o.append(org), d.append(dirs)
    # origins inside a sphere, inside a box, inside the coincident pairs
    for org in ([0.0, 0.0, 5.0], [0.3, -0.2, 5.4], [3.0, 0.0, 5.0], [3.4, 0.7, 4.2], [-3.0, 0.0, 5.0], [-2.5, 0.2, 5.1], [0.0, 3.0, 5.0], [0.5, 3.2, 4.6]):
        for dirs in _unit(rng.normal(size=(6, 3))):
            o.append(org), d.append(list(dirs))
        o.append(org), d.append([z, z, 1.0])
    # random rays aimed at the pairs: exact ties between two coincident objects
    for c in ([-3.0, 0.0, 5.0], [0.0, 3.0, 5.0]):
        for _ in range(40):
            org = rng.uniform(-6, 6, 3) + [0, 0, -6]
            o.append(list(org)), d.append(list(_unit(np.array(c) + rng.uniform(-0.9, 0.9, 3) - org)[0]))
    O4, D4 = _rays(o, d)
    ref = _oracle(oracle, oarr, n, O4, D4)
    g = _trace(pt, O4, D4)
    hits, misses = _check(g, ref, oarr, D4)
    assert hits > 100 and misses > 10
    # the earlier list entry keeps a tie: the later twin of a pair is never reported
    assert set(np.unique(g["object"])) == {-1, 0, 1, 2, 3}
    # origins exactly on a surface, taken from the POSITION output: onward, back, and random directions
    on = g["position"][g["object"] >= 0][:, :3]
    dn = D4[g["object"] >= 0][:, :3]
    o2 = np.concatenate([on, on, on])
    d2 = np.concatenate([dn, -dn, _unit(rng.normal(size=(len(on), 3)))])
    O4, D4 = _rays(o2, d2)
    hits, misses = _check(_trace(pt, O4, D4), _oracle(oracle, oarr, n, O4, D4), oarr, D4)
    assert hits > 100 and misses > 10
    pt.close()


def test_nan_directions_miss_and_other_lanes_are_unharmed(srt, oracle, scene1):
    pt, oarr, n = scene1
    O4, D4 = _box_rays(np.random.default_rng(11), 130)
    nan = float("nan")
    bad = {0: (nan, 0.0, 1.0), 5: (0.0, nan, 1.0), 64: (0.6, 0.8, nan), 129: (nan, nan, nan)}
    for i, v in bad.items():
        D4[i, :3] = v
    g = _trace(pt, O4, D4)
    for i in bad:
        assert g["object"][i] == -1 and g["occluded"][i] == 0 and np.array_equal(g["normal_depth"][i].view(np.uint32), MISS_ND), i
        assert not g["position"][i].view(np.uint32).any() and not g["albedo"][i].view(np.uint32).any(), i
    rest = np.array([i for i in range(130) if i not in bad])
    _check({k: g[k][rest] for k in NAMES}, _oracle(oracle, oarr, n, O4[rest], D4[rest]), oarr, D4[rest])


@pytest.mark.parametrize("scale", [0.5, 3.0])
def test_directions_that_are_not_unit_length_in_analytic_scenes(srt, oracle, scene1, scale):
    pt, oarr, n = scene1  # 64 clustered spheres: the brute-force branch of the cluster phase runs
    rng = np.random.default_rng(21)
    O4, D4 = _box_rays(rng, 300)
    # Sphere::Raytrace tests the point o + d * |dot(c - o, d)| against the radius: with |d| = s that point lies s * s times as
    # far along the ray as the foot of the perpendicular, so at s = 3 only origins inside a sphere can hit.  Half the origins
    # are therefore put near the centres of Scene1's spheres; the oracle counts 214 / 86 hits / misses at 0.5, 73 / 227 at 3.
    centre = np.array([oarr[i].position[:] for i in range(n)], np.float32)
    radius = np.array([oarr[i].radius for i in range(n)], np.float32)
    pick = rng.integers(0, n, 150)
    O4[150:, :3] = (centre[pick] + rng.uniform(-0.3, 0.3, (150, 3)) * radius[pick, None]).astype(np.float32)
    D4[:, :3] *= np.float32(scale)
    D4[:, 3] = 4.0
    hits, misses = _check(_trace(pt, O4, D4), _oracle(oracle, oarr, n, O4, D4), oarr, D4)
    assert hits > 30 and misses > 30
    # ... and with spheres and boxes, a mixed wave: every third direction is left at unit length
    pt2, oarr2, n2, _ = _tracer(srt, oracle, _edge_scene(oracle))
    rng = np.random.default_rng(22)
    org = rng.uniform(-6, 6, (200, 3)) + [0, 0, -4]
    dirs = _unit(rng.uniform(-3, 3, (200, 3)) + [0, 1, 5] - org)
    dirs[::3] *= np.float32(scale)
    O4, D4 = _rays(org, dirs, 9.0)
    hits, misses = _check(_trace(pt2, O4, D4), _oracle(oracle, oarr2, n2, O4, D4), oarr2, D4)
    assert hits > 30 and misses > 10
    pt2.close()


# ---- instantiations ---------------------------------------------------------------------------------------------------------
def test_memory_instantiation_with_a_sphere_of_infinite_radius(srt, oracle):
    objs = _scene1(oracle)
    objs.insert(3, dict(type=oracle.OBJ_SPHERE, position=(0.0, 0.0, 2e19), radius=float("inf"), base=(.9, .2, .1)))
    pt, oarr, n, _ = _tracer(srt, oracle, objs)
    O4, D4 = _box_rays(np.random.default_rng(31), 700)
    _check(_trace(pt, O4, D4), _oracle(oracle, oarr, n, O4, D4), oarr, D4)
    pt.close()


def _mesh_scene(oracle, stacks=16, slices=20):
    """Scene1 with its r = 1 ball at (0, 0, 5) replaced by a UV sphere of 2 * slices * (stacks - 1) triangles, and a box."""
    objs = _scene1(oracle)
    big = objs[64]
    objs[64] = dict(type=oracle.OBJ_MESH, position=big["position"], mesh=0, base=big["base"], emissive=big["emissive"],
                    smoothness=big["smoothness"], specular_amount=big["specular_amount"], specular=big["specular"])
    objs.append(dict(type=oracle.OBJ_BOX, position=(2.5, 0.0, 5.5), half_size=(0.5, 0.75, 0.5), base=(0.3, 0.5, 0.7)))
    V, T = oracle.uv_sphere(1.0, stacks, slices)
    assert len(T) == 2 * slices * (stacks - 1)
    return objs, [(V, T)]


def _aimed_rays(rng, n, centre, spread):
    """Origins in the box around Scene1, unit directions towards points within `spread` of `centre`."""
    org = rng.uniform((-5, -1, 0), (5, 4, 10), (n, 3))
    return _rays(org, _unit(np.asarray(centre) + rng.uniform(-spread, spread, (n, 3)) - org))


def test_mesh_scene_and_rays_that_start_on_the_mesh(srt, oracle):
    objs, meshes = _mesh_scene(oracle)
    assert len(meshes[0][1]) == 600
    pt, oarr, n, om = _tracer(srt, oracle, objs, meshes=meshes)
    rng = np.random.default_rng(41)
    O4a, D4a = _aimed_rays(rng, 500, (0.0, 0.0, 5.0), 1.3)
    O4b, D4b = _box_rays(rng, 300)
    O4, D4 = np.concatenate([O4a, O4b]), np.concatenate([D4a, D4b])
    D4[:, 3] = rng.uniform(0.0, 10.0, len(D4)).astype(np.float32)
    ref = _oracle(oracle, oarr, n, O4, D4, om)
    g = _trace(pt, O4, D4)
    hits, misses = _check(g, ref, oarr, D4)
    on_mesh = g["object"] == 64
    assert on_mesh.sum() > 150 and misses > 50 and ((g["object"] >= 0) & ~on_mesh).sum() > 50
    # rays starting on the mesh: at the hit points themselves and lifted off along the normal as a bounce is, outwards, inwards
    # and at random
    p, nrm = g["position"][on_mesh][:, :3], g["normal_depth"][on_mesh][:, :3]
    lifted = (p + nrm * np.float32(.00001)).astype(np.float32)
    rnd = _unit(rng.normal(size=(len(p), 3)))
    o2 = np.concatenate([p, p, lifted, lifted, p])
    d2 = np.concatenate([rnd, nrm, rnd, D4[on_mesh][:, :3], -nrm])
    O4, D4 = _rays(o2, d2)
    hits, misses = _check(_trace(pt, O4, D4), _oracle(oracle, oarr, n, O4, D4, om), oarr, D4)
    assert hits > 100 and misses > 100
    pt.close()


def test_a_mesh_of_five_triangles(srt, oracle):
    V = np.array([[0, 0, 0], [1, 0, 0], [0.4, 0.9, 0.2], [-0.7, 0.6, 0.1], [-0.9, -0.5, -0.2], [0.2, -1.0, 0.3], [1.0, -0.6, -0.1]], np.float32)
    T = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 5], [0, 5, 6]], np.uint32)
    objs = [dict(type=oracle.OBJ_SPHERE, position=(1.5, 0.0, 6.0), radius=0.75, base=(0.5, 0.6, 0.7)),
            dict(type=oracle.OBJ_MESH, position=(0.0, 0.5, 4.0), mesh=0, base=(0.9, 0.4, 0.2)),
            dict(type=oracle.OBJ_BOX, position=(-1.5, 0.0, 5.0), half_size=(0.5, 0.5, 0.5), base=(0.2, 0.9, 0.4))]
    pt, oarr, n, om = _tracer(srt, oracle, objs, meshes=[(V, T)])
    rng = np.random.default_rng(51)
    org = rng.uniform((-3, -2, -2), (3, 3, 9), (400, 3))
    O4, D4 = _rays(org, _unit(np.array([0.0, 0.5, 4.0]) + rng.uniform(-1.6, 1.6, (400, 3)) - org), 5.0)
    g = _trace(pt, O4, D4)
    hits, misses = _check(g, _oracle(oracle, oarr, n, O4, D4, om), oarr, D4)
    assert (g["object"] == 1).sum() > 40 and misses > 40
    pt.close()


# ---- SRT_RAYS_NORMALIZE -----------------------------------------------------------------------------------------------------
def test_normalize_flag_equals_float32_normalization(srt, oracle, scene1):
    pt, oarr, n = scene1
    rng = np.random.default_rng(61)
    k = 600
    org = rng.uniform((-5, -1, 0), (5, 4, 10), (k, 3))
    raw = (_unit(rng.normal(size=(k, 3))) * (10.0 ** rng.uniform(-3, 3, (k, 1))).astype(np.float32)).astype(np.float32)
    lens = np.linalg.norm(raw.astype(np.float64), axis=1)
    assert lens.min() < 3e-3 and lens.max() > 300
    O4, D4 = _rays(org, raw, 3.0)
    g = _trace(pt, O4, D4, normalize=True)
    On, Dn = _rays(org, _unit(raw), 3.0)
    hits, misses = _check(g, _oracle(oracle, oarr, n, On, Dn), oarr, Dn)
    assert hits > 60 and misses > 60
    # the flag is off by default: the same rays without it are the un-normalized rays' answers (exact for analytic objects)
    _check(_trace(pt, O4, D4), _oracle(oracle, oarr, n, O4, D4), oarr, D4)


# ---- OCCLUDED ---------------------------------------------------------------------------------------------------------------
def test_occluded_at_and_around_the_closest_distance(srt, oracle, scene1):
    pt, oarr, n = scene1
    O4, D4 = _box_rays(np.random.default_rng(71), 400)
    idx, _, _, dist = _oracle(oracle, oarr, n, O4, D4)
    hit = idx >= 0
    assert hit.sum() > 40 and (~hit).sum() > 40
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    cases = [(dist, np.zeros_like(idx)),                                  # t_max equal to the distance: not occluded
             (np.nextafter(dist, inf), hit.astype(np.int32)),             # one ulp above: occluded
             (np.nextafter(dist, -inf), np.zeros_like(idx)),              # one ulp below: not
             (np.full_like(dist, inf), hit.astype(np.int32)),             # +inf: every hit, no miss
             (np.full_like(dist, nan), np.zeros_like(idx)),               # NaN: never
             (np.full_like(dist, -inf), np.zeros_like(idx))]
    for tmax, want in cases:
        D4[:, 3] = tmax
        pt.write_rays(O4, D4)
        pt.trace_rays(outputs=["occluded", "object"])
        assert np.array_equal(pt.ray_output("object"), idx)
        assert np.array_equal(pt.ray_output("occluded"), want)
        assert not pt.ray_output("occluded")[~hit].any()


# ---- output mask ------------------------------------------------------------------------------------------------------------
def test_each_single_bit_writes_only_its_buffer(srt, oracle, scene1):
    pt, oarr, n = scene1
    count = 100
    O4, D4 = _box_rays(np.random.default_rng(81), count)
    D4[:, 3] = 5.0
    ref = _oracle(oracle, oarr, n, O4, D4)
    full = _trace(pt, O4, D4)
    _check(full, ref, oarr, D4)
    try:
        for name in NAMES:
            t = _sentinels(count)
            for k in NAMES:
                pt.bind_ray_output(k, t[k])
            pt.trace_rays(outputs=name)
            pt.wait()
            for k in NAMES:
                if k == name:
                    assert np.array_equal(t[k].cpu().numpy().view(np.uint32), full[k].view(np.uint32)), k
                    assert np.array_equal(pt.ray_output(k).view(np.uint32), full[k].view(np.uint32)), k
                else:
                    assert _untouched(t[k]), (name, k)
                    with pytest.raises(srt.SrtError) as e:  # not written by the last trace
                        pt.ray_output(k)
                    assert e.value.code == srt.capi.ERR_STATE, (name, k)
    finally:
        _unbind(pt)
    # the same through the handle's own buffers: a later trace of other outputs leaves an earlier output unreadable, not stale
    pt.trace_rays(outputs=["position", "occluded"])
    assert np.array_equal(pt.ray_output("position").view(np.uint32), full["position"].view(np.uint32))
    with pytest.raises(srt.SrtError) as e:
        pt.ray_output("object")
    assert e.value.code == srt.capi.ERR_STATE


# ---- binding ----------------------------------------------------------------------------------------------------------------
def test_origins_bound_to_the_position_gbuffer_on_a_torch_stream(srt, oracle):
    import torch

    w, h = 64, 36
    pt, oarr, n, _ = _tracer(srt, oracle, _scene1(oracle), w=w, h=h)
    pt.set_camera(srt.default_camera())
    stream = torch.cuda.Stream(device=0)
    pos = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    nd = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    # directions: towards the sun of the default environment (a shadow ray per pixel), t_max = +inf
    sun = _unit(np.array([[-1.0, 1.0, 1.0]]))[0]
    D4 = np.zeros((w * h, 4), np.float32)
    D4[:, :3], D4[:, 3] = sun, np.inf
    dirs = torch.from_numpy(D4).to("cuda:0")
    out = {k: torch.empty((w * h,) if k in ("object", "occluded") else (w * h, 4), dtype=torch.int32 if k in ("object", "occluded") else torch.float32,
                          device="cuda:0") for k in NAMES}
    torch.cuda.synchronize()
    pt.set_stream(stream.cuda_stream)
    pt.bind_gbuffer("position", pos)
    pt.bind_gbuffer("normal_depth", nd)
    pt.render_gbuffer(outputs=["position", "normal_depth"])
    pt.bind_rays(pos.view(-1, 4), dirs)  # the handle's SRT_GBUF_POSITION device buffer as it stands: (point, 1), misses (0, 0, 0, 0)
    for k in NAMES:
        pt.bind_ray_output(k, out[k])
    pt.trace_rays()  # enqueued behind the G-buffer pass on the caller's stream; nothing has waited so far
    stream.synchronize()
    O4 = pos.cpu().numpy().reshape(-1, 4)
    g = {k: out[k].cpu().numpy() for k in NAMES}
    hits, misses = _check(g, _oracle(oracle, oarr, n, O4, D4), oarr, D4)
    assert hits > 50 and misses > 50 and (O4[:, 3] == 1.0).sum() > 500
    # back to the handle's own rays: none have been written yet
    pt.bind_rays(None, None)
    with pytest.raises(srt.SrtError) as e:
        pt.trace_rays()
    assert e.value.code == srt.capi.ERR_STATE
    # tensors that cannot be bound are refused before the library is touched
    for bad in (torch.empty((10, 3), dtype=torch.float32, device="cuda:0"), torch.empty((10, 4), dtype=torch.float64, device="cuda:0"),
                torch.empty((10, 8), dtype=torch.float32, device="cuda:0")[:, ::2]):
        with pytest.raises((TypeError, ValueError)):
            pt.bind_rays(bad, dirs[:10])
    with pytest.raises((TypeError, ValueError)):
        pt.bind_ray_output("object", torch.empty((10,), dtype=torch.float32, device="cuda:0"))
    with pytest.raises((TypeError, ValueError)):
        pt.bind_ray_output("albedo", torch.empty((10, 3), dtype=torch.float32, device="cuda:0"))
    pt.set_stream(0)
    pt.close()


# ---- order ------------------------------------------------------------------------------------------------------------------
def test_traces_before_and_after_a_refit_see_their_own_scene(srt, oracle):
    objs, meshes = _mesh_scene(oracle)
    pt, oarr, n, om = _tracer(srt, oracle, objs, meshes=meshes, refit=True)
    O4, D4 = _aimed_rays(np.random.default_rng(91), 400, (0.3, 0.2, 5.0), 1.5)
    moved = [dict(o) for o in objs]
    moved[64]["position"] = (0.6, 0.35, 5.2)
    oarr2, n2 = oracle.make_objects(moved)
    first, second = _sentinels(400), _sentinels(400)
    pt.write_rays(O4, D4)
    for k in NAMES:
        pt.bind_ray_output(k, first[k])
    pt.trace_rays()
    pt.update_scene(C.cast(oarr2, C.POINTER(srt.Object)), n2)
    for k in NAMES:
        pt.bind_ray_output(k, second[k])
    pt.trace_rays()
    pt.wait()
    assert pt.update_info()["path"] == 2
    a, b = ({k: t[k].cpu().numpy() for k in NAMES} for t in (first, second))
    _check(a, _oracle(oracle, oarr, n, O4, D4, om), oarr, D4)
    _check(b, _oracle(oracle, oarr2, n2, O4, D4, om), oarr2, D4)
    assert (a["object"] != b["object"]).sum() > 20
    pt.close()


# ---- left alone -------------------------------------------------------------------------------------------------------------
def test_a_trace_leaves_renders_gbuffer_and_stats_alone(srt, oracle):
    w, h = 160, 96
    objs = _scene1(oracle)
    fields = ("rays", "sample_chunks", "tile_rows", "chunk_samples", "shape_source", "path_samples")
    O4, D4 = _box_rays(np.random.default_rng(95), 3000)
    runs = []
    for with_trace in (False, True):
        pt, oarr, n, _ = _tracer(srt, oracle, objs, w=w, h=h)
        pt.set_camera(srt.default_camera())
        pt.render(spp=8, bounces=3, seed=5, count_rays=True, count_work=True)
        pt.render_gbuffer()
        before = (pt.accumulator(), pt.framebuffer(), {k: pt.gbuffer(k) for k in NAMES[:4]}, pt.stats(), pt.work_counts().as_dict())
        if with_trace:
            pt.write_rays(O4, D4)
            pt.trace_rays()
            pt.wait()
            after = (pt.accumulator(), pt.framebuffer(), {k: pt.gbuffer(k) for k in NAMES[:4]}, pt.stats(), pt.work_counts().as_dict())
            assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)) and np.array_equal(before[1], after[1])
            assert all(np.array_equal(before[2][k].view(np.uint32), after[2][k].view(np.uint32)) for k in NAMES[:4])
            assert all(getattr(before[3], f) == getattr(after[3], f) for f in fields) and before[3].kernel_ms == after[3].kernel_ms
            assert before[4] == after[4]
            assert (pt.ray_output("object") >= 0).any()
        pt.render(spp=8, first_sample=9, reset=False, bounces=3, seed=5, count_rays=True, count_work=True)
        st = pt.stats()
        runs.append(([getattr(st, f) for f in fields], pt.work_counts().as_dict(), pt.framebuffer(), pt.accumulator()))
        pt.close()
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1]
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32))


# ---- errors -----------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_previous_rays_and_outputs_intact(srt, oracle):
    c = srt.capi
    fresh = srt.PathTracer(16, 16)
    O4, D4 = _box_rays(np.random.default_rng(97), 90)
    fresh.write_rays(O4, D4)
    with pytest.raises(srt.SrtError) as e:  # before srt_set_scene
        fresh.trace_rays()
    assert e.value.code == c.ERR_STATE and "srt_set_scene" in str(e.value)
    oarr, n = oracle.make_objects(_scene1(oracle))
    pt = srt.PathTracer(16, 16)
    pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
    with pytest.raises(srt.SrtError) as e:  # no rays written or bound
        pt.trace_rays()
    assert e.value.code == c.ERR_STATE
    assert pt.L.srt_read_ray_output(pt._h, 1, O4.ctypes.data_as(C.c_void_p)) == c.ERR_STATE  # no trace yet
    good = _trace(pt, O4, D4)
    ref = _oracle(oracle, oarr, n, O4, D4)
    _check(good, ref, oarr, D4)

    def intact():
        for k in NAMES:  # the outputs of the last good trace are still readable ...
            assert np.array_equal(pt.ray_output(k).view(np.uint32), good[k].view(np.uint32)), k
        pt.trace_rays()  # ... and the previous rays are still the current ones
        for k in NAMES:
            assert np.array_equal(pt.ray_output(k).view(np.uint32), good[k].view(np.uint32)), k

    for kw in (dict(outputs=0), dict(outputs=32), dict(outputs=31 | 64), dict(flags=2), dict(flags=0x80000000), dict(outputs=0, flags=4)):
        with pytest.raises(srt.SrtError) as e:
            pt.trace_rays(**kw)
        assert e.value.code == c.ERR_INVALID_ARG, kw
        intact()
    f = C.POINTER(C.c_float)
    po, pd = O4.ctypes.data_as(f), D4.ctypes.data_as(f)
    for count in (0, 2 ** 30 + 1, 2 ** 40):  # refused on the count alone: the arrays are not read
        assert pt.L.srt_write_rays(pt._h, po, pd, count) == c.ERR_INVALID_ARG, count
        assert pt.L.srt_bind_rays(pt._h, C.c_void_p(4096), C.c_void_p(8192), count) == c.ERR_INVALID_ARG, count
        intact()
    assert pt.L.srt_write_rays(pt._h, None, pd, 5) == c.ERR_INVALID_ARG and pt.L.srt_write_rays(pt._h, po, None, 5) == c.ERR_INVALID_ARG
    assert pt.L.srt_bind_rays(pt._h, None, C.c_void_p(8192), 5) == c.ERR_INVALID_ARG and pt.L.srt_bind_rays(pt._h, C.c_void_p(4096), None, 5) == c.ERR_INVALID_ARG
    intact()
    for bit in (0, 3, 32, 48):
        assert pt.L.srt_bind_ray_output(pt._h, bit, None) == c.ERR_INVALID_ARG
        assert pt.L.srt_read_ray_output(pt._h, bit, O4.ctypes.data_as(C.c_void_p)) == c.ERR_INVALID_ARG
    assert pt.L.srt_read_ray_output(pt._h, 1, None) == c.ERR_INVALID_ARG and pt.L.srt_trace_rays(pt._h, None) == c.ERR_INVALID_ARG
    intact()
    fresh.close()
    pt.close()


# ---- layers -----------------------------------------------------------------------------------------------------------------
def test_host_library_host_py_and_cli_give_the_bytes_of_the_c_calls(srt, oracle, tmp_path):
    rng = np.random.default_rng(99)
    k = 150
    org = rng.uniform((-5, -1, 0), (5, 4, 10), (k, 3))
    O4, D4 = _rays(org, (_unit(rng.normal(size=(k, 3))) * rng.uniform(0.5, 2.0, (k, 1))).astype(np.float32), 6.0)
    oarr, n = oracle.make_objects(_scene1(oracle))
    blobs = {}
    for normalize in (False, True):
        pt = srt.PathTracer(16, 16)
        pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
        want = _trace(pt, O4, D4, normalize=normalize)
        pt.close()
        assert (want["object"] >= 0).any() and (want["object"] < 0).any()
        blobs[normalize] = b"".join(want[name].tobytes() for name in NAMES)
        # host.py over the C++ host's PathTraceRenderer::traceRays
        r = srt.host.Renderer(32, 24)
        scene = srt.host.Scene(scene_path("Scene1"))
        r.set_scene(scene)
        r.trace_rays(O4, D4, normalize=normalize)
        assert b"".join(r.ray_output(name).tobytes() for name in NAMES) == blobs[normalize]
        r.close()
        # the command-line tool
        rays, out = tmp_path / "in.f32", tmp_path / ("out%d.bin" % normalize)
        np.concatenate([O4, D4], axis=1).astype(np.float32).tofile(str(rays))
        run = subprocess.run([CLI, "--scene", scene_path("Scene1"), "--rays", str(rays), "--rays-out", str(out)] + (["--rays-normalize"] if normalize else []),
                             capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr[-2000:]
        assert out.read_bytes() == blobs[normalize]
    assert blobs[False] != blobs[True]
