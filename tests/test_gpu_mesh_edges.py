"""The mesh BVH and its traversal (phase 4 of closest_hit) on adversarial geometry: every conservative filter between a ray and
its triangle — the per-ray pad, the root-box test on unclamped reciprocals, the bounding-sphere cull, the t >= 0.0099 and
tmin <= 10001 culls, the order of exact ties, queue overflow and the strict last resort — against the brute-force oracle, bit
for bit, NaNs as NaNs.  (What the tie cases pin is the order of the 64-bit atomicMin key, (distance, global triangle id), and the
list-index comparison against the best analytic hit.  The cull of a box against the current best cannot lose a tie whether it
compares with < or <=: the per-ray pad and the slack of the comparison put a box's entry distance strictly below every hit
inside it, so making that cull strict changes no result.)

Every case is checked twice: srt_render_gbuffer against srt_oracle_closest_m at EVERY pixel (a failure names the pixel and its
ray) with srt_pick at a sample of pixels, and srt_render against oracle.render on rays, accumulator and framebuffer with
>= 2 samples and >= 4 bounces, so that bounce rays start on the mesh.  Conditions that keep a case from passing emptily are
asserted on oracle output only: a mesh triangle is the first hit on >= 10 % of the pixels, a miss or an analytic object on >= 5 %.

Not tested, on grounds of memory: the limit of 2^24 - 1 triangles of ONE mesh (srt_set_meshes; its index array alone is
200 MB) and of 2^26 - 1 BVH nodes (more nodes than 2^24 triangles can make).  The scene total of 2^24 - 1 is tested with
triangles whose indices are out of range (counted by the limit, dropped by the build).  The depth limit of 61 levels cannot be
reached by a mesh of testable size (the builder makes at most 40 + log2(triangles / 4) levels); tests/native/builders_check.cpp
asserts it for every mesh it builds."""
import ctypes as C
import itertools

import numpy as np
import pytest

from test_gpu_fuzz import _same_bits

pytestmark = pytest.mark.gpu

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
def _camera(oracle, pos, forward=(0, 0, 1), up=(0, 1, 0), fov=55, right=None):
    f, u = np.asarray(forward, np.float64), np.asarray(up, np.float64)
    r = np.cross(u, f) if right is None else np.asarray(right, np.float64)
    cam = oracle.Camera()
    cam.position, cam.right, cam.up, cam.forward, cam.fov_degrees = oracle.f3(pos), oracle.f3(r), oracle.f3(u), oracle.f3(f), fov
    return cam


def _rays(oracle, cam, w, h):
    d, out = (C.c_float * 3)(), np.empty((h, w, 3), F32)
    for y in range(h):
        for x in range(w):
            oracle.lib().srt_oracle_ray_direction(C.byref(cam), w, h, x, y, d)
            out[y, x] = d[:]
    return out


def _oracle_first_hits(oracle, oarr, n, marr, mn, cam, rays):
    h, w, _ = rays.shape
    L = oracle.lib()
    nn, pp, t, d = (C.c_float * 3)(), (C.c_float * 3)(), C.c_float(), (C.c_float * 3)()
    origin = (C.c_float * 3)(*cam.position)
    idx = np.full((h, w), -1, np.int32)
    nd, pos = np.zeros((h, w, 4), F32), np.zeros((h, w, 4), F32)
    nd[..., 3] = np.inf
    for y in range(h):
        for x in range(w):
            d[:] = [float(v) for v in rays[y, x]]
            i = L.srt_oracle_closest_m(oarr, n, marr, mn, origin, d, nn, pp, C.byref(t))
            idx[y, x] = i
            if i >= 0:
                nd[y, x] = [nn[0], nn[1], nn[2], t.value]
                pos[y, x] = [pp[0], pp[1], pp[2], 1.0]
    return idx, nd, pos


def _world_triangles(objs, meshes):
    """(v0, e1, e2) float32 [k, 3] of every valid triangle in (list index, triangle index) order, as srt_pathtrace.h defines them"""
    v0, e1, e2 = [], [], []
    for o in objs:
        if o.get("type") != 3 or not 0 <= o.get("mesh", -1) < len(meshes):
            continue
        V, T = meshes[o["mesh"]]
        V, T = np.asarray(V, F32).reshape(-1, 3), np.asarray(T, np.int64).reshape(-1, 3)
        T = T[(T < len(V)).all(1)]
        W = V + np.asarray(o.get("position", (0, 0, 0)), F32)
        a, b, c = W[T[:, 0]], W[T[:, 1]], W[T[:, 2]]
        ok = np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1)
        v0.append(a[ok]), e1.append((b - a)[ok]), e2.append((c - a)[ok])
    return np.concatenate(v0), np.concatenate(e1), np.concatenate(e2)


def _triangle_distances(v0, e1, e2, o, d):
    """The oracle's triangle_raytrace for one ray against all triangles: binary32, no FMA, its operation order.  Distance of the
    valid hits, inf elsewhere.  (Cross-checked against the oracle's own answer wherever it is used.)"""
    o, d = np.asarray(o, F32), np.asarray(d, F32)
    cross = lambda a, b: np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                                   a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    with np.errstate(all="ignore"):
        pv = cross(np.broadcast_to(d, e2.shape), e2)
        det = dot(e1, pv)
        inv = F32(1.0) / det
        tv = o - v0
        u = dot(tv, pv) * inv
        qv = cross(tv, e1)
        v = dot(np.broadcast_to(d, qv.shape), qv) * inv
        t = dot(e2, qv) * inv
        ok = (np.abs(det) >= F32(1e-12)) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= F32(1.0)) & (t >= F32(0.01)) & (t <= F32(10000.0))
    return np.where(ok, t, F32(np.inf)).astype(F32)


def _count_ties(oracle, objs, meshes, cam, rays, idx, nd, stride=1):
    """pixels whose closest triangle distance is reached by two or more triangles, bit for bit"""
    v0, e1, e2 = _world_triangles(objs, meshes)
    ties = 0
    h, w, _ = rays.shape
    for y in range(0, h, stride):
        for x in range(0, w, stride):
            t = _triangle_distances(v0, e1, e2, cam.position[:], rays[y, x])
            m = t.min()
            if np.isfinite(m):
                if idx[y, x] >= 0 and objs[idx[y, x]].get("type") == 3:
                    assert m == nd[y, x, 3], (x, y, m, nd[y, x, 3])  # the emulation is the oracle's arithmetic
                ties += int((t == m).sum() >= 2)
    return ties


class Case:
    def __init__(self, objs, meshes, cam, w=64, h=48, spp=2, bounces=4, seed=3, min_mesh=0.10, min_other=0.05, note=""):
        self.objs, self.meshes, self.cam, self.w, self.h, self.spp, self.bounces, self.seed = objs, meshes, cam, w, h, spp, bounces, seed
        self.min_mesh, self.min_other, self.note = min_mesh, min_other, note


def _tracer(srt, oracle, case):
    oarr, n = oracle.make_objects(case.objs)
    marr, mn, keep = oracle.make_meshes(case.meshes)
    pt = srt.PathTracer(case.w, case.h)
    pt.set_meshes(C.cast(marr, C.POINTER(srt.Mesh)), mn)
    pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
    pt.set_camera(srt.Camera.from_buffer_copy(bytes(case.cam)))
    return pt, oarr, n, marr, mn, keep


def _check_first_hits(pt, oracle, case, oarr, n, marr, mn):
    """srt_render_gbuffer vs srt_oracle_closest_m at every pixel; srt_pick on a sample.  Returns the oracle's buffers."""
    w, h = case.w, case.h
    rays = _rays(oracle, case.cam, w, h)
    idx, nd, pos = _oracle_first_hits(oracle, oarr, n, marr, mn, case.cam, rays)
    is_mesh = np.array([o.get("type") == 3 for o in case.objs] + [False])[idx]  # (-1 -> the appended False)
    share = float(is_mesh.mean())
    print("%s: mesh first hits %.1f %%, other %.1f %%" % (case.note, 100 * share, 100 * (1 - share)))
    assert share >= case.min_mesh and 1 - share >= case.min_other, (case.note, share)
    pt.render_gbuffer()
    g_idx, g_nd, g_pos = pt.gbuffer("object"), pt.gbuffer("normal_depth"), pt.gbuffer("position")
    bad = (g_idx != idx) | ~_same_bits(g_nd, nd) | ~_same_bits(g_pos, pos)
    if bad.any():
        y, x = [int(v[0]) for v in np.nonzero(bad)]
        raise AssertionError("%s: %d pixels differ; first (x=%d, y=%d): origin %r direction %r (%s): HIP object %d normal/depth %r, "
                             "oracle object %d normal/depth %r" % (case.note, int(bad.sum()), x, y, list(case.cam.position), rays[y, x].tolist(),
                                                                   [hex(v) for v in rays[y, x].view(np.uint32)], g_idx[y, x], g_nd[y, x].tolist(),
                                                                   idx[y, x], nd[y, x].tolist()))
    for y in range(1, h, max(1, h // 7)):
        for x in range(2, w, max(1, w // 9)):
            assert pt.pick(x, y) == idx[y, x], (case.note, x, y)
    return rays, idx, nd


def _check_paths(pt, oracle, case, oarr, n, marr, mn, spp=None, resume=False):
    import torch

    w, h = case.w, case.h
    kw = dict(spp=spp or case.spp, bounces=case.bounces, seed=case.seed)
    env = oracle.default_environment()
    if resume:  # continue a frame in a caller's accumulator
        rng = np.random.default_rng(case.seed)
        acc0 = rng.uniform(0, 2, (h, w, 4)).astype(F32)
        acc0[..., 3] = 0
        t = torch.from_numpy(acc0).to("cuda:0")
        torch.cuda.synchronize()
        pt.bind_output(d_accumulator=t.data_ptr())
        kw.update(first_sample=7, reset=False)
        pt.render(count_rays=True, **kw)
        pt.wait()
        gacc, gfb, grays = t.cpu().numpy(), pt.framebuffer(), pt.stats().rays
        pt.bind_output()
        ofb, oacc, orays = oracle.render(oarr, n, env, case.cam, w, h, meshes=(marr, mn), accumulator=acc0, **kw)
    else:
        pt.render(count_rays=True, **kw)
        gacc, gfb, grays = pt.accumulator(), pt.framebuffer(), pt.stats().rays
        ofb, oacc, orays = oracle.render(oarr, n, env, case.cam, w, h, meshes=(marr, mn), **kw)
    assert grays == orays, (case.note, kw, grays, orays)
    same = _same_bits(gacc, oacc)
    assert same.all(), (case.note, kw, int((~same).sum()), [int(v[0]) for v in np.nonzero(~same)][::-1])
    assert np.array_equal(gfb, ofb), (case.note, kw)


def _check(srt, oracle, case, chunks=False, resume=False, ties=0, tie_stride=1):
    pt, oarr, n, marr, mn, keep = _tracer(srt, oracle, case)
    rays, idx, nd = _check_first_hits(pt, oracle, case, oarr, n, marr, mn)
    if ties:
        count = _count_ties(oracle, case.objs, case.meshes, case.cam, rays, idx, nd, tie_stride)
        print("%s: %d pixels with an exact cross-triangle tie" % (case.note, count))
        assert count >= ties, (case.note, count)
    _check_paths(pt, oracle, case, oarr, n, marr, mn)
    if chunks:  # >= 32 samples with meshes (chunks=True), >= 64 without a triangle: sample chunks + fold_kernel
        _check_paths(pt, oracle, case, oarr, n, marr, mn, spp=33 if chunks is True else chunks)
        assert pt.stats().sample_chunks > 1
    if resume:
        _check_paths(pt, oracle, case, oarr, n, marr, mn, resume=True)
    pt.close()
    return rays, idx, nd


# ---------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------
def _grid(n, axis, c, step, flip=False, centre=(0.0, 0.0)):
    """n x n quads of side `step` (a binary fraction) lying exactly in the plane coordinate[axis] = c"""
    u, v = (axis + 1) % 3, (axis + 2) % 3
    V = np.zeros(((n + 1) * (n + 1), 3), F32)
    j, i = np.mgrid[0:n + 1, 0:n + 1]
    V[:, axis], V[:, u], V[:, v] = c, (centre[0] + (i - n / 2) * step).ravel(), (centre[1] + (j - n / 2) * step).ravel()
    T = []
    for j in range(n):
        for i in range(n):
            a, b, d, e = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i, (j + 1) * (n + 1) + i + 1
            T += [(a, b, d), (b, e, d)] if flip else [(a, b, e), (a, e, d)]
    return V, np.array(T, np.uint32)


CUBE_V = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], F32)
CUBE_T = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [2, 3, 7], [2, 7, 6], [1, 2, 6], [1, 6, 5], [0, 4, 7], [0, 7, 3]], np.uint32)


def _mesh(oracle, mesh, position=(0, 0, 0), base=(0.8, 0.7, 0.6), **kw):
    return dict(type=oracle.OBJ_MESH, mesh=mesh, position=tuple(float(v) for v in position), base=base, **kw)


def _sphere(oracle, position, radius, base=(0.3, 0.6, 0.9), **kw):
    return dict(type=oracle.OBJ_SPHERE, position=tuple(float(v) for v in position), radius=float(radius), base=base, **kw)


def _box(oracle, position, half, base=(0.9, 0.4, 0.3), **kw):
    return dict(type=oracle.OBJ_BOX, position=tuple(float(v) for v in position), half_size=tuple(float(v) for v in half), base=base, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# 1. axis-aligned flat meshes: the root test on unclamped reciprocals, 0 * inf, zero-extent cells
# ---------------------------------------------------------------------------------------------------------------------
def _flat_scene(oracle):
    """three flat grids: a back wall in z = 6, a floor in y = -1.5, a side wall in x = -2.5; a sphere, a box"""
    meshes = [_grid(8, 2, 6.0, 0.75), _grid(8, 1, -1.5, 0.75, centre=(3.0, 0.0)), _grid(8, 0, -2.5, 0.75, centre=(0.0, 3.0))]
    objs = [_mesh(oracle, 0, base=(0.8, 0.3, 0.3)), _mesh(oracle, 1, base=(0.7, 0.7, 0.7), smoothness=0.9, specular_amount=0.6),
            _mesh(oracle, 2, base=(0.3, 0.8, 0.3), emissive=(0.4, 0.4, 0.2)), _sphere(oracle, (1.0, -0.75, 4.0), 0.75, specular_amount=0.8, smoothness=0.95),
            _box(oracle, (-1.25, -1.0, 3.5), (0.5, 0.5, 0.5))]
    return objs, meshes


FLAT_CAMERAS = {
    # name: (position, forward, up, right or None for up x forward, must a whole pixel column or row have a zero component?).  The
    # frame is 64 x 48: pixel column 32 has nX = 0 and row 24 has nY = 0 exactly (GetRayDirection, Raytracer.cpp:109-110).
    "along z": ((0, 0, 0), (0, 0, 1), (0, 1, 0), None, True),
    # (a mirrored basis with a -0.0 in `forward`: the middle column's z component is -0.0 in the lower half of the frame)
    "along -x": ((2.5, 0, 3), (-1, 0, -0.0), (0, 1, 0), (0, 0, -1), True),
    "along -y": ((0, 4, 3), (0, -1, 0), (0, 0, 1), None, True),
    "in the floor's plane": ((0.25, -1.5, 0), (0, 0, 1), (0, 1, 0), None, True),
    "in the back wall's plane": ((2.75, 0.25, 6.0), (-1, 0, 0), (0, 1, 0), None, True),
    "on the floor's box plane x = 3": ((3.0, 0, 0.5), (-0.5, 0, 0.8660254037844386), (0, 1, 0), None, False),
    "on the wall's box plane z = 6": ((0.5, 0.5, 6.0), (-0.8, 0, -0.6), (0, 1, 0), None, False),
}


@pytest.mark.parametrize("name", list(FLAT_CAMERAS))
def test_axis_aligned_flat_meshes(srt, oracle, name):
    pos, fwd, up, right, zero = FLAT_CAMERAS[name]
    objs, meshes = _flat_scene(oracle)
    case = Case(objs, meshes, _camera(oracle, pos, fwd, up, right=right), w=64, h=48, note="flat, camera " + name)
    rays = _rays(oracle, case.cam, case.w, case.h)
    if zero:  # a whole pixel column or row whose rays have an exactly zero direction component (-0.0 counts: it is == 0)
        cols = [(rays[:, x, a] == 0).all() for x in range(case.w) for a in range(3)]
        rows = [(rays[y, :, a] == 0).all() for y in range(case.h) for a in range(3)]
        assert any(cols) or any(rows), name
        print(name, "zero-component columns", sum(cols), "rows", sum(rows), "negative zeros", int((np.signbit(rays) & (rays == 0)).sum()))
    _check(srt, oracle, case, chunks=name == "along z", resume=name == "along -x")


def test_flat_mesh_rays_include_negative_zero(oracle):
    """(no GPU needed, but it belongs to the cases above) the cameras above do produce -0.0 components"""
    seen = 0
    for pos, fwd, up, right, zero in FLAT_CAMERAS.values():
        rays = _rays(oracle, _camera(oracle, pos, fwd, up, right=right), 64, 48)
        seen += int((np.signbit(rays) & (rays == 0)).sum())
    assert seen > 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. exact ties across leaves: the <= best culls, the 64-bit atomicMin key, bord
# ---------------------------------------------------------------------------------------------------------------------
def _tie_backdrop(oracle):
    return [_sphere(oracle, (0.0, -1001.5, 5.0), 1000.0, base=(0.5, 0.5, 0.5)), _sphere(oracle, (1.9, 0.9, 3.0), 0.5, emissive=(1.0, 0.8, 0.3))]


def test_ties_same_grid_twice_with_opposite_diagonals(srt, oracle):
    meshes = [_grid(10, 2, 4.0, 0.25), _grid(10, 2, 4.0, 0.25, flip=True)]
    objs = _tie_backdrop(oracle)[:1] + [_mesh(oracle, 1, base=(0.2, 0.9, 0.2)), _mesh(oracle, 0, base=(0.9, 0.2, 0.2), emissive=(0.3, 0, 0))] + _tie_backdrop(oracle)[1:]
    _check(srt, oracle, Case(objs, meshes, oracle.default_camera(), note="ties: one grid, two diagonals"), ties=100, chunks=True)


def test_ties_each_triangle_nine_times_under_shuffled_indices(srt, oracle):
    V, T = _grid(9, 2, 4.0, 0.25)
    rng = np.random.default_rng(9)
    T9 = np.repeat(T, 9, axis=0)[rng.permutation(9 * len(T))]
    # the copies differ in nothing the traversal sees, so the lowest triangle index of a group is met in no particular order
    objs = [_mesh(oracle, 0, position=(0.25, 0.125, 0.0))] + _tie_backdrop(oracle)
    _check(srt, oracle, Case(objs, [(V, T9)], oracle.default_camera(), note="ties: nine copies of every triangle"), ties=100, resume=True)


@pytest.mark.parametrize("order", list(itertools.permutations(range(3))))
def test_ties_mesh_face_on_a_box_face_and_a_sphere_tangent_point(srt, oracle, order):
    """a cube mesh (every triangle twice) whose faces are those of a box, and a sphere that touches the front face from the
    camera's side — in every list order"""
    trio = [_mesh(oracle, 0, position=(0.0, 0.0, 4.0), base=(0.9, 0.2, 0.2)), _box(oracle, (0.0, 0.0, 4.0), (0.75, 0.75, 0.75), base=(0.2, 0.2, 0.9), emissive=(0, 0, 0.5)),
            _sphere(oracle, (0.25, 0.25, 3.0), 0.25, base=(0.2, 0.9, 0.2))]
    # (a mesh floor instead of the ground sphere: where the box comes first it wins every tie, and the cube alone is no tenth of the frame)
    objs = [_mesh(oracle, 1, base=(0.5, 0.5, 0.5))] + [trio[i] for i in order] + _tie_backdrop(oracle)[1:]
    meshes = [(CUBE_V * F32(0.75), np.concatenate([CUBE_T, CUBE_T[::-1]])), _grid(6, 1, -1.5, 2.0, centre=(5.0, 0.0))]
    _check(srt, oracle, Case(objs, meshes, oracle.default_camera(), note="ties: mesh / box / sphere order %r" % (order,)), ties=100)


# ---------------------------------------------------------------------------------------------------------------------
# 3. coarse quantization cells
# ---------------------------------------------------------------------------------------------------------------------
def test_coarse_cells_ground_and_fine_sphere_in_one_mesh(srt, oracle):
    V, T = oracle.uv_sphere(1.0, 32, 32)  # 1984 triangles
    G = np.array([[-2000, -1, -2000], [2000, -1, -2000], [2000, -1, 2000], [-2000, -1, 2000]], F32)
    mesh = (np.concatenate([G, V + F32([0.25, 0.0, 4.0])]), np.concatenate([np.array([[0, 2, 1], [0, 3, 2]], np.uint32), T + np.uint32(4)]))
    objs = [_mesh(oracle, 0, smoothness=0.8, specular_amount=0.3), _sphere(oracle, (-1.75, -0.5, 3.5), 0.5, emissive=(0.5, 0.5, 0.5)), _box(oracle, (2.0, -0.5, 5.0), (0.5, 0.5, 0.5))]
    _check(srt, oracle, Case(objs, [mesh], oracle.default_camera(), w=56, h=40, note="coarse: 4000-unit ground + sphere"), chunks=True)


def test_coarse_cells_overlapping_diagonal_slivers(srt, oracle):
    rng = np.random.default_rng(3)
    nt, L = 400, 8.0
    s = rng.uniform(-1.5, 1.5, (nt, 3)).astype(F32) * F32([1, 1, 0.25])
    V = np.zeros((3 * nt, 3), F32)
    V[0::3] = s
    V[1::3] = s + F32([L, L, L])
    V[2::3] = s + F32([0.2, -0.2, 0.0]) * F32(rng.uniform(0.0004, 1.0))  # from 1e5 : 1 up to slivers wide enough to be seen
    V[2:300:3] = s[:100] + F32([L * 1e-5, -L * 1e-5, 0.0])
    T = np.arange(3 * nt, dtype=np.uint32).reshape(nt, 3)
    objs = [_mesh(oracle, 0, position=(-4.0, -4.0, 1.0), emissive=(0.2, 0.1, 0.0)), _sphere(oracle, (0.0, -1001.5, 5.0), 1000.0), _sphere(oracle, (1.0, 0.0, 8.0), 1.0)]
    _check(srt, oracle, Case(objs, [(V, T)], oracle.default_camera(), note="coarse: diagonal slivers"), resume=True)


def test_coarse_cells_extent_ratio_one_million(srt, oracle):
    """a ground 4096 units wide whose heights span 1/256: the y cells are a million times finer than the x and z cells"""
    V, T = _grid(24, 1, -1.0, 4096.0 / 24)
    rng = np.random.default_rng(8)
    V[:, 1] += (rng.integers(0, 2, len(V)) / 256.0).astype(F32)
    assert (V[:, 0].max() - V[:, 0].min()) / (V[:, 1].max() - V[:, 1].min()) >= 1e6
    objs = [_mesh(oracle, 0, specular_amount=0.5, smoothness=0.9), _sphere(oracle, (0.5, 0.0, 5.0), 1.0, emissive=(0.4, 0.2, 0.1)), _box(oracle, (-2.0, 0.0, 6.0), (0.5, 1.0, 0.5))]
    _check(srt, oracle, Case(objs, [(V, T)], oracle.default_camera(), note="coarse: extent ratio 1e6"))


# ---------------------------------------------------------------------------------------------------------------------
# 4. magnitude sweep: the pad formula, r1, the tmin <= 10001 and t <= 10000 windows
# ---------------------------------------------------------------------------------------------------------------------
def _sweep_scene(oracle, origin, s, fov=55):
    """a tessellated ball, a cube mesh, spheres and a box 4 s to 7 s in front of a camera at `origin`, everything of size ~s"""
    depth = 6.0
    origin = np.asarray(origin, np.float64)
    at = lambda x, y, z: tuple(origin + s * np.array([x, y, z]))
    V, T = oracle.uv_sphere(1.0, 10, 14)
    meshes = [((V * s).astype(F32), T), ((CUBE_V * 0.5 * s).astype(F32), CUBE_T)]
    objs = [_sphere(oracle, at(-1.5, 0.5, depth), 0.5 * s, emissive=(0.6, 0.5, 0.2)), _mesh(oracle, 0, at(0.25, 0.0, depth), specular_amount=0.4, smoothness=0.9),
            _box(oracle, at(1.75, -0.5, depth - 1), (0.5 * s, 0.5 * s, 0.5 * s)), _mesh(oracle, 1, at(-0.75, -0.6, depth - 2), base=(0.3, 0.9, 0.4)),
            _sphere(oracle, at(0.0, -101.0, depth), 100.0 * s, base=(0.5, 0.5, 0.5)), _sphere(oracle, at(1.5, 1.0, depth + 1), 0.4 * s)]
    return objs, meshes, _camera(oracle, tuple(origin), fov=fov)


# (offset along the diagonal (1, -1, 1) / sqrt(3), size).  A float ulp is 1 at 1e7 and 32 at 5e8, and a triangle hit must lie within
# 10000, so the scene grows with the offset only as far as its vertices need to stay distinct: 1200 units at 5e8 puts the ball's
# triangles ~10 ulps apart and the farthest hits at ~8000.
@pytest.mark.parametrize("offset,size", [(0.0, 1.0), (1e3, 1.0), (1e5, 1.0), (1e7, 50.0), (5e8, 1200.0)])
def test_magnitude_sweep_translated(srt, oracle, offset, size):
    origin = offset / np.sqrt(3.0) * np.array([1.0, -1.0, 1.0])
    objs, meshes, cam = _sweep_scene(oracle, origin, size)
    _check(srt, oracle, Case(objs, meshes, cam, w=60, h=44, note="sweep: offset %g size %g" % (offset, size)), chunks=offset == 1e7, resume=offset == 5e8)


# scaled about the camera (the ball's centre at 6 * scale, radius `scale`; the cube mesh at 4 * scale).  At 1e-3 every triangle is
# nearer than 0.01 and at 1e4 farther than 10000: no mesh hit is valid and every ray is culled or rejected (the mesh-share condition
# cannot hold there and is waived; it does hold for the factors in between, whose hits straddle the two ends of the window:
# 2e-3 -> cube 0.007, ball from 0.010, seen through a narrower lens so that what is left of the ball still fills a tenth of the
# frame; 1.5e3 -> cube 5250, ball 7500..10500)
@pytest.mark.parametrize("scale,fov,min_mesh", [(1e-3, 55, 0.0), (2e-3, 30, 0.10), (3e-3, 55, 0.10), (1e3, 55, 0.10), (1.5e3, 55, 0.10), (1e4, 55, 0.0)])
def test_magnitude_sweep_scaled(srt, oracle, scale, fov, min_mesh):
    objs, meshes, cam = _sweep_scene(oracle, (0.0, 0.0, 0.0), scale, fov)
    _check(srt, oracle, Case(objs, meshes, cam, w=60, h=44, min_mesh=min_mesh, note="sweep: scale %g" % scale))


# ---------------------------------------------------------------------------------------------------------------------
# 5. the distance window
# ---------------------------------------------------------------------------------------------------------------------
def _facing_triangle(z, half):
    """one triangle in the plane z = const in front of a camera at the origin that looks along +z"""
    return np.array([[-3 * half, -half, z], [3 * half, -half, z], [0, 2 * half, z]], F32), np.array([[0, 1, 2]], np.uint32)


def _well_inside(V, rays, z):
    """pixels whose ray meets the plane z well inside the triangle V (float64, barycentric coordinates >= 0.02)"""
    p = rays[..., :2].astype(np.float64) * (float(z) / rays[..., 2:3].astype(np.float64))
    a, b, c = V[0, :2].astype(np.float64), V[1, :2].astype(np.float64), V[2, :2].astype(np.float64)
    m = np.linalg.inv(np.array([b - a, c - a]).T)
    uv = (p - a) @ m.T
    return (uv[..., 0] >= 0.02) & (uv[..., 1] >= 0.02) & (uv.sum(-1) <= 0.98)


def _window_case(oracle, z, half, far, note):
    objs = [_mesh(oracle, 0, base=(0.9, 0.5, 0.2), emissive=(0.1, 0.1, 0.1))] + far
    return Case(objs, [_facing_triangle(z, half)], oracle.default_camera(), w=48, h=48, note=note)


def _threshold_plane(oracle, d, lo, hi, want_valid_above, half_of):
    """the float z at which the oracle's answer for the ray `d` against the facing triangle (z, half_of(z)) flips: the smallest z
    in (lo, hi] with valid(z) == want_valid_above.  Bisection on the float's bits (positive floats order like their bits)."""
    L = oracle.lib()
    L.srt_oracle_triangle.argtypes = [C.POINTER(C.c_float)] * 5 + [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.srt_oracle_triangle.restype = C.c_int
    nn, pp, t, o = (C.c_float * 3)(), (C.c_float * 3)(), C.c_float(), (C.c_float * 3)(0, 0, 0)
    dd = (C.c_float * 3)(*[float(v) for v in d])

    def valid(bits):
        z = float(np.uint32(bits).view(F32))
        V, _ = _facing_triangle(z, half_of(z))
        return bool(L.srt_oracle_triangle((C.c_float * 3)(*V[0]), (C.c_float * 3)(*V[1]), (C.c_float * 3)(*V[2]), o, dd, nn, pp, C.byref(t)))

    a, b = int(F32(lo).view(np.uint32)), int(F32(hi).view(np.uint32))
    assert valid(a) != want_valid_above and valid(b) == want_valid_above
    while b - a > 1:
        m = (a + b) // 2
        a, b = (a, m) if valid(m) == want_valid_above else (m, b)
    return b


BLUE_BALL = lambda oracle: [_sphere(oracle, (0.0, 0.0, 6.0), 2.0, base=(0.2, 0.4, 0.9))]


def test_distance_window_near_end_sweep(srt, oracle):
    """a camera-facing triangle at z = 0.0096: its hit distance 0.0096 / d.z sweeps over 0.0099 (MESH_T_MIN_CULL) and 0.01 (the
    smallest valid distance) from the middle of the frame outwards; a second one at z = 0.00995 sweeps over 0.01 and 0.0101.  The
    triangle is 0.024 wide (a pad of ~3e-7) and leaves the frame's corners free."""
    for z, windows in ((0.0096, [(0.0, 0.0099, False), (0.0099, 0.0099999, False), (0.0100001, 0.0101, True), (0.0101, 1.0, True)]),
                       (0.00995, [(0.0099, 0.0099999, False), (0.0100001, 0.0101, True), (0.0101, 1.0, True)])):
        case = _window_case(oracle, z, 0.004, BLUE_BALL(oracle), "window: plane at %g" % z)
        rays, idx, nd = _check(srt, oracle, case)
        inside = _well_inside(case.meshes[0][0], rays, F32(z))
        t = np.float64(F32(z)) / rays[..., 2].astype(np.float64)  # (distance along the ray to the plane)
        for lo, hi, valid in windows:
            sel = (t > lo) & (t < hi) & inside
            assert sel.any(), (z, lo, hi)
            assert ((idx[sel] == 0) == valid).all(), (z, lo, hi)  # the oracle's answer differs across 0.01, not across 0.0099


@pytest.mark.parametrize("end", ["near", "far"])
def test_distance_window_ends_to_the_ulp(srt, oracle, end):
    """for the ray of one pixel, the plane at which the oracle's answer flips, found by bisection, and the planes one and two
    float steps either side of it: hit distances of 0.01f (10000.0f) to the ulp.  Near end: a pixel near the middle, so that the
    pixels outside its circle are valid hits; far end: a pixel near a corner, the pixels inside its circle are."""
    rays = _rays(oracle, oracle.default_camera(), 48, 48)
    if end == "near":
        (px, py), half_of = (32, 28), (lambda z: 0.03)
        flip = _threshold_plane(oracle, rays[py, px], 0.009, 0.0101, True, half_of)
    else:
        (px, py), half_of = (4, 5), (lambda z: 2.0 * z)
        flip = _threshold_plane(oracle, rays[py, px], 5000.0, 10001.0, False, half_of)
    answers = []
    for step in (-2, -1, 0, 1):
        z = float(np.uint32(flip + step).view(F32))
        case = _window_case(oracle, z, half_of(z), BLUE_BALL(oracle), "window: %s end, flip %+d float steps" % (end, step))
        rays2, idx, nd = _check(srt, oracle, case)
        answers.append(bool(idx[py, px] == 0))
    assert answers == ([False, False, True, True] if end == "near" else [True, True, False, False]), answers


def test_distance_window_far_end_sweep(srt, oracle):
    """a facing triangle whose distance sweeps from ~8000 in the middle of the frame to ~10300 in the corners, over 10000 (the
    largest valid distance) and 10001 (the cull on the box entry: the root box is flat, so the entry distance is the hit distance);
    it is placed so that one chosen pixel's distance is 10000.5, between the two"""
    rays = _rays(oracle, oracle.default_camera(), 48, 48)
    z = float(F32(10000.5 * float(rays[5, 4, 2])))
    case = _window_case(oracle, z, 2.0 * z, [_sphere(oracle, (0.3, -0.2, 5.0), 1.0)], "window: plane at %g" % z)
    rays, idx, nd = _check(srt, oracle, case)
    t = float(F32(z)) / rays[..., 2].astype(np.float64)
    behind = idx != 1
    for lo, hi, valid in [(5000.0, 9999.9, True), (10000.1, 10001.0, False), (10001.0, 20000.0, False)]:
        sel = (t > lo) & (t < hi) & behind
        assert sel.any(), (lo, hi)
        assert ((idx[sel] == 0) == valid).all(), (lo, hi)


def test_camera_inside_a_closed_mesh(srt, oracle):
    V, T = oracle.uv_sphere(3.0, 12, 16)
    objs = [_mesh(oracle, 0, position=(0.2, 0.1, 0.5), emissive=(0.3, 0.3, 0.4)), _sphere(oracle, (0.5, -0.5, 2.0), 0.75, specular_amount=0.9, smoothness=0.95),
            _box(oracle, (-1.0, 0.75, 2.0), (0.4, 0.4, 0.4))]
    _check(srt, oracle, Case(objs, [(V, T)], oracle.default_camera(), note="window: camera inside a mesh"), chunks=True)


def test_closed_room_made_of_a_mesh(srt, oracle):
    """every bounce starts on a triangle or ends on one: six walls of 2 x 2 quads each (inward or outward makes no difference to
    the two-sided test), a light panel just under the ceiling, a ball mesh, a sphere and a box inside"""
    walls = [_grid(2, a, c, 2.0, centre=ctr) for a, c, ctr in [(0, -2.0, (0.0, 3.0)), (0, 2.0, (0.0, 3.0)), (1, -2.0, (3.0, 0.0)), (1, 2.0, (3.0, 0.0)),
                                                             (2, 1.0, (0.0, 0.0)), (2, 5.0, (0.0, 0.0))]]
    V = np.concatenate([w[0] for w in walls])
    T = np.concatenate([w[1] + np.uint32(9 * k) for k, w in enumerate(walls)])
    # (the camera sits in the room: z from 1 to 5 would exclude it, so the room is moved to hold the origin)
    objs = [_mesh(oracle, 0, position=(0.0, 0.0, -1.5), base=(0.7, 0.7, 0.7)), _mesh(oracle, 1, position=(0.0, 0.0, -1.5), emissive=(4.0, 4.0, 3.5)),
            _mesh(oracle, 2, position=(0.5, -1.25, 2.0), base=(0.9, 0.3, 0.3), specular_amount=0.3, smoothness=0.8),
            _sphere(oracle, (-0.9, -1.4, 2.2), 0.6, specular_amount=0.9, smoothness=0.97), _box(oracle, (1.2, 0.6, 2.8), (0.3, 0.6, 0.3))]
    meshes = [(V, T), _grid(2, 1, 1.9375, 0.5, centre=(3.0, 0.0)), oracle.uv_sphere(0.75, 8, 10)]
    _check(srt, oracle, Case(objs, meshes, oracle.default_camera(), bounces=8, note="window: closed room"), resume=True)


# ---------------------------------------------------------------------------------------------------------------------
# 6. deep trees and the last resort
# ---------------------------------------------------------------------------------------------------------------------
def test_deep_tree_of_geometrically_spaced_centroids(srt, oracle):
    """the mesh of tests/native/builders_check.cpp that lets the binned SAH peel one triangle off per level (40 levels of wide
    nodes), seen from just beyond its largest triangles, which fill a quarter of the frame"""
    nt = 60000
    f = (1e-30 * np.cumprod(np.full(nt, 1.0012))).astype(F32)
    V = np.zeros((3 * nt, 3), F32)
    V[0::3, 0] = f
    V[1::3, 0], V[1::3, 1] = f * F32(1.0001), f * F32(1e-3)
    V[2::3, 0], V[2::3, 2] = f, f * F32(1e-3)
    T = np.arange(3 * nt, dtype=np.uint32).reshape(nt, 3)
    top = float(f[-1])
    cam = _camera(oracle, (top * 1.0015, top * 2.5e-4, top * 2.5e-4), forward=(-1, 0, 0), up=(0, 1, 0))
    objs = [_sphere(oracle, (top * 0.9, 0.0, 0.0), top * 0.02, emissive=(0.5, 0.4, 0.3)), _mesh(oracle, 0, base=(0.4, 0.8, 0.9))]
    _check(srt, oracle, Case(objs, [(V, T)], cam, w=40, h=30, note="deep: geometric centroids"), resume=True)


def test_pile_of_exactly_coincident_triangles(srt, oracle):
    """4000 copies of three large triangles: a ray that meets one enters every box and every leaf below it, so the queues
    overflow, batches are redone with fewer rays, and a single ray still overflows them — some 375 bottom-level nodes wait at
    once — and ends in strict depth-first mode.  Counters of a STATS=1 build for exactly this scene: 284 overflows and 71
    strict-mode entries in 78 mesh phases at 2 samples, 2080 and 520 in 548 phases at 33 (with 1000 copies: 151 overflows and no
    strict entry, which is why the pile is this large).  Every hit is a 4000-way tie.  Also chunked and resumed."""
    base = np.array([[[-2, -2, 0], [2, -2, 0], [0, 2, 0]], [[-2, 2, 0.5], [2, 2, 0.5], [0, -2, 0.5]], [[-2.5, -1, 1], [2.5, -1, 1], [0, 0, 1]]], F32)
    V = np.tile(base.reshape(9, 3), (4000, 1))
    T = np.arange(36000, dtype=np.uint32).reshape(12000, 3)
    objs = [_mesh(oracle, 0, position=(0.0, 0.0, 6.0), smoothness=0.2), _sphere(oracle, (0.0, -1002.5, 6.0), 1000.0, base=(0.5, 0.5, 0.5))]
    _check(srt, oracle, Case(objs, [(V, T)], oracle.default_camera(), w=40, h=30, spp=2, bounces=4, seed=4, note="deep: coincident pile"), ties=100, chunks=True, resume=True)


# ---------------------------------------------------------------------------------------------------------------------
# 7. many mesh objects; mesh objects that contribute no triangle
# ---------------------------------------------------------------------------------------------------------------------
TETRA = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F32) * F32(0.5), np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.uint32))
EMPTY = (np.zeros((0, 3), F32), np.zeros((0, 3), np.uint32))
ALL_INVALID = (np.array([[0, 0, 4], [1, 0, 4], [0, 1, 4], [np.nan, 0, 4]], F32), np.array([[0, 1, 7], [0, 3, 2], [9, 9, 9]], np.uint32))


def _many_objects(oracle, n=200, seed=21):
    """`n` small mesh objects over three meshes with distinct colours; before, between and after them an SRT_OBJ_NONE and objects
    of an empty mesh and of a mesh without one valid triangle, which take a primitive id (a row of the material table) and add
    nothing — the objects after them must keep their own colours and list indices"""
    rng = np.random.default_rng(seed)
    meshes = [TETRA, (CUBE_V * F32(0.25), CUBE_T), _grid(2, 2, 0.0, 0.25), EMPTY, ALL_INVALID]
    objs = [_mesh(oracle, 3, emissive=(9, 0, 0)), dict(type=oracle.OBJ_NONE), _mesh(oracle, 4, position=(0, 0, 1), emissive=(0, 9, 0))]
    for k in range(n):
        p = (rng.uniform(-2.5, 2.5), rng.uniform(-1.8, 1.8), rng.uniform(3.0, 7.0))
        objs.append(_mesh(oracle, k % 3, p, base=tuple(rng.uniform(0.1, 1, 3)), emissive=tuple(rng.uniform(0, 1.5, 3) * (k % 4 == 0))))
        if k % 37 == 5:
            objs.append(_mesh(oracle, 3 + k % 2, p, emissive=(9, 9, 9)))
        if k % 53 == 7:
            objs.append(dict(type=oracle.OBJ_NONE))
    objs += [_sphere(oracle, (0.0, -1003.0, 5.0), 1000.0, base=(0.5, 0.5, 0.5)), _box(oracle, (2.5, -1.5, 4.0), (0.5, 0.5, 0.5))]
    return objs, meshes


def test_many_mesh_objects_with_empty_ones_before_them(srt, oracle):
    objs, meshes = _many_objects(oracle)
    case = Case(objs, meshes, oracle.default_camera(), w=80, h=56, note="many: 200 mesh objects")
    rays, idx, nd = _check(srt, oracle, case, chunks=True, resume=True)
    first = set(int(i) for i in np.unique(idx) if i >= 0 and objs[i].get("type") == oracle.OBJ_MESH)
    assert len(first) >= 50 and not any(objs[i]["mesh"] >= 3 for i in first)
    # every mesh object shines a colour of its own: the accumulator of one sample without bounces names the object
    for i, o in enumerate(objs):
        o["emissive"] = (float(i + 1), 1000.0, 0.0)
    pt, oarr, n, marr, mn, keep = _tracer(srt, oracle, Case(objs, meshes, case.cam, w=case.w, h=case.h))
    pt.render(spp=1, bounces=0, seed=0)
    acc = pt.accumulator()
    hit = idx >= 0
    assert np.array_equal(acc[..., 0][hit], (idx[hit] + 1).astype(F32)) and np.all(acc[..., 1][hit] == 1000.0) and np.all(acc[..., 1][~hit] != 1000.0)
    pt.close()


def test_scene_whose_meshes_are_all_empty_or_invalid(srt, oracle):
    """mesh objects, no triangle: the mesh instantiation with n_tris == 0 (no mesh can be a first hit, so that condition is waived)"""
    objs = [_mesh(oracle, 0, emissive=(5, 5, 5)), _sphere(oracle, (0.0, 0.0, 5.0), 1.0), _mesh(oracle, 1), _box(oracle, (-2.0, 0.0, 5.0), (0.5, 0.5, 0.5)), _mesh(oracle, 1, position=(np.nan, 0, 0)),
            _mesh(oracle, 2, position=(np.inf, 0, 0)), _sphere(oracle, (0.0, -1001.0, 5.0), 1000.0)]
    _check(srt, oracle, Case(objs, [EMPTY, ALL_INVALID, TETRA], oracle.default_camera(), min_mesh=0.0, note="many: no valid triangle"), chunks=70)


# ---------------------------------------------------------------------------------------------------------------------
# 8. limits (srt_pathtrace.h): each is refused just beyond it, with a message that names it, and accepted just inside
# ---------------------------------------------------------------------------------------------------------------------
def _refused(srt, pt, objs, oracle, *words):
    oarr, n = oracle.make_objects(objs)
    with pytest.raises(srt.SrtError) as e:
        pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
    assert e.value.code == srt.capi.ERR_INVALID_ARG
    assert all(w in str(e.value) for w in words), str(e.value)


def _renders_like_the_oracle(srt, oracle, pt, case):
    oarr, n = oracle.make_objects(case.objs)
    marr, mn, keep = oracle.make_meshes(case.meshes)
    pt.set_meshes(C.cast(marr, C.POINTER(srt.Mesh)), mn)
    pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
    pt.set_camera(srt.Camera.from_buffer_copy(bytes(case.cam)))
    _check_first_hits(pt, oracle, case, oarr, n, marr, mn)
    _check_paths(pt, oracle, case, oarr, n, marr, mn)


def test_limit_world_coordinates(srt, oracle):
    objs, meshes, cam = _sweep_scene(oracle, (0.0, 0.0, 0.0), 1.0)
    case = Case(objs, meshes, cam, w=48, h=36, note="limits: after a refused scene")
    pt = srt.PathTracer(case.w, case.h)
    marr, mn, keep = oracle.make_meshes(meshes)
    pt.set_meshes(C.cast(marr, C.POINTER(srt.Mesh)), mn)
    pt.set_camera(srt.Camera.from_buffer_copy(bytes(cam)))
    for axis in range(3):
        for sign in (1.0, -1.0):
            p = [0.0, 0.0, 0.0]
            p[axis] = sign * 1.1e9
            _refused(srt, pt, objs + [_mesh(oracle, 1, p)], oracle, "coordinates", "1e9")
            with pytest.raises(srt.SrtError) as e:  # the context holds no scene now, not half of one
                pt.render()
            assert e.value.code == srt.capi.ERR_STATE
            p[axis] = sign * 9e8
            oarr, n = oracle.make_objects(objs + [_mesh(oracle, 1, p)])
            pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)  # accepted
    _refused(srt, pt, objs + [_mesh(oracle, 1, (1.1e9, 0, 0))], oracle, "coordinates")
    _renders_like_the_oracle(srt, oracle, pt, case)  # the same context, after a refusal: bit-exact
    # and a scene at 9e8 does not only load, it renders (the far copy is out of every ray's reach, the near scene is what is seen)
    case.objs = objs + [_mesh(oracle, 1, (9e8, -9e8, 9e8))]
    case.note = "limits: a mesh at 9e8"
    _renders_like_the_oracle(srt, oracle, pt, case)
    pt.close()


def test_limit_triangles_in_a_scene(srt, oracle):
    """2^24 - 1 triangles over all mesh objects are accepted, 2^24 refused before anything is built.  The triangles here have
    indices out of range: the limit counts them, the build drops them, so the test needs 12 MB and no time."""
    big = (np.zeros((0, 3), F32), np.zeros((1 << 20, 3), np.uint32))          # 2^20 triangles, none valid
    less = (np.zeros((0, 3), F32), np.zeros(((1 << 20) - 1, 3), np.uint32))   # one fewer
    objs, meshes, cam = _sweep_scene(oracle, (0.0, 0.0, 0.0), 1.0)
    nreal = sum(len(meshes[o["mesh"]][1]) for o in objs if o["type"] == oracle.OBJ_MESH)
    assert nreal < (1 << 20) - 1
    pad = (np.zeros((0, 3), F32), np.zeros(((1 << 20) - 1 - nreal, 3), np.uint32))
    all_meshes = meshes + [big, less, pad]
    case = Case(objs + [_mesh(oracle, 2)] * 15 + [_mesh(oracle, 4)], all_meshes, cam, w=48, h=36, note="limits: 2^24 - 1 triangles")
    pt = srt.PathTracer(case.w, case.h)
    marr, mn, keep = oracle.make_meshes(all_meshes)
    pt.set_meshes(C.cast(marr, C.POINTER(srt.Mesh)), mn)
    _refused(srt, pt, objs + [_mesh(oracle, 2)] * 15 + [_mesh(oracle, 4), _mesh(oracle, 4 if nreal == 0 else 1)], oracle, "triangles", "2^24")  # >= 2^24
    _refused(srt, pt, [_mesh(oracle, 2)] * 16, oracle, "triangles", "2^24")                                                                       # exactly 2^24
    _renders_like_the_oracle(srt, oracle, pt, case)                                                                                              # exactly 2^24 - 1
    pt.close()


def test_mesh_index_out_of_range_is_refused(srt, oracle):
    """srt_set_scene refuses an SRT_OBJ_MESH object whose `mesh` is negative or >= the number of meshes set, naming the object (so
    the skip of such objects in build_mesh_image is reached by no caller of the C interface; tests/native/builders_check.cpp covers it
    there).  The valid scene set afterwards on the same context renders exactly."""
    objs, meshes = _many_objects(oracle, n=40)
    case = Case(objs, meshes, oracle.default_camera(), w=48, h=36, note="limits: after a bad mesh index")
    pt = srt.PathTracer(case.w, case.h)
    marr, mn, keep = oracle.make_meshes(meshes)
    pt.set_meshes(C.cast(marr, C.POINTER(srt.Mesh)), mn)
    for bad in (-1, len(meshes), 1 << 30):
        _refused(srt, pt, objs[:5] + [_mesh(oracle, bad)] + objs[5:], oracle, "object 5", "mesh %d" % bad)
    _renders_like_the_oracle(srt, oracle, pt, case)
    pt.close()
