"""closest_hit's cluster bound test about the ray's foot point (csrc/srt_kernel.hip.h; form and proof in csrc/srt_scene_image.h)
on the MI355X: frames and ray queries bit for bit against the oracle (framebuffer and all four accumulator lanes, NaNs compared as
NaNs) where the new form could go wrong — the shipped cluster scenes; Scene1 moved, with its camera, 1e3 and 1e5 away from the
origin (the bounds are taken about a reference point of the scene, and the slack must not grow with the distance); more than 32
clusters (the second mask word); clusters whose radii are tiny against their coordinates, so that every ray passes every cluster
and a wave's work list overflows (the per-lane loop); a mesh scene with clusters; and caller-supplied rays far out, axis-parallel,
of non-unit length and with NaN origins.  The frames are the 40 x 24 of test_gpu_sample_rows.py: partial blocks, several workgroups;
2 and 5 samples take the rows kernels, the mesh scene the ring kernel.  The CPU side of the same claim is test_bound_form.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu

W, H = 40, 24
THREADS = 16


def _f32(v):
    return float(np.float32(v))


def _moved(objs, by):
    """the objects moved by `by` in x and z, in binary32 (what both sides then read)"""
    out = [dict(o) for o in objs]
    for o in out:
        p = o.get("position", (0, 0, 0))
        o["position"] = (_f32(np.float32(p[0]) + np.float32(by)), _f32(p[1]), _f32(np.float32(p[2]) + np.float32(by)))
    return out


def _camera(mod, at):
    c = mod.default_camera()
    c.position = (C.c_float * 3)(*[float(v) for v in at])
    return c


def _floor(oracle, at=(0.0, 0.0, 0.0)):
    return dict(type=oracle.OBJ_SPHERE, position=(at[0], _f32(at[1] - 1001.0), _f32(at[2] + 5.0)), radius=1000.0, base=(.8, .8, .8))


def _grid(oracle, n, spacing, radius, centre):
    """n small spheres on a grid of 7 columns (x) by rows (z), two layers"""
    objs = []
    for k in range(n):
        x, z, y = k % 7, (k // 7) % 10, k // 70
        objs.append(dict(type=oracle.OBJ_SPHERE, position=(_f32(centre[0] + (x - 3) * spacing), _f32(centre[1] + y * spacing), _f32(centre[2] + z * spacing)),
                         radius=radius, base=(.2 + .1 * (k % 7), .3 + .05 * (k % 11), .9 - .1 * (k % 5)), specular_amount=0.25 * (k % 4), smoothness=0.8,
                         emissive=(2.0, 2.0, 1.0) if k % 9 == 0 else (0, 0, 0)))
    return objs


def _scene(oracle, kind):
    """kind -> (objects, meshes or None, camera position)"""
    if kind in ("Scene1", "Scene3", "Scene_indirect"):
        return oracle.load_scene_json_py(scene_path(kind)), None, (0, 0, 0)
    if kind in ("moved_1e3", "moved_1e5"):
        by = 1e3 if kind == "moved_1e3" else 1e5
        return _moved(oracle.load_scene_json_py(scene_path("Scene1")), by), None, (by, 0, by)
    if kind == "clusters_40":  # 140 small spheres: 35 clusters of four, the floor stays a uniform sphere
        return [_floor(oracle)] + _grid(oracle, 140, 0.45, 0.15, (0.0, -0.8, 3.0)), None, (0, 0, 0)
    if kind == "all_pass":  # 40 spheres of radius 0.05 at coordinates of 4e5: the bounds' slack (8e-6 of them, twice) reaches 19 units
        far = (4.0e5, -4.0e5, 4.0e5)
        return [_floor(oracle, far)] + _grid(oracle, 40, 0.4, 0.05, (far[0], far[1] - 0.8, far[2] + 3.0)), None, far
    assert kind == "mesh"  # Scene1 and two instances of a ball of 264 triangles
    objs = oracle.load_scene_json_py(scene_path("Scene1"))
    objs.insert(2, dict(type=oracle.OBJ_MESH, position=(0.4, -0.2, 3.0), mesh=0, base=(.9, .3, .2), specular_amount=0.5, smoothness=0.8))
    objs.append(dict(type=oracle.OBJ_MESH, position=(-0.8, 0.2, 3.6), mesh=0, base=(.2, .8, .3), emissive=(0.4, 0.4, 0.1)))
    return objs, [oracle.uv_sphere(0.7, 12, 12)], (0, 0, 0)


def _same_frame(pt, ofb, oacc):
    acc = pt.accumulator()
    assert np.array_equal(np.isnan(acc), np.isnan(oacc))
    bad = np.where(np.isnan(oacc), False, acc.view(np.uint32) != oacc.view(np.uint32))
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:8].tolist())
    assert np.array_equal(pt.framebuffer(), ofb)


CASES = [(k, spp) for k in ("Scene1", "Scene3", "Scene_indirect") for spp in (2, 5)] + \
        [("moved_1e3", 5), ("moved_1e5", 5), ("clusters_40", 3), ("all_pass", 3), ("mesh", 5)]


@pytest.mark.parametrize("kind,spp", CASES, ids=["%s-%d" % c for c in CASES])
def test_frames(srt, oracle, kind, spp):
    objs, meshes, at = _scene(oracle, kind)
    oarr, n = oracle.make_objects(objs)
    om = oracle.make_meshes(meshes) if meshes else None
    pt = srt.PathTracer(W, H)
    if om:
        pt.set_meshes(C.cast(om[0], C.POINTER(srt.Mesh)), om[1])
    pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
    pt.set_camera(_camera(srt, at))
    pt.render(spp=spp, bounces=8, seed=5, count_rays=True, count_work=True)
    ofb, oacc, orays = oracle.render(oarr, n, oracle.default_environment(), _camera(oracle, at), W, H, threads=THREADS, spp=spp, bounces=8, seed=5,
                                     meshes=(om[0], om[1]) if om else None)
    assert pt.stats().rays == orays
    _same_frame(pt, ofb, oacc)
    c = pt.work_counts().as_dict()
    assert c["valid"] == 1 and c["pool_steps"] > 0, "the scene must run the LDS instantiations, where the counts are kept"
    print(kind, spp, {k: c[k] for k in sorted(c)})
    if kind == "all_pass":  # every camera ray passes all ten clusters: a full wave has 640 items, more than its work list holds
        assert c["cluster_items"] >= 10 * W * H
    if kind == "clusters_40":
        assert c["cluster_bound_tests"] % 35 == 0 and c["cluster_items"] < 10 * orays
    # ... and the launch that is timed, without the counts
    pt.render(spp=spp, bounces=8, seed=5)
    _same_frame(pt, ofb, oacc)
    pt.close()


def test_caller_rays(srt, oracle):
    """srt_trace_rays on Scene1: origins 1e4 away aimed at the spheres, axis-parallel rays through the grid, directions of length
    0.5, 1 + 1e-5 and 3 (the kernel then leaves the bounds alone), NaN origins and directions"""
    rng = np.random.default_rng(77)
    objs = oracle.load_scene_json_py(scene_path("Scene1"))
    oarr, n = oracle.make_objects(objs)
    centres = np.array([o["position"] for o in objs if o.get("radius", 1e9) < 1.0], np.float64)
    o_list, d_list = [], []
    for i in range(160):  # far out, aimed at (or just past) a small sphere
        c = centres[i % len(centres)] + rng.normal(size=3) * 0.12
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        o_list.append(c - u * 1e4), d_list.append(u)
    for i in range(160):  # axis-parallel, through or beside a small sphere
        c = centres[(7 * i) % len(centres)] + rng.normal(size=3) * 0.1
        ax = np.zeros(3)
        ax[i % 3] = 1.0 if i % 2 else -1.0
        o_list.append(c - ax * float(rng.uniform(0.5, 20.0))), d_list.append(ax)
    for i in range(96):  # not of unit length
        c = centres[(5 * i) % len(centres)] + rng.normal(size=3) * 0.1
        o = np.array([0.0, 0.5, -2.0]) + rng.normal(size=3)
        u = (c - o) / np.linalg.norm(c - o)
        o_list.append(o), d_list.append(u * (0.5, 1.0 + 1e-5, 3.0)[i % 3])
    for i in range(32):  # a NaN in the origin or the direction, next to good rays of the same wave
        o, u = np.array([0.0, 0.0, 0.0]), np.array([0.0, -0.2, 1.0]) / np.linalg.norm([0.0, -0.2, 1.0])
        (o if i % 2 else u)[i % 3] = np.nan
        o_list.append(o), d_list.append(u)
    k = len(o_list)
    O4, D4 = np.zeros((k, 4), np.float32), np.zeros((k, 4), np.float32)
    O4[:, :3], D4[:, :3], D4[:, 3] = np.array(o_list, np.float32), np.array(d_list, np.float32), np.inf
    pt = srt.PathTracer(16, 16)
    pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
    pt.write_rays(O4, D4)
    pt.trace_rays()
    obj, nd = np.asarray(pt.ray_output("object"))[:k], np.asarray(pt.ray_output("normal_depth"))[:k]
    pt.close()
    L = oracle.lib()
    nn, pp, t = (C.c_float * 3)(), (C.c_float * 3)(), C.c_float()
    hits = 0
    for i in range(k):
        idx = L.srt_oracle_closest(oarr, n, (C.c_float * 3)(*O4[i, :3]), (C.c_float * 3)(*D4[i, :3]), nn, pp, C.byref(t))
        assert obj[i] == idx, (i, int(obj[i]), idx)
        if idx >= 0:
            hits += 1
            want = np.array([nn[0], nn[1], nn[2], t.value], np.float32)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(nd[i]), nan) and np.array_equal(nd[i].view(np.uint32)[~nan], want.view(np.uint32)[~nan]), i
    assert hits > k // 4
