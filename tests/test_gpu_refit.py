"""Refitting the mesh BVH on the MI355X (srt_update_mode, srt_refit.hip.h): an srt_update_scene that only moves objects rewrites
the triangle records and requantizes the nodes on the device.  The image after a round trip is the image of the build; after
any refit the renders, first-hit buffers, sub-samples and picks are a fresh srt_set_scene's bits and the oracle's; the decoded
child boxes enclose the moved triangles; every path and reason is reached; the temporal chain, the order of enqueued work and the
layers above see no difference from a rebuild.  No test asserts a time, a work count or a launch shape."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import test_gpu_temporal as T
from conftest import ROOT, scene_path

pytestmark = pytest.mark.gpu

W, H = 37, 21
REBUILT, REFITTED, KEPT = 1, 2, 3


def strip(n):
    """n triangles along x, wobbling in y and z, sharing vertices (tests/native/refit_check.cpp's)."""
    V = np.array([[0.37 * k, 0.9 if k & 1 else -0.2 * (k % 5), 0.11 * ((k * 7) % 4)] for k in range(n + 2)], np.float32)
    V -= np.float32(0.185 * n)  # roughly centred on the object's position
    I = np.array([[k, k + 1, k + 2] for k in range(n)], np.uint32)
    return V, I


def shape(oracle, n):
    return oracle.uv_sphere(1.0, 16, 20) if n == 600 else strip(n)  # 2 * 20 * 15 = 600 triangles


def mesh_obj(oracle, pos, mesh=0, base=(0.8, 0.3, 0.2), **kw):
    return dict(type=oracle.OBJ_MESH, position=pos, mesh=mesh, base=base, **kw)


def stage(oracle):
    """A ground box and a small emissive ball: something for the mesh to shadow and be lit by."""
    return [dict(type=oracle.OBJ_BOX, position=(0.0, -1.6, 5.0), half_size=(30.0, 0.1, 30.0), base=(0.6, 0.6, 0.6)),
            dict(type=oracle.OBJ_SPHERE, position=(-1.8, 0.4, 4.0), radius=0.4, base=(0.2, 0.4, 0.9), emissive=(2.0, 2.0, 1.0))]


class Rig:
    """A tracer with meshes and a scene; keeps the ctypes arrays alive."""

    def __init__(self, srt, oracle, objs, meshes, refit=True, cam=None, w=W, h=H):
        self.srt, self.oracle = srt, oracle
        self.marr, self.mn, self.keep = oracle.make_meshes(meshes)
        self.cam = cam if cam is not None else srt.default_camera()
        self.pt = srt.PathTracer(w, h)
        self.pt.set_meshes(C.cast(self.marr, C.POINTER(srt.Mesh)), self.mn)
        if refit is not None:
            self.pt.update_mode(refit)
        self.set(objs)
        self.pt.set_camera(self.cam)

    def _arr(self, objs):
        self.oarr, self.n = self.oracle.make_objects(objs)
        return C.cast(self.oarr, C.POINTER(self.srt.Object)), self.n

    def set(self, objs):
        self.pt.set_scene(*self._arr(objs))

    def update(self, objs):
        self.pt.update_scene(*self._arr(objs))
        return self.pt.update_info()

    def oracle_acc(self, w=W, h=H, **kw):
        ocam = self.oracle.Camera.from_buffer_copy(bytes(self.cam))
        return self.oracle.render(self.oarr, self.n, self.oracle.default_environment(), ocam, w, h, meshes=(self.marr, self.mn), **kw)[1]

    def close(self):
        self.pt.close()


RENDER = dict(spp=2, bounces=3, seed=3)


def pictures(pt, row=H // 2):
    pt.render(**RENDER)
    out = {"acc": pt.accumulator().view(np.uint32), "fb": pt.framebuffer()}
    pt.render_gbuffer()
    for name in ("object", "normal_depth", "position", "albedo"):
        out[name] = np.ascontiguousarray(pt.gbuffer(name)).view(np.uint32)
    pt.render_subsamples(2)
    out["sub"] = pt.subsamples()
    out["pick"] = np.array([pt.pick(x, row) for x in range(pt.width)])
    return out


def same(a, b):
    return [k for k in a if not np.array_equal(a[k], b[k])]


def moved(objs, index, to):
    out = [dict(o) for o in objs]
    out[index]["position"] = tuple(float(np.float32(v)) for v in to)
    return out


def image_bytes(pt):
    nodes, tris = pt.mesh_image()
    return nodes.tobytes(), tris.tobytes()


# ---- 1. round trip ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 5, 9, 33, 600])
def test_round_trip_restores_the_image(srt, oracle, n):
    objs = stage(oracle) + [mesh_obj(oracle, (0.2, 0.1, 5.0))]
    rig = Rig(srt, oracle, objs, [shape(oracle, n)])
    first = image_bytes(rig.pt)
    assert len(first[1]) == 48 * n and len(first[0]) % 80 == 0 and rig.pt.update_info()["path"] == 0
    info = rig.update(moved(objs, 2, (0.55, -0.3, 6.25)))
    assert (info["path"], info["reason"], info["triangles"], info["moved_mesh_objects"]) == (REFITTED, 0, n, 1)
    assert info["nodes"] == len(first[0]) // 80 and 1 <= info["levels"] <= info["nodes"]
    there = image_bytes(rig.pt)
    assert there[1] != first[1]
    info = rig.update(objs)
    assert info["path"] == REFITTED
    assert image_bytes(rig.pt) == first
    rig.close()


# ---- 2. the same pictures as a fresh set ------------------------------------------------------------------------------------
def _cases(oracle):
    far = 1.0e6
    ball = dict(type=oracle.OBJ_SPHERE, position=(0.3, 0.0, 5.0), radius=0.7, base=(0.9, 0.9, 0.2))
    two = stage(oracle) + [mesh_obj(oracle, (-0.9, 0.0, 5.0)), mesh_obj(oracle, (0.9, 0.1, 5.5), base=(0.2, 0.8, 0.3))]
    return {
        # name: (meshes, objects, index of the moved object, its new position, camera position)
        "one triangle": ([strip(1)], stage(oracle) + [mesh_obj(oracle, (0.0, 0.0, 3.0))], 2, (0.2, 0.15, 3.5), None),
        "five triangles": ([strip(5)], stage(oracle) + [mesh_obj(oracle, (0.0, 0.0, 4.0))], 2, (-0.3, 0.2, 4.4), None),
        "sphere by 0.1 extents": ([shape(oracle, 600)], stage(oracle) + [mesh_obj(oracle, (0.0, 0.0, 5.0))], 2, (0.2, 0.0, 5.0), None),
        "sphere by 20 extents": ([shape(oracle, 600)], stage(oracle) + [mesh_obj(oracle, (3.0, 1.0, 45.0))], 2, (0.0, 0.0, 5.0), None),
        "shared mesh, the later one moves": ([shape(oracle, 600)], two, 3, (0.4, 0.3, 4.6), None),
        "coincident: list order wins": ([shape(oracle, 600)], two, 3, (-0.9, 0.0, 5.0), None),
        "straddling an analytic sphere": ([shape(oracle, 600)], stage(oracle) + [mesh_obj(oracle, (2.5, 0.0, 6.0)), ball], 2, (0.0, 0.2, 4.8), None),
        "at 1e6": ([shape(oracle, 600)], [mesh_obj(oracle, (far, 0.0, far + 5.0)), dict(ball, position=(far + 1.0, 0.0, far + 5.0))], 0,
                   (far + 0.25, 0.0625, far + 5.5), (far, 0.0, far)),
    }


@pytest.mark.parametrize("name", ["one triangle", "five triangles", "sphere by 0.1 extents", "sphere by 20 extents",
                                  "shared mesh, the later one moves", "coincident: list order wins", "straddling an analytic sphere", "at 1e6"])
def test_a_refit_gives_the_pictures_of_a_fresh_set(srt, oracle, name):
    meshes, objs, index, to, cam_pos = _cases(oracle)[name]
    cam = T.camera(srt, cam_pos) if cam_pos else None
    after = moved(objs, index, to)
    rig = Rig(srt, oracle, objs, meshes, cam=cam)
    info = rig.update(after)
    assert info["path"] == REFITTED, info
    got = pictures(rig.pt)
    fresh = Rig(srt, oracle, after, meshes, refit=None, cam=cam)
    want = pictures(fresh.pt)
    assert same(got, want) == []
    assert np.array_equal(got["acc"], rig.oracle_acc(**RENDER).view(np.uint32))
    if name.startswith("coincident"):
        assert not (got["object"] == 3).any() and (got["object"] == 2).any()  # every hit is a tie: the earlier object wins
    else:
        assert (want["object"] == index).any(), "the moved object is not in the frame (test input)"
    rig.close(), fresh.close()


# ---- 3. enclosure on the device --------------------------------------------------------------------------------------------
def _decode_and_check(nodes, tris, tri_lo, tri_hi):
    """Walk the node array per the layout comment of csrc/srt_mesh_bvh.h; every child box must enclose the boxes (float64 of
    float32 world vertices) of the triangles below it, every triangle must be in exactly one leaf."""
    nw = nodes.view(np.uint32)
    seen = np.zeros(len(tris), int)

    def walk(k, depth):
        assert depth < 64
        w0, topo = int(nw[k, 0, 3]), nw[k, 1]
        inner, leaf, counts = w0 >> 24, int(topo[2]) & 255, int(topo[2]) >> 8
        assert inner & leaf == 0
        origin = nodes[k, 0, :3].astype(np.float64)
        cell = np.array([2.0 ** (((w0 >> (8 * ax)) & 255) - 127) for ax in range(3)])
        words = nw[k, 2:5].reshape(12)
        q = np.array([[(int(words[2 * row + (c >> 2)]) >> (8 * (c & 3))) & 255 for c in range(8)] for row in range(6)])
        lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
        child, tri = int(topo[0]), int(topo[1])
        for c in range(8):
            if inner >> c & 1:
                assert k < child < len(nodes)
                clo, chi = walk(child, depth + 1)
                child += 1
            elif leaf >> c & 1:
                cnt = 1 + ((counts >> (2 * c)) & 3)
                assert tri + cnt <= len(tris)
                seen[tri:tri + cnt] += 1
                clo, chi = tri_lo[tri:tri + cnt].min(0), tri_hi[tri:tri + cnt].max(0)
                tri += cnt
            else:
                assert (q[:3, c] > q[3:, c]).all(), "an absent child must keep the inverted box"
                continue
            assert (origin + q[:3, c] * cell <= clo).all() and (chi <= origin + q[3:, c] * cell).all(), (k, c)
            lo, hi = np.minimum(lo, clo), np.maximum(hi, chi)
        return lo, hi

    walk(0, 0)
    assert (seen == 1).all()


def test_refitted_boxes_enclose_the_moved_triangles(srt, oracle):
    meshes = [shape(oracle, 600), strip(33)]
    objs = stage(oracle) + [mesh_obj(oracle, (-1.0, 0.0, 5.0)), mesh_obj(oracle, (1.5, 0.3, 6.0), mesh=1), mesh_obj(oracle, (0.0, 1.0, 7.0))]
    rig = Rig(srt, oracle, objs, meshes)
    nodes0, tris0 = rig.pt.mesh_image()
    after = moved(moved(objs, 2, (-40.0, 3.0, 90.0)), 3, (1.625, 0.2, 5.75))
    assert rig.update(after)["path"] == REFITTED
    nodes, tris = rig.pt.mesh_image()
    assert np.array_equal(nodes.view(np.uint32)[:, 1], nodes0.view(np.uint32)[:, 1]), "float4 1 of a node changed"
    assert np.array_equal(nodes.view(np.uint32)[:, 0, 3] >> 24, nodes0.view(np.uint32)[:, 0, 3] >> 24)
    assert np.array_equal(tris.view(np.uint32)[:, :, 3], tris0.view(np.uint32)[:, :, 3]), "a triangle's .w words changed"
    # the world vertices, recomputed: float32 vertex + position, per global triangle id (list order, then triangle index)
    world = []
    for o in after:
        if o["type"] == oracle.OBJ_MESH:
            V, I = meshes[o["mesh"]]
            world.append((V[I] + np.array(o["position"], np.float32)).astype(np.float32))
    world = np.concatenate(world)  # (gid, vertex, axis)
    gid = tris.view(np.uint32)[:, 1, 3]
    assert sorted(gid.tolist()) == list(range(len(world)))
    mine = world[gid]
    assert np.array_equal(tris[:, 0, :3], mine[:, 0]) and np.array_equal(tris[:, 1, :3], mine[:, 1] - mine[:, 0])
    assert np.array_equal(tris[:, 2, :3], mine[:, 2] - mine[:, 0])
    _decode_and_check(nodes, tris, mine.min(1).astype(np.float64), mine.max(1).astype(np.float64))
    rig.close()


# ---- 4. paths and reasons ----------------------------------------------------------------------------------------------------
def _path(info):
    return info["path"], info["reason"]


def test_paths_and_reasons(srt, oracle):
    meshes = [shape(oracle, 33)]
    objs = stage(oracle) + [mesh_obj(oracle, (0.0, 0.0, 5.0))]
    rig = Rig(srt, oracle, objs, meshes)
    assert _path(rig.pt.update_info()) == (0, 0)
    first = image_bytes(rig.pt)
    # only a sphere moves: kept, the same image
    info = rig.update(moved(objs, 1, (-1.5, 0.5, 4.2)))
    assert _path(info) == (KEPT, 0) and info["moved_mesh_objects"] == 0 and image_bytes(rig.pt) == first
    kept = pictures(rig.pt)
    fresh = Rig(srt, oracle, moved(objs, 1, (-1.5, 0.5, 4.2)), meshes, refit=None)
    assert same(kept, pictures(fresh.pt)) == []
    fresh.close()
    # nothing moves at all: kept
    assert _path(rig.update(moved(objs, 1, (-1.5, 0.5, 4.2)))) == (KEPT, 0)
    # a material changes: rebuilt, reason 2
    recoloured = [dict(o) for o in objs]
    recoloured[2]["base"] = (0.1, 0.9, 0.1)
    assert _path(rig.update(recoloured)) == (REBUILT, 2)
    # ... which left refit data behind: the next move refits
    assert _path(rig.update(moved(recoloured, 2, (0.3, 0.0, 5.2)))) == (REFITTED, 0)
    # REBUILD mode: reason 1, and the image a context that never heard of the mode gets
    rig.pt.update_mode(False)
    there = moved(recoloured, 2, (0.5, 0.1, 5.6))
    assert _path(rig.update(there)) == (REBUILT, 1)
    plain = Rig(srt, oracle, recoloured, meshes, refit=None)
    plain.update(there)
    assert _path(plain.pt.update_info()) == (REBUILT, 1) and image_bytes(plain.pt) == image_bytes(rig.pt)
    # the mode switched on after the scene was built: reason 4 once, then refits
    plain.pt.update_mode(True)
    assert _path(plain.update(moved(there, 2, (0.6, 0.1, 5.6)))) == (REBUILT, 4)
    assert _path(plain.update(moved(there, 2, (0.7, 0.1, 5.6)))) == (REFITTED, 0)
    fresh = Rig(srt, oracle, moved(there, 2, (0.7, 0.1, 5.6)), meshes, refit=None)
    assert same(pictures(plain.pt), pictures(fresh.pt)) == []
    plain.close(), rig.close(), fresh.close()


def test_a_dropped_triangle_or_a_non_finite_position_rebuilds(srt, oracle):
    V, I = shape(oracle, 9)
    V = V.copy()
    V[4, 1] = np.nan  # three triangles of the strip share vertex 4
    objs = stage(oracle) + [mesh_obj(oracle, (0.0, 0.0, 5.0)), mesh_obj(oracle, (0.0, 1.0, 6.0), mesh=1)]
    rig = Rig(srt, oracle, objs, [(V, I), shape(oracle, 5)])
    assert len(image_bytes(rig.pt)[1]) == 48 * (9 - 3 + 5)
    assert _path(rig.update(moved(objs, 2, (0.1, 0.0, 5.0)))) == (REBUILT, 3)
    # the clean mesh's object may move: the dropped triangles stay dropped
    there = moved(moved(objs, 2, (0.1, 0.0, 5.0)), 3, (0.2, 0.9, 5.5))
    assert _path(rig.update(there)) == (REFITTED, 0)
    fresh = Rig(srt, oracle, there, [(V, I), shape(oracle, 5)], refit=None)
    assert same(pictures(rig.pt), pictures(fresh.pt)) == []
    fresh.close()
    assert _path(rig.update(moved(there, 3, (np.inf, 0.9, 5.5)))) == (REBUILT, 3)
    rig.close()


def test_errors_leave_the_previous_scene(srt, oracle):
    meshes = [shape(oracle, 33)]
    objs = stage(oracle) + [mesh_obj(oracle, (0.0, 0.0, 5.0))]
    rig = Rig(srt, oracle, objs, meshes)
    pt, E = rig.pt, srt.capi
    assert rig.update(moved(objs, 2, (0.2, 0.0, 5.0)))["path"] == REFITTED
    before, image = pictures(pt), image_bytes(pt)
    with pytest.raises(srt.SrtError) as e:
        rig.update(moved(objs, 2, (0.2, 0.0, 2.0e9)))
    assert e.value.code == E.ERR_INVALID_ARG and "beyond 1e9" in str(e.value)
    assert pt.update_info()["path"] == REFITTED  # of the last successful update
    assert image_bytes(pt) == image and same(pictures(pt), before) == []
    with pytest.raises(srt.SrtError) as e:
        pt.update_scene(C.cast(rig.oarr, C.POINTER(srt.Object)), rig.n - 1)
    assert e.value.code == E.ERR_INVALID_ARG and same(pictures(pt), before) == []
    assert pt.L.srt_update_mode(pt._h, 2) == E.ERR_INVALID_ARG and pt.L.srt_update_mode(pt._h, -1) == E.ERR_INVALID_ARG
    assert rig.update(moved(objs, 2, (0.3, 0.0, 5.0)))["path"] == REFITTED  # the bad values did not change the mode
    rig.close()
    empty = srt.PathTracer(W, H)
    empty.update_mode(True)
    oarr, n = oracle.make_objects(objs)
    with pytest.raises(srt.SrtError) as e:
        empty.update_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
    assert e.value.code == E.ERR_STATE and empty.update_info()["path"] == 0
    with pytest.raises(srt.SrtError) as e:
        empty.mesh_image()
    assert e.value.code == E.ERR_STATE
    # a scene without meshes: kept, and an empty image
    empty.set_scene(C.cast(oarr, C.POINTER(srt.Object)), 2)
    oarr[1].position = (C.c_float * 3)(-1.0, 0.4, 4.0)
    empty.update_scene(C.cast(oarr, C.POINTER(srt.Object)), 2)
    assert empty.update_info()["path"] == KEPT and [a.size for a in empty.mesh_image()] == [0, 0]
    empty.close()


def test_new_meshes_are_not_refitted_into_the_old_image(srt, oracle):
    objs = stage(oracle) + [mesh_obj(oracle, (0.0, 0.0, 5.0))]
    rig = Rig(srt, oracle, objs, [shape(oracle, 33)])
    other = oracle.make_meshes([shape(oracle, 600)])
    rig.pt.set_meshes(C.cast(other[0], C.POINTER(srt.Mesh)), other[1])
    assert _path(rig.update(moved(objs, 1, (-1.5, 0.5, 4.2)))) == (REBUILT, 4)  # not even kept: the geometry is another
    assert len(image_bytes(rig.pt)[1]) == 48 * 600
    assert _path(rig.update(moved(objs, 2, (0.4, 0.0, 5.0)))) == (REFITTED, 0)
    rig.close()


# ---- 5. the temporal chain does not notice -----------------------------------------------------------------------------------
def _temporal_run(srt, oracle, refit):
    meshes = [shape(oracle, 600)]
    objs = stage(oracle) + [mesh_obj(oracle, (-0.6, 0.0, 5.0))]
    rig = Rig(srt, oracle, objs, meshes, refit=refit)
    pt = rig.pt
    pt.motion_output(True)
    pt.moments_output(True)
    out = []
    for k in range(3):
        if k:
            info = rig.update(moved(objs, 2, (-0.6 + 0.25 * k, 0.05 * k, 5.0 + 0.2 * k)))
            assert info["path"] == (REFITTED if refit else REBUILT)
        pt.render(spp=1, bounces=3, seed=10 + k)
        pt.temporal(samples=1, reset=k == 0)
        pt.temporal_variance()
        out.append({"acc": pt.accumulator().view(np.uint32), "length": pt.history_length().view(np.uint32), "motion": pt.motion().view(np.uint32),
                    "moments": pt.moments().view(np.uint32), "variance": pt.variance_map().view(np.uint32)})
    rig.close()
    return out


def test_the_temporal_chain_is_the_same_under_both_modes(srt, oracle):
    a, b = _temporal_run(srt, oracle, True), _temporal_run(srt, oracle, False)
    assert [same(x, y) for x, y in zip(a, b)] == [[], [], []]
    assert (a[2]["length"].view(np.float32) > 1).any() and a[2]["motion"].view(np.float32)[..., :2].any(), "the history did not follow the mesh (test input)"


# ---- 6. ordering -------------------------------------------------------------------------------------------------------------
def test_renders_before_the_update_see_the_old_scene(srt, oracle):
    meshes = [shape(oracle, 600)]
    objs = stage(oracle) + [mesh_obj(oracle, (-0.6, 0.0, 5.0))]
    after = moved(objs, 2, (0.7, 0.3, 4.5))
    old = Rig(srt, oracle, objs, meshes, refit=None)
    new = Rig(srt, oracle, after, meshes, refit=None)
    old.pt.render(**RENDER), new.pt.render(**RENDER)
    want_old, want_new = old.pt.accumulator().view(np.uint32), new.pt.accumulator().view(np.uint32)
    assert not np.array_equal(want_old, want_new)
    old.close(), new.close()
    rig = Rig(srt, oracle, objs, meshes)
    for _ in range(2):
        rig.pt.render(**RENDER)                              # enqueued before the update, read after it
        assert rig.update(after)["path"] == REFITTED
        assert np.array_equal(rig.pt.accumulator().view(np.uint32), want_old)
        rig.pt.render(**RENDER)                              # enqueued after the update
        assert np.array_equal(rig.pt.accumulator().view(np.uint32), want_new)
        assert rig.update(objs)["path"] == REFITTED
    rig.close()


# ---- 7. layers ---------------------------------------------------------------------------------------------------------------
CLI = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
VIEWER = os.path.join(ROOT, "software-raytracer_amd", "srt_viewer")


def _mesh_scene_file(tmp_path):
    scene = json.load(open(scene_path("Scene1")))
    scene["SceneObjects"][64]["Renderer"] = {"Type": "Mesh", "Primitive": "UVSphere", "Radius": 1.0, "Stacks": 16, "Slices": 20}
    p = tmp_path / "mesh_scene.json"
    p.write_text(json.dumps(scene))
    return str(p)


def test_layers_give_the_same_frame_with_and_without_refit(srt, oracle, tmp_path):
    w, h, spp, bounces, seed, frames = 64, 36, 1, 2, 5, 3
    path = _mesh_scene_file(tmp_path)
    cmd = [CLI, "--scene", path, "--width", str(w), "--height", str(h), "--spp", str(spp), "--bounces", str(bounces), "--seed", str(seed),
           "--temporal", str(frames), "--move-object", "64:0.06,0.01,0.03"]
    runs = {}
    for flag in ([], ["--refit"]):
        out = tmp_path / ("t%d.ppm" % len(flag))
        r = subprocess.run(cmd + flag + ["--out", str(out)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[len(flag)] = (T._ppm_rgb(out, w, h), r.stderr)
    assert np.array_equal(runs[0][0], runs[1][0])
    assert re.findall(r"update path (\d) reason (\d)", runs[1][1]) == [("2", "0")] * (frames - 1) and "update path" not in runs[0][1]
    bad = subprocess.run(cmd[:-2] + ["--refit"], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "--refit needs --move-object" in bad.stderr
    cams = T._parse_cameras(runs[1][1])
    places = [[float(v) for v in m.group(1).split()] for m in re.finditer(r"object 64 position((?: +[-+0-9.eE]+){3})", runs[1][1])]
    assert len(cams) == len(places) == frames
    # PathTraceRenderer with refitUpdates
    scene = srt.host.Scene(path)
    hr = srt.host.Renderer(w, h)
    hr.refit_updates(True)
    hr.set_scene(scene)
    hr.settings(fov=55, max_bounces=bounces, seed=seed)
    for k, ((p, basis), q) in enumerate(zip(cams, places)):
        if k:
            scene.set_position(64, q)
            hr.update_scene(scene)
            assert hr.update_info()["path"] == REFITTED
        hr.move_camera(p, [x for row in basis for x in row])
        hr.render_temporal_frame(spp, False)
    hr.wait()
    assert np.array_equal(T._rgb(hr.framebuffer()), runs[1][0])
    # the C calls, through PathTracer
    marr, mn = scene.meshes()
    optr, on = scene.objects()
    pt = srt.PathTracer(w, h)
    pt.update_mode(True)
    pt.set_meshes(C.cast(marr, C.POINTER(srt.Mesh)), mn)
    for k, ((p, basis), q) in enumerate(zip(cams, places)):
        optr[64].position = (C.c_float * 3)(*q)
        if k:
            pt.update_scene(C.cast(optr, C.POINTER(srt.Object)), on)
            assert pt.update_info()["path"] == REFITTED
        else:
            pt.set_scene(C.cast(optr, C.POINTER(srt.Object)), on)
        pt.set_camera(T.camera(srt, p, basis=basis, fov=55))
        pt.render(spp=spp, bounces=bounces, seed=seed + k)
        pt.render_gbuffer(outputs=srt.capi.TEMPORAL_GUIDES)
        pt.temporal(samples=spp, max_samples=max(32.0, spp), reset=k == 0, framebuffer=True, gbuffer=False)
    assert np.array_equal(T._rgb(pt.framebuffer()), runs[1][0])
    pt.close(), hr.close()


def test_viewer_refit_key_and_status_line(srt, oracle, tmp_path):
    w, h = 64, 36
    path = _mesh_scene_file(tmp_path)
    frames = {}
    for keys in ("T", "TH"):
        out = tmp_path / ("v%d.ppm" % len(keys))
        lines = ["press " + keys, "select 64", "frames 1", "update", "hold il", "frames 2", "update", "release il", "hold u", "frames 1", "update",
                 "save %s" % out]
        script = tmp_path / ("s%d.txt" % len(keys))
        script.write_text("\n".join(lines) + "\n")
        r = subprocess.run([VIEWER, "--scene", path, "--width", str(w), "--height", str(h), "--script", str(script)], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        frames[keys] = T._ppm_rgb(out, w, h)
        status = re.findall(r"^update refit (on|off) path (\w+) reason (\d)", r.stdout, flags=re.M)
        if keys == "TH":  # the scene was set before the key: the first move rebuilds (reason 4), the later ones refit
            assert status == [("on", "none", "0"), ("on", "refitted", "0"), ("on", "refitted", "0")], r.stdout
        else:
            assert status == [("off", "none", "0"), ("off", "rebuilt", "1"), ("off", "rebuilt", "1")], r.stdout
    assert np.array_equal(frames["T"], frames["TH"])
