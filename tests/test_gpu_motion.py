"""Moving objects and motion vectors on the MI355X (srt_update_scene, srt_motion_output): the definition of
include/srt_pathtrace.h against a float64 restatement on analytic guides whose objects move, the identity of an update that
moves nothing, the scene an update leaves behind, real renders of a moving sphere, reshaped and recoloured objects, errors and
state, the layers above and the noise the kept history removes.  Helpers come from test_gpu_temporal.py."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import test_gpu_temporal as T
from conftest import ROOT, scene_path
from test_gpu_temporal import REL_TOL, _bind, _frame, _guides, _same_bits, camera, moving_cameras, reference

pytestmark = pytest.mark.gpu

# (u - x, v - y): the largest error measured on the MI355X over every frame of test_moved_objects_match_the_definition is
# 2.89e-5 pixel at 256 x 160 and 8.3e-6 at 67 x 45.  The tolerance is ten times the larger, because u carries
# a few binary32 roundings at magnitude W and that differs per case; it stays far below the 0.01 pixel it must not exceed.
MV_TOL = 2.9e-4
assert MV_TOL <= 0.01
# Wsum is a sum of four products of fx, 1 - fx, fy, 1 - fy, each off by at most the error of u or v
WSUM_TOL = 4 * MV_TOL


def f32(v):
    return [float(np.float32(x)) for x in v]


def _objects(oracle, spheres, ground=(0.0, -1.0, 0.0), radii=None, colors=None):
    """Dummy objects that match the analytic guides of test_gpu_temporal.cast: 0 the ground, 1..3 the spheres."""
    objs = [dict(type=oracle.OBJ_BOX, position=ground, half_size=(100.0, 0.0, 100.0))]
    for k, (c, r) in enumerate(spheres):
        objs.append(dict(type=oracle.OBJ_SPHERE, position=c, radius=radii[k] if radii else r,
                         base=colors[k] if colors else (1, 1, 1)))
    return oracle.make_objects(objs)


def _cast(cam, w, h, spheres):
    old = T.SPHERES
    T.SPHERES = spheres
    try:
        return T.cast(cam, w, h)
    finally:
        T.SPHERES = old


def motion_reference(acc, obj, nd, pos, hist, delta, keep, n, max_samples, sigma_t, thr):
    """The contract with a motion table in float64: reference() of test_gpu_temporal.py on x~ = x - delta[o] (binary32, as the
    kernel subtracts), pixels of keep = 0 objects without history, and step 2''s (u - x, v - y).  Returns reference()'s tuple
    plus (mv (H,W,2), mv_ok: where u, v are written)."""
    H, W = obj.shape
    hit = obj >= 0
    d = np.zeros((H, W, 3), np.float32)
    k = np.ones((H, W), bool)
    listed = hit & (obj < len(delta))  # an object index beyond the table counts as delta = 0, keep = 1
    d[listed] = np.asarray(delta, np.float32)[obj[listed]]
    k[listed] = np.asarray(keep, bool)[obj[listed]]
    pos_t = pos.copy()
    pos_t[..., :3] = pos[..., :3] - d  # float32 - float32, rounded to float32
    out, L, sens, scale, sw, others = reference(acc, obj, nd, pos_t, hist, n, max_samples, sigma_t, thr)
    mv = np.zeros((H, W, 2))
    ok = np.zeros((H, W), bool)
    if hist is not None:
        drop = hit & ~k
        out[drop] = acc[..., :3].astype(np.float64)[drop]
        L[drop] = n
        sw[drop] = 0
        sens[drop] = False
        Bi = np.linalg.inv(T.ray_basis(hist["cam"], W, H)).astype(np.float32).astype(np.float64)
        rel = pos_t[..., :3].astype(np.float64) - np.array(hist["cam"].position[:], np.float32).astype(np.float64)
        abg = rel @ Bi.T
        with np.errstate(all="ignore"):
            u = (abg[..., 0] / abg[..., 2] + 1) * W / 2
            v = (abg[..., 1] / abg[..., 2] + 1) * H / 2
        ok = hit & k & (abg[..., 2] > 0) & (u > -1) & (u < W) & (v > -1) & (v < H)
        ys, xs = np.mgrid[0:H, 0:W]
        mv[..., 0] = np.where(ok, u - xs, 0.0)
        mv[..., 1] = np.where(ok, v - ys, 0.0)
    return out, L, sens, scale, sw, others, mv, ok


def _table(prev_objs, now_objs, cnt):
    """(delta, keep) of the contract from two ctypes object lists."""
    delta = np.zeros((cnt, 3), np.float32)
    keep = np.ones(cnt, bool)
    for i in range(cnt):
        a, b = prev_objs[i], now_objs[i]
        delta[i] = np.array(b.position[:], np.float32) - np.array(a.position[:], np.float32)
        aa, bb = bytearray(bytes(a)), bytearray(bytes(b))
        aa[4:16] = bb[4:16]  # the position
        keep[i] = aa == bb
    return delta, keep


def _copy(arr, cnt):
    out = type(arr)()
    C.memmove(out, arr, C.sizeof(arr))
    return out


# ---- 1. the definition --------------------------------------------------------------------------------------------------
BASE = [(f32(c), float(np.float32(r))) for c, r in T.SPHERES]


def _moved(spheres, steps):
    return [(f32(np.float32(c) + np.float32(s)), r) for (c, r), s in zip(spheres, steps)]


# every frame: (moves of the three spheres since the previous frame (several lists: several updates that compose), camera)
FRAMES = [
    ([], ((0.0, 0.0, 0.0), 0.0, 55)),
    ([[(0.15, 0.0, 0.0), (-0.1, 0.0, 0.0), (0.0, 0.08, 0.0)]], ((0.0, 0.0, 0.0), 0.0, 55)),                 # sideways
    ([[(0.0, 0.0, 0.3), (0.0, 0.0, -0.25), (0.0, 0.0, 0.2)]], ((0.0, 0.0, 0.0), 0.0, 55)),                  # in depth
    ([[(0.05, 0.02, -0.1), (-0.08, 0.0, 0.1), (0.1, -0.05, 0.0)]], ((0.04, 0.01, 0.12), 2.5, 49)),          # + translation, yaw, fov
    ([[(0.3, 0.0, 0.0), (0.0, 0.1, 0.0), (0.0, 0.0, 0.0)], [(-0.25, 0.0, 0.05), (0.0, -0.05, 0.0), (0.05, 0.0, 0.0)]],
     ((-0.1, 0.03, 0.2), -1.5, 62)),                                                                          # two updates compose
    ([], ((-0.06, 0.03, 0.25), -1.0, 62)),                                                                    # camera only: no table
]


@pytest.mark.parametrize("w,h", [(67, 45), (256, 160)])
@pytest.mark.parametrize("mv_on", [True, False])
@pytest.mark.parametrize("n,max_samples,sigma_t,thr", [(1, 32.0, 0.02, 0.9), (2, 7.0, 0.05, -1.0)])
def test_moved_objects_match_the_definition(srt, oracle, w, h, mv_on, n, max_samples, sigma_t, thr):
    rng = np.random.default_rng(w + 7 * n)
    pt = srt.PathTracer(w, h)
    pt.motion_output(mv_on)
    spheres = BASE
    hist = prev_objs = keepalive = None
    worst_mv = 0.0
    for k, (updates, (p, yaw, fov)) in enumerate(FRAMES):
        for steps in updates:
            spheres = _moved(spheres, steps)
            oarr, cnt = _objects(oracle, spheres)
            pt.update_scene(C.cast(oarr, C.POINTER(srt.Object)), cnt)
        if k == 0:
            oarr, cnt = _objects(oracle, spheres)
            pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), cnt)
        cam = camera(srt, p, yaw, fov)
        obj, nd, pos = _cast(cam, w, h, spheres)
        keepalive = _bind(pt, (obj, nd, pos))
        pt.set_camera(cam)
        acc = np.concatenate([rng.uniform(0.02, 3.0, (h, w, 3)), rng.choice([0.0, 1.0], (h, w, 1))], -1).astype(np.float32)
        pt.write_accumulator(acc)
        pt.temporal(samples=n, max_samples=max_samples, plane_tolerance=sigma_t, normal_threshold=thr, gbuffer=False)
        got, L = pt.accumulator(), pt.history_length()
        delta, keep = _table(prev_objs, oarr, cnt) if prev_objs is not None else (np.zeros((cnt, 3), np.float32), np.ones(cnt, bool))
        if k in (1, 2, 3, 4):
            assert np.any(delta != 0), "the frame moves nothing"
        ref, refL, sens, scale, sw, _, rmv, mv_ok = motion_reference(acc, obj, nd, pos, hist, delta, keep, n, max_samples, sigma_t, thr)
        hit = obj >= 0
        assert _same_bits(got[~hit], acc[~hit]) and np.all(L[~hit] == 0)
        assert _same_bits(got[..., 3], acc[..., 3]), "alpha was written"
        chk = hit & ~sens
        err = np.max(np.abs(got[..., :3].astype(np.float64) - ref), axis=2)
        bad = chk & (err > REL_TOL * scale)
        assert not bad.any(), (k, int(bad.sum()), float(np.max(err[chk] / scale[chk])))
        assert np.all(np.abs(L[chk] - refL[chk]) <= REL_TOL * refL[chk]), k
        kept = chk & (sw == 0)
        assert _same_bits(got[kept], acc[kept]) and np.all(L[kept] == n)
        moved = chk & np.any(delta[np.maximum(obj, 0)] != 0, axis=2)
        print("%dx%d frame %d: %d hit, %d checked, %d blended, %d checked on moved objects (%d blended)" % (
            w, h, k, hit.sum(), chk.sum(), (chk & (sw > 0)).sum(), moved.sum(), (moved & (sw > 0)).sum()))
        # the float64 reference alone must pin down at least 90 % of the hit pixels, and blend at least 25 % of them
        assert chk.sum() >= 0.9 * hit.sum(), k
        if k > 0:
            assert (chk & (sw > 0)).sum() >= 0.25 * hit.sum(), k
            if k < 5:
                assert (moved & (sw > 0)).sum() >= 0.25 * moved.sum() > 0, k
        if mv_on:
            mv = pt.motion()
            assert not mv[~hit].any() and not mv[..., 3].any()
            e = np.max(np.abs(mv[..., :2].astype(np.float64) - rmv), axis=2)
            worst = float(e[chk].max())
            worst_mv = max(worst_mv, worst)
            print("%dx%d frame %d: motion max abs error %.3g px over %d pixels (%d with u, v), Wsum max error %.3g" % (
                w, h, k, worst, chk.sum(), (chk & mv_ok).sum(), float(np.abs(mv[..., 2] - sw)[chk].max())))
            assert worst <= MV_TOL, (k, worst)
            assert np.all(np.abs(mv[..., 2] - sw)[chk] <= WSUM_TOL), k
            assert not mv[chk & ~mv_ok][:, :3].any(), "a pixel without previous coordinates has a motion vector"
            if k == 0:
                assert not mv.any()
            elif k < 5:
                assert np.abs(rmv[moved]).max() > 0.5, "the objects hardly move on screen"
        else:
            with pytest.raises(srt.SrtError) as ex:
                pt.motion()
            assert ex.value.code == srt.capi.ERR_STATE
        hist = dict(cam=cam, color=got, L=L, obj=obj, nd=nd, pos=pos)
        prev_objs = _copy(oarr, cnt)
    print("%dx%d: worst motion error %.3g px" % (w, h, worst_mv))
    pt.close()
    del keepalive


# ---- 2. identity --------------------------------------------------------------------------------------------------------
def _scene_tracer(srt, oracle, name, w, h):
    oarr, cnt = oracle.make_objects(oracle.load_scene_json_py(scene_path(name)))
    pt = srt.PathTracer(w, h)
    pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), cnt)
    pt.set_camera(srt.default_camera())
    return pt, oarr, cnt


def _move(oarr, idx, step):
    p = np.array(oarr[idx].position[:], np.float32) + np.array(step, np.float32)
    oarr[idx].position = (C.c_float * 3)(*[float(v) for v in p])


def test_an_update_that_moves_nothing_changes_no_bit(srt, oracle):
    w, h = 160, 96
    cams = [camera(srt, (0.02 * k, 0.0, 0.05 * k), 0.4 * k) for k in range(6)]
    outs = []
    for update in (False, True):
        pt, oarr, cnt = _scene_tracer(srt, oracle, "Scene1", w, h)
        seq = []
        for k, cam in enumerate(cams):
            if update:
                pt.update_scene(C.cast(oarr, C.POINTER(srt.Object)), cnt)
                if k == 3:  # a move and back between two temporal calls composes to nothing
                    _move(oarr, 64, (0.25, 0.0, 0.0))
                    pt.update_scene(C.cast(oarr, C.POINTER(srt.Object)), cnt)
                    oarr, cnt = oracle.make_objects(oracle.load_scene_json_py(scene_path("Scene1")))
                    pt.update_scene(C.cast(oarr, C.POINTER(srt.Object)), cnt)
            _frame(pt, cam, 1, 4, k, framebuffer=True)
            seq.append((pt.accumulator(), pt.history_length(), pt.framebuffer()))
        assert (seq[-1][1] > 4).any()
        outs.append(seq)
        pt.close()
    for (a1, l1, f1), (a2, l2, f2) in zip(*outs):
        assert _same_bits(a1, a2) and _same_bits(l1, l2) and np.array_equal(f1, f2)


def test_reset_miss_and_alpha_rules_hold_with_a_table(srt, oracle):
    w, h = 160, 96
    pt, oarr, cnt = _scene_tracer(srt, oracle, "Scene1", w, h)
    pt.motion_output(True)
    _frame(pt, srt.default_camera(), 1, 4, 0)
    _frame(pt, srt.default_camera(), 1, 4, 1)
    _move(oarr, 64, (0.1, 0.0, 0.0))
    pt.update_scene(C.cast(oarr, C.POINTER(srt.Object)), cnt)
    acc = _frame(pt, srt.default_camera(), 1, 4, 2)
    got, L, obj, mv = pt.accumulator(), pt.history_length(), pt.gbuffer("object"), pt.motion()
    assert (obj < 0).any() and (obj == 64).any()
    assert _same_bits(got[obj < 0], acc[obj < 0]) and np.all(L[obj < 0] == 0) and not mv[obj < 0].any()
    assert _same_bits(got[..., 3], acc[..., 3]), "alpha was written"
    assert (L[obj == 64] > 1).mean() > 0.9 and np.abs(mv[obj == 64][:, 0]).max() > 0.5
    # SRT_TEMPORAL_RESET with a table in play: every hit keeps its input, L = n, no motion vector
    _move(oarr, 64, (0.1, 0.0, 0.0))
    pt.update_scene(C.cast(oarr, C.POINTER(srt.Object)), cnt)
    acc = _frame(pt, srt.default_camera(), 1, 4, 3, reset=True)
    obj = pt.gbuffer("object")
    assert _same_bits(pt.accumulator(), acc)
    assert np.array_equal(pt.history_length(), np.where(obj >= 0, 1.0, 0.0).astype(np.float32))
    assert not pt.motion().any()
    pt.close()


# ---- 3. the scene an update leaves behind -------------------------------------------------------------------------------
def _mesh_scene(oracle):
    objs = oracle.load_scene_json_py(scene_path("Scene1"))
    big = objs[64]
    objs[64] = dict(type=oracle.OBJ_MESH, position=big["position"], mesh=0, base=big["base"], emissive=big["emissive"],
                    smoothness=big["smoothness"], specular_amount=big["specular_amount"], specular=big["specular"])
    return objs, [oracle.uv_sphere(1.0, 16, 24)]


@pytest.mark.parametrize("name,idx", [("Scene1", 64), ("Scene_indirect", 52), ("mesh", 64)])
def test_an_updated_scene_is_the_scene_set_afresh(srt, oracle, name, idx):
    w, h = 160, 96
    meshes = []
    if name == "mesh":
        objs, meshes = _mesh_scene(oracle)
    else:
        objs = oracle.load_scene_json_py(scene_path(name))
    marr, mn, keep = oracle.make_meshes(meshes)
    a_arr, cnt = oracle.make_objects(objs)
    b_arr, _ = oracle.make_objects(objs)
    _move(b_arr, idx, (0.35, 0.15, -0.4))
    _move(b_arr, 3, (0.0, 0.1, 0.0))
    outs = []
    for updated in (True, False):
        pt = srt.PathTracer(w, h)
        if mn:
            pt.set_meshes(C.cast(marr, C.POINTER(srt.Mesh)), mn)
        if updated:
            pt.set_scene(C.cast(a_arr, C.POINTER(srt.Object)), cnt)
            pt.set_camera(srt.default_camera())
            pt.render(spp=2, bounces=4, seed=1, count_rays=True, count_work=True)  # (records block work for the old scene)
            pt.render(spp=2, bounces=4, seed=1, first_sample=3, reset=False)
            pt.wait()
            pt.update_scene(C.cast(b_arr, C.POINTER(srt.Object)), cnt)
        else:
            pt.set_scene(C.cast(b_arr, C.POINTER(srt.Object)), cnt)
            pt.set_camera(srt.default_camera())
        pt.render(spp=3, bounces=5, seed=7, count_rays=True, count_work=True)
        st = pt.stats()
        out = dict(fb=pt.framebuffer(), acc=pt.accumulator(), rays=st.rays)
        pt.render_gbuffer()
        for g in ("object", "normal_depth", "position", "albedo"):
            out[g] = pt.gbuffer(g)
        out["pick"] = [pt.pick(x, y) for x in range(4, w, 13) for y in range(3, h, 11)]
        out["costs"] = pt.estimate_row_costs(4, 0)
        outs.append(out)
        pt.close()
    u, f = outs
    assert idx in u["pick"] and (u["object"] == idx).any()
    for k in ("fb", "acc", "object", "normal_depth", "position", "albedo"):
        assert np.array_equal(u[k].view(np.uint32), f[k].view(np.uint32)), k
    for k in ("rays", "pick", "costs"):
        assert u[k] == f[k], k
    del keep


# ---- 4. real renders ----------------------------------------------------------------------------------------------------
def test_a_moving_sphere_keeps_its_history(srt, oracle):
    """Scene1, still camera, 8 frames of 1 spp, the big sphere moved by a fixed step per frame.  The uncovered static pixels
    are judged where float32 can pin them down.  A still camera reprojects a pixel to within a rounding error of itself (about
    1e-5 pixel), so one of its eight neighbours may take a weight of that size, and by the existing step 3 a tap of any
    positive weight counts: an uncovered pixel next to a previous-frame pixel of its own object may therefore blend with that
    neighbour, whichever way the rounding falls (measured with a step of 0.05, under one pixel a frame: 13 uncovered pixels,
    every one with such a neighbour, 10 kept their bits).  The step is 0.15, about three pixels a frame, so that the uncovered
    strip has pixels whose whole previous 3 x 3 neighbourhood showed other objects: those must keep their bits."""
    w, h, frames, idx, step = 160, 96, 8, 64, (0.15, 0.0, 0.0)
    cam = srt.default_camera()
    res = {}
    for how in ("update", "set"):
        pt, oarr, cnt = _scene_tracer(srt, oracle, "Scene1", w, h)
        prev = None
        for k in range(frames):
            if k:
                _move(oarr, idx, step)
                (pt.update_scene if how == "update" else pt.set_scene)(C.cast(oarr, C.POINTER(srt.Object)), cnt)
            if k == frames - 1:
                prev = dict(cam=cam, color=pt.accumulator(), L=pt.history_length())
                prev.update(zip(("obj", "nd", "pos"), _guides(pt)))
            acc = _frame(pt, cam, 1, 4, 50 + k)
        res[how] = (acc, pt.accumulator(), pt.history_length(), _guides(pt), prev)
        pt.close()
    acc, got, L, (obj, nd, pos), prev = res["update"]
    on_both = (obj == idx) & (prev["obj"] == idx)
    print("sphere pixels in both frames %d, mean L %.3f" % (on_both.sum(), L[on_both].mean()))
    assert on_both.sum() > 200 and L[on_both].mean() >= 0.9 * frames
    Ls = res["set"][2]
    assert np.all(Ls[res["set"][3][0] >= 0] == 1), "srt_set_scene kept a history"
    # static pixels the sphere uncovered in the last frame
    unc = (prev["obj"] == idx) & (obj >= 0) & (obj != idx)
    po = np.pad(prev["obj"], 1, constant_values=-1)
    same_near = np.zeros((h, w), bool)  # a previous-frame pixel of the 3 x 3 neighbourhood showed this pixel's object
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            same_near |= po[dy:dy + h, dx:dx + w] == obj
    pinned = unc & ~same_near
    print("uncovered pixels %d, pinned down %d, keeping their bits %d" % (unc.sum(), pinned.sum(),
          sum(_same_bits(got[y, x], acc[y, x]) for y, x in zip(*np.nonzero(unc)))))
    assert pinned.sum() >= 10
    assert _same_bits(got[pinned], acc[pinned]) and np.all(L[pinned] == 1)
    # static pixels away from it (nothing of the sphere within 4 pixels in any frame's reach)
    near = np.zeros((h, w), bool)
    ys, xs = np.nonzero((obj == idx) | (res["set"][4]["obj"] == idx))
    near[max(ys.min() - 4, 0):ys.max() + 5, 0:xs.max() + 5] = True
    far = (obj >= 0) & ~near
    assert far.sum() > 1000 and np.allclose(L[far], frames, rtol=1e-5)


# ---- 5. keep = 0 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change", ["radius", "color"])
def test_a_reshaped_or_recoloured_object_restarts_its_own_pixels(srt, oracle, change):
    w, h, n = 128, 80, 1
    cams = [camera(srt, (0.0, 0.0, 0.0)), camera(srt, (0.03, 0.0, 0.05), 0.8), camera(srt, (0.05, 0.01, 0.1), 1.2)]
    steps = [(0.05, 0.0, 0.0), (0.0, 0.0, 0.1), (-0.05, 0.02, 0.0)]
    outs = []
    for changed in (True, False):
        rng = np.random.default_rng(5)
        pt = srt.PathTracer(w, h)
        pt.motion_output(True)
        spheres = BASE
        for k, cam in enumerate(cams):
            if k:
                spheres = _moved(spheres, steps)
            kw = {}
            if changed and k == 2 and change == "radius":
                kw["radii"] = [0.8, 1.25, 0.9]
            if changed and k == 2 and change == "color":
                kw["colors"] = [(1, 1, 1), (0.2, 0.4, 0.9), (1, 1, 1)]
            oarr, cnt = _objects(oracle, spheres, **kw)
            (pt.update_scene if k else pt.set_scene)(C.cast(oarr, C.POINTER(srt.Object)), cnt)
            obj, nd, pos = _cast(cam, w, h, spheres)
            keepalive = _bind(pt, (obj, nd, pos))
            pt.set_camera(cam)
            acc = np.concatenate([rng.uniform(0.02, 3.0, (h, w, 3)), np.ones((h, w, 1))], -1).astype(np.float32)
            pt.write_accumulator(acc)
            pt.temporal(samples=n, gbuffer=False)
        outs.append((acc, pt.accumulator(), pt.history_length(), pt.motion(), obj))
        pt.close()
        del keepalive
    (acc, got, L, mv, obj), (_, got0, L0, mv0, _) = outs
    own = obj == 2
    assert own.sum() > 100
    assert _same_bits(got[own], acc[own]) and np.all(L[own] == n) and not mv[own].any()
    assert (L0[own] > n).mean() > 0.8, "the unchanged object does not blend"
    assert _same_bits(got[~own], got0[~own]) and _same_bits(L[~own], L0[~own]) and _same_bits(mv[~own], mv0[~own])
    assert (L[~own] > n).sum() > 0.5 * (obj[~own] >= 0).sum()


# ---- 6. errors and state ------------------------------------------------------------------------------------------------
def test_errors_and_state(srt, oracle):
    import torch

    w, h = 160, 96
    fields = ("rays", "sample_chunks", "tile_rows", "chunk_samples", "shape_source", "path_samples")
    oarr, cnt = oracle.make_objects(oracle.load_scene_json_py(scene_path("Scene1")))
    ptr = C.cast(oarr, C.POINTER(srt.Object))
    pt = srt.PathTracer(w, h)
    # no scene set
    assert pt.L.srt_update_scene(pt._h, ptr, cnt) == srt.capi.ERR_STATE
    with pytest.raises(srt.SrtError) as e:
        pt.motion()
    assert e.value.code == srt.capi.ERR_STATE
    pt.set_scene(ptr, cnt)
    cam = srt.default_camera()
    canary = torch.full((h, w, 4), 123.5, dtype=torch.float32, device="cuda:0")
    pt.bind_motion(canary)
    _frame(pt, cam, 1, 4, 0)
    _frame(pt, cam, 1, 4, 1)
    assert (pt.history_length() == 2).any()
    # a count mismatch, an unknown type: refused before anything is touched; scene and history keep working
    assert pt.L.srt_update_scene(pt._h, ptr, cnt - 1) == srt.capi.ERR_INVALID_ARG
    assert pt.L.srt_update_scene(pt._h, ptr, cnt + 1) == srt.capi.ERR_INVALID_ARG
    bad_arr = _copy(oarr, cnt)
    bad = C.cast(bad_arr, C.POINTER(srt.Object))
    bad[5].type = 77
    assert pt.L.srt_update_scene(pt._h, bad, cnt) == srt.capi.ERR_INVALID_ARG
    _frame(pt, cam, 1, 4, 2)
    assert (pt.history_length() == 3).any(), "a refused update dropped the history"
    # motion output off: nothing written, nothing to read
    pt.wait()
    torch.cuda.synchronize()
    assert bool((canary == 123.5).all()), "the motion buffer was written with the output off"
    with pytest.raises(srt.SrtError) as e:
        pt.motion()
    assert e.value.code == srt.capi.ERR_STATE
    # on: the bound buffer is what motion() reads; own buffer after unbinding has not been written
    pt.motion_output(True)
    _move(oarr, 64, (0.08, 0.0, 0.0))
    pt.update_scene(ptr, cnt)
    pt.render(spp=1, bounces=4, seed=3, count_rays=True, count_work=True)
    first, work = pt.stats(), pt.work_counts().as_dict()
    pt.render_gbuffer(outputs=15)
    g = {n: pt.gbuffer(n) for n in ("object", "normal_depth", "position", "albedo")}
    pt.temporal(gbuffer=False)
    mv = pt.motion()
    torch.cuda.synchronize()
    assert np.array_equal(canary.cpu().numpy().view(np.uint32), mv.view(np.uint32))
    assert np.abs(mv[g["object"] == 64][:, 0]).max() > 0.5 and (pt.history_length() == 4).any()
    after = pt.stats()
    assert all(getattr(after, f) == getattr(first, f) for f in fields) and after.kernel_ms == first.kernel_ms
    assert pt.work_counts().as_dict() == work
    for n in g:
        assert np.array_equal(pt.gbuffer(n).view(np.uint32), g[n].view(np.uint32)), n
    pt.bind_motion(None)
    with pytest.raises(srt.SrtError) as e:  # the own buffer is not the one that was written
        pt.motion()
    assert e.value.code == srt.capi.ERR_STATE
    pt.motion_output(False)
    _frame(pt, cam, 1, 4, 4)
    canary.fill_(7.0)
    _frame(pt, cam, 1, 4, 5)
    pt.wait()
    torch.cuda.synchronize()
    assert bool((canary == 7.0).all())
    # srt_set_scene after updates still drops the history
    pt.update_scene(ptr, cnt)
    pt.set_scene(ptr, cnt)
    acc = _frame(pt, cam, 1, 4, 6)
    assert _same_bits(pt.accumulator(), acc)
    assert np.array_equal(pt.history_length(), np.where(pt.gbuffer("object") >= 0, 1.0, 0.0).astype(np.float32))
    pt.close()


def test_the_same_calls_give_the_same_bits_and_later_renders_their_shape(srt, oracle):
    w, h = 200, 120
    fields = ("rays", "sample_chunks", "tile_rows", "chunk_samples", "shape_source", "path_samples")
    runs = []
    for with_motion in (True, True, False):
        pt, oarr, cnt = _scene_tracer(srt, oracle, "Scene1", w, h)
        pt.motion_output(with_motion)
        seq = []
        for k, cam in enumerate(moving_cameras(srt, 4)):
            if k:
                _move(oarr, 64, (0.04, 0.0, 0.02))
                # the plain sequence sets the scene instead: the same scene for the later render
                (pt.update_scene if with_motion else pt.set_scene)(C.cast(oarr, C.POINTER(srt.Object)), cnt)
            _frame(pt, cam, 2, 4, k)
            if with_motion:
                seq.append((pt.accumulator(), pt.history_length(), pt.motion()))
        pt.set_camera(srt.default_camera())
        pt.render(spp=4, bounces=4, seed=9, count_rays=True, count_work=True)
        st = pt.stats()
        runs.append(([getattr(st, f) for f in fields], pt.work_counts().as_dict(), pt.framebuffer(), pt.accumulator(), seq))
        pt.close()
    a, b, c = runs
    for x in (b, c):
        assert a[0] == x[0] and a[1] == x[1]
        assert np.array_equal(a[2], x[2]) and _same_bits(a[3], x[3])
    for s1, s2 in zip(a[4], b[4]):
        assert all(_same_bits(p, q) for p, q in zip(s1, s2)), "two identical sequences differ"


# ---- 7. layers ----------------------------------------------------------------------------------------------------------
CLI = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
VIEWER = os.path.join(ROOT, "software-raytracer_amd", "srt_viewer")
OBJ_RE = re.compile(r"object (\d+) position((?: +[-+0-9.eE]+){3})")


def _sequence(srt, oracle, w, h, cams, places, spp, bounces, seed):
    """What RenderTemporalFrame does after UpdateScene, through the C-ABI.  places[k]: {object: position} of frame k."""
    pt, oarr, cnt = _scene_tracer(srt, oracle, "Scene1", w, h)
    for k, ((p, basis), place) in enumerate(zip(cams, places)):
        for i, q in place.items():
            oarr[i].position = (C.c_float * 3)(*q)
        if k:
            pt.update_scene(C.cast(oarr, C.POINTER(srt.Object)), cnt)
        pt.set_camera(camera(srt, p, basis=basis, fov=55))
        pt.render(spp=spp, bounces=bounces, seed=seed + k)
        pt.render_gbuffer(outputs=srt.capi.TEMPORAL_GUIDES)
        pt.temporal(samples=spp, max_samples=max(32.0, spp), reset=k == 0, framebuffer=True, gbuffer=False)
    fb, L = pt.framebuffer(), pt.history_length()
    pt.close()
    return fb, L


def test_layers_give_the_same_frame(srt, oracle, tmp_path):
    w, h, spp, bounces, seed, frames = 160, 90, 2, 3, 5, 5
    cmd = [CLI, "--scene", scene_path("Scene1"), "--width", str(w), "--height", str(h), "--spp", str(spp), "--bounces", str(bounces),
           "--seed", str(seed), "--temporal", str(frames), "--move", "0.01,0.005,0.03", "--turn", "0.7",
           "--move-object", "64:0.04,0,0.015", "--move-object", "3:0,0.02,0", "--out", str(tmp_path / "t.ppm")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    cams = T._parse_cameras(r.stderr)
    places = [dict() for _ in range(frames)]
    for m in re.finditer(r"temporal frame (\d+) " + OBJ_RE.pattern, r.stderr):
        places[int(m.group(1))][int(m.group(2))] = [float(v) for v in m.group(3).split()]
    assert len(cams) == frames and all(sorted(p) == [3, 64] for p in places)
    assert places[0][64] == [0.0, 0.0, 5.0] and places[-1][64] != places[0][64]
    want, L = _sequence(srt, oracle, w, h, cams, places, spp, bounces, seed)
    assert (L > 3 * spp).sum() > 0.5 * (L > 0).sum(), "the history did not survive the edits"
    assert np.array_equal(T._ppm_rgb(tmp_path / "t.ppm", w, h), T._rgb(want))
    # PathTraceRenderer::UpdateScene + RenderTemporalFrame
    scene = srt.host.Scene(scene_path("Scene1"))
    hr = srt.host.Renderer(w, h)
    hr.set_scene(scene)
    hr.settings(fov=55, max_bounces=bounces, seed=seed)
    hr.motion_output(True)
    for k, ((p, basis), place) in enumerate(zip(cams, places)):
        if k:
            for i, q in place.items():
                scene.set_position(i, q)
            hr.update_scene(scene)
        hr.move_camera(p, [x for row in basis for x in row])
        hr.render_temporal_frame(spp, False)
    hr.wait()
    assert np.array_equal(hr.framebuffer(), want)
    assert _same_bits(hr.history_length(), L)
    assert np.abs(hr.motion()[hr.gbuffer("object") == 64][:, :2]).max() > 0.3
    # SetScene drops the history, UpdateScene with another number of objects falls back to it
    scene.remove(10)
    hr.update_scene(scene)
    hr.render_temporal_frame(spp, False)
    assert np.all(hr.history_length()[hr.gbuffer("object") >= 0] == spp)
    hr.close()
    bad = subprocess.run(cmd[:-2] + ["--move-object", "999:0,0,1"], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "no object" in bad.stderr


def test_viewer_moves_the_selected_object_in_temporal_mode(srt, oracle, tmp_path):
    w, h = 128, 72
    lines = ["press T", "select 64", "frames 1", "camera", "object", "hold il", "frames 1", "camera", "object", "hold D", "frames 1", "camera",
             "object", "release il", "hold uj", "frames 1", "camera", "object", "release ujD", "hold ok", "frames 1", "camera", "object",
             "save %s" % (tmp_path / "v.ppm")]
    script = tmp_path / "s.txt"
    script.write_text("\n".join(lines) + "\n")
    r = subprocess.run([VIEWER, "--scene", scene_path("Scene1"), "--width", str(w), "--height", str(h), "--script", str(script)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    cams = T._parse_cameras(r.stdout)
    places = [{int(m.group(1)): [float(v) for v in m.group(2).split()]} for m in OBJ_RE.finditer(r.stdout)]
    assert len(cams) == len(places) == 5 and all(list(p) == [64] for p in places)
    q = [p[64] for p in places]
    assert q[0] == [0.0, 0.0, 5.0] and q[1][0] > q[0][0] and q[1][2] > q[0][2] and q[3][1] > q[2][1] and q[3][0] < q[2][0]
    assert q[4][1] < q[3][1] and q[4][2] < q[3][2]
    want, L = _sequence(srt, oracle, w, h, cams, places, 1, 2, 0)
    assert (L >= 4).sum() > 0.5 * (L > 0).sum(), "the viewer's edits dropped the history"
    assert np.array_equal(T._ppm_rgb(tmp_path / "v.ppm", w, h), T._rgb(want))


# ---- 8. value -----------------------------------------------------------------------------------------------------------
# measured on the MI355X (profiles/temporal/motion_quality.jsonl): tone-mapped MSE of the last frame against
# a 1024-spp render, relative to the same sequence with srt_set_scene per frame (a plain 1-spp last frame):
#   Scene1 0.070 over hit pixels and 0.096 over the moved object, mean linear shift 0.40 %;
#   Scene_indirect 0.109 and 0.066, shift 1.17 %.
# The test asserts twice the measured ratios (the camera-only ratios moved by less than that between seeds and boxes).
MSE_RATIO_MAX = {"Scene1": (0.141, 0.192), "Scene_indirect": (0.217, 0.132)}
assert all(v < 1 for pair in MSE_RATIO_MAX.values() for v in pair)


@pytest.mark.parametrize("name,idx", [("Scene1", 64), ("Scene_indirect", 52)])
def test_it_keeps_samples_while_an_object_moves(srt, oracle, name, idx):
    w, h, bounces, frames = 320, 180, 8, 16
    cams = moving_cameras(srt, frames)
    res = {}
    for how in ("update", "set"):
        pt, oarr, cnt = _scene_tracer(srt, oracle, name, w, h)
        for k, cam in enumerate(cams):
            if k:
                _move(oarr, idx, (0.01, 0.0, 0.004))
                (pt.update_scene if how == "update" else pt.set_scene)(C.cast(oarr, C.POINTER(srt.Object)), cnt)
            _frame(pt, cam, 1, bounces, 1000 + k)
        res[how] = pt.accumulator()
        obj = pt.gbuffer("object")
        if how == "set":
            pt.render(spp=1024, bounces=bounces, seed=777)
            ref = pt.accumulator()
        pt.close()
    hit, own = obj >= 0, obj == idx
    tm = lambda a, m: (a[..., :3] / (1.0 + a[..., :3]))[m].astype(np.float64)  # noqa: E731
    mse = lambda a, m: float(np.mean((tm(a, m) - tm(ref, m)) ** 2))  # noqa: E731
    r_hit = mse(res["update"], hit) / mse(res["set"], hit)
    r_own = mse(res["update"], own) / mse(res["set"], own)
    shift = abs(float(np.mean(res["update"][..., :3][hit], dtype=np.float64)) / float(np.mean(ref[..., :3][hit], dtype=np.float64)) - 1)
    line = dict(scene=name, width=w, height=h, frames=frames, bounces=bounces, object=idx, object_pixels=int(own.sum()),
                mse_ratio_hit=round(r_hit, 4), mse_ratio_object=round(r_own, 4), mean_shift=round(shift, 5))
    print(json.dumps(line))
    assert own.sum() > 500
    assert r_hit <= MSE_RATIO_MAX[name][0] and r_own <= MSE_RATIO_MAX[name][1]
