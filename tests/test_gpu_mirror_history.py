"""The mirror history (srt_mirror_history: srt_temporal_accumulate reprojecting through mirror chains) on the MI355X: the mode on
without mirrors is the mode off, the blend against the float64 definition (tests/mirror_history_reference.py), hand-built tap
decisions, no carrying across a reflected edge in a real scene, moving objects, the state rules and errors, and the layers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mirror_history_reference as mh
from conftest import ROOT, scene_path

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
U = 2.0 ** -24  # the unit roundoff of binary32
F = np.float32
INF = float("inf")


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _bind(pt, g, albedo=None):
    """The guides g as torch tensors bound into the three G-buffer slots and the four reflection outputs the mode reads."""
    import torch

    dev = "cuda:%d" % pt.device
    t = {("g", k): torch.from_numpy(np.ascontiguousarray(g[s])).to(dev) for k, s in (("object", "obj"), ("normal_depth", "nd"), ("position", "pos"))}
    t.update({("r", k): torch.from_numpy(np.ascontiguousarray(g[s])).to(dev)
              for k, s in (("object", "r_obj"), ("normal_depth", "r_nd"), ("position", "r_pos"), ("bounces", "bounces"))})
    if albedo is not None:
        t[("g", "albedo")] = torch.from_numpy(np.ascontiguousarray(albedo)).to(dev)
    torch.cuda.synchronize()
    for (kind, k), v in t.items():
        (pt.bind_gbuffer if kind == "g" else pt.bind_reflection)(k, v)
    return t


def _acc(rgb):
    return np.concatenate([np.asarray(rgb, np.float64), np.ones(rgb.shape[:2] + (1,))], -1).astype(np.float32)


def _scene_tracer(srt, path, w, h):
    objs, n = srt.host.Scene(path).objects_copy()
    pt = srt.PathTracer(w, h)
    pt.set_scene(objs, n)
    pt.set_camera(srt.default_camera())
    return pt, (objs, n)


# ---- 1. the mode on without mirrors is the mode off -------------------------------------------------------------------------------
def test_mode_on_without_mirrors_is_the_mode_off_scene1(srt):
    w, h = 24, 20
    cams = [mh.camera(srt, (0.02 * k, 0.0, 0.05 * k), 0.4 * k) for k in range(5)]
    runs = []
    for on in (False, True):
        pt, _ = _scene_tracer(srt, scene_path("Scene1"), w, h)
        pt.motion_output(True)
        pt.moments_output(True, albedo=True)
        if on:
            pt.mirror_history(True)
        out = []
        for k, cam in enumerate(cams):
            pt.set_camera(cam)
            pt.render(spp=1, bounces=3, seed=k)
            pt.temporal(samples=1)  # (with the mode on this renders the reflection outputs too)
            out.append((pt.accumulator(), pt.history_length(), pt.motion(), pt.moments()))
            if on:
                assert not pt.read_reflection("bounces").any(), "Scene1 shows a mirror to this camera"
        runs.append(out)
        pt.close()
    for k, (a, b) in enumerate(zip(*runs)):
        assert all(_same_bits(x, y) for x, y in zip(a, b)), k
    assert (runs[0][-1][1] > 1).any()


def test_mode_on_without_mirrors_is_the_mode_off_plane_guides(srt):
    from test_gpu_moments import SYNTH_MOVES, plane_guides

    w, h = 37, 21
    runs = []
    for on in (False, True):
        rng = np.random.default_rng(4)
        pt = srt.PathTracer(w, h)
        pt.motion_output(True)
        pt.moments_output(True, albedo=True)
        if on:
            pt.mirror_history(True, radius_pixels=0.5)
        out, keep = [], None
        for dx, dy in SYNTH_MOVES:
            cam = mh.camera(srt, (dx, dy, 0.0))
            obj, nd, pos, alb = plane_guides(cam, w, h)
            g = dict(cam=cam, obj=obj, nd=nd, pos=pos, r_obj=obj.copy(), r_nd=nd.copy(), r_pos=pos.copy(), bounces=np.zeros_like(obj))
            keep = _bind(pt, g, alb)
            pt.set_camera(cam)
            pt.write_accumulator(_acc(rng.uniform(0.02, 3.0, (h, w, 3))))
            pt.temporal(samples=2, max_samples=5.0, gbuffer=False)
            out.append((pt.accumulator(), pt.history_length(), pt.motion(), pt.moments()))
        runs.append(out)
        pt.close()
        del keep
    for k, (a, b) in enumerate(zip(*runs)):
        assert all(_same_bits(x, y) for x, y in zip(a, b)), k
    assert (runs[0][-1][1] > 2).any()


# ---- 2. the definition --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,max_samples", [(1, 32.0), (2, 5.0), (3, INF)])
def test_blend_matches_the_definition(srt, n, max_samples):
    w, h = 37, 21
    sigma_t, thr, radius = 0.02, 0.9, 2.0
    rng = np.random.default_rng(21 + n)
    pt = srt.PathTracer(w, h)
    pt.mirror_history(True, radius_pixels=radius)
    pt.motion_output(True)
    prev = keep = None
    reused = 0
    for k, (dx, dy) in enumerate(mh.SYNTH_MOVES):
        cam = mh.camera(srt, (dx, dy, 0.0))
        g = mh.flat_mirror_guides(cam, w, h)
        keep = _bind(pt, g)
        pt.set_camera(cam)
        acc = _acc(rng.uniform(0.02, 3.0, (h, w, 3)))
        pt.write_accumulator(acc)
        pt.temporal(samples=n, max_samples=max_samples, plane_tolerance=sigma_t, normal_threshold=thr, gbuffer=False)
        got, L, mv = pt.accumulator(), pt.history_length(), pt.motion()
        ref = mh.accumulate(acc, g, prev, n, max_samples, sigma_t, thr, radius)
        hit = g["obj"] >= 0
        mirror = hit & (g["bounces"] >= 1)
        ended = mirror & (g["r_obj"] >= 0)
        assert np.all(ref["edge"][hit] > 1e-3), "a tap decision lies near its threshold: the guides are misplaced"
        assert _same_bits(got[~hit], acc[~hit]) and np.all(L[~hit] == 0) and np.all(mv[~hit] == 0) and np.all(mv[..., 3] == 0)
        sky = mirror & ~ended  # M3: kept bit for bit, L = n, no motion
        assert _same_bits(got[sky], acc[sky]) and np.all(L[sky] == n) and np.all(mv[sky] == 0)
        assert _same_bits(got[..., 3], acc[..., 3])
        if prev is None:
            assert _same_bits(got, acc) and np.all(L[hit] == n)
        # Roundings of a colour channel, relative to S = the largest colour in play: each of up to four taps the product w * h'
        # and its addition, 2 each and 8 in all; W itself 4 more; 1 / W and the product with it 2; L_p's sum of products 8, its
        # scaling, sum and cap 3, a = n / L and 1 - a 2, the two blend products and their sum 3: 30, rounded up to 32 (the count
        # of tests/test_gpu_moments.py's blend).  The weights come from u and v, which binary32 computes with an absolute error of
        # up to 8 roundings of their size (a, g, the quotient, the sum and the scaling), at most max(W, H); the virtual point adds
        # four (D / t0, the difference x0 - C, the product and the sum with C): 12.  A shift of the footprint by d changes a
        # convex combination of the taps by at most 2 d S per axis.
        d = 12 * max(w, h) * U
        col = np.zeros((h, w, 4)) if prev is None else prev["color"]
        S = max(float(np.max(np.abs(acc[..., :3]))), float(np.max(np.abs(col[..., :3]))))
        tol = (32 * U + 2 * 2 * d) * S
        err = np.abs(got[..., :3].astype(np.float64) - ref["out"])[hit]
        print("frame %d: colour err %.3g of tol %.3g" % (k, err.max(), tol))
        assert err.max() <= tol
        SL = max(float(np.max(ref["L"])), 1.0)
        assert np.max(np.abs(L - ref["L"])[hit]) <= (32 * U + 2 * 2 * d) * SL
        # motion: u - x carries u's error and one more rounding; W = four products of two factors that are each off by at most d
        # plus their own rounding (1 - f, the product), summed: 8 d + 12 roundings
        assert np.max(np.abs(mv[..., :2] - ref["motion"][..., :2])[hit]) <= d + U * max(w, h)
        assert np.max(np.abs(mv[..., 2] - ref["motion"][..., 2])[hit]) <= 8 * d + 12 * U
        # a count comparison, not a threshold: the same mirror pixels reuse history
        assert int((L[ended] > n).sum()) == int((ref["L"][ended] > n).sum())
        assert np.array_equal(L[hit] > n, ref["L"][hit] > n)
        if prev is not None:
            reused += int((L[ended] > n).sum())
            assert (ref["candidate"][ended] == 1).sum() > 0.8 * ended.sum()
        prev = mh.store_of(g, np.concatenate([got[..., :3], L[..., None]], -1))
    assert reused > 0.8 * ended.sum() * (len(mh.SYNTH_MOVES) - 1) * 0.9
    pt.close()
    del keep


# ---- 3. hand-built decisions --------------------------------------------------------------------------------------------------------
W3, H3 = 5, 3


def _unique(g):
    """Every pixel ends on an object of its own, so that only a pixel's own history can count for it."""
    h, w = g["obj"].shape
    ys, xs = np.mgrid[0:h, 0:w]
    return dict(g, r_obj=(100 + xs + w * ys).astype(np.int32))


def _two_frames(srt, first, second, radius=2.0, cams=None, colours=(1.0, 3.0), n=1):
    """Two calls on a small frame (5 x 3 unless the guides say otherwise): guides `first` with a grey accumulator of colours[0],
    then `second` with colours[1].
    Returns (accumulator, L, motion) of the second call.  A pixel that reuses its history ends at L = 2 n and the mean of the
    two greys; one that restarts keeps colours[1] bit for bit at L = n."""
    h, w = first["obj"].shape
    pt = srt.PathTracer(w, h)
    pt.mirror_history(True, radius_pixels=radius)
    pt.motion_output(True)
    keep = []
    for k, g in enumerate((first, second)):
        keep.append(_bind(pt, g))
        pt.set_camera(g["cam"] if cams is None else cams[k])
        c = colours[k]
        pt.write_accumulator(_acc(np.full((h, w, 3), c) if np.isscalar(c) else c))
        pt.temporal(samples=n, max_samples=INF, normal_threshold=0.9, gbuffer=False)
    res = pt.accumulator(), pt.history_length(), pt.motion()
    pt.close()
    del keep
    return res


def _reused(acc, L, mask, n=1):
    return bool(mask.any() and np.allclose(L[mask], 2 * n, rtol=1e-5) and np.allclose(acc[mask][:, :3], 2.0, rtol=1e-5))


def _restarted(acc, L, mask, n=1, colour=3.0):
    return bool(mask.any() and np.all(L[mask] == n) and _same_bits(acc[mask][:, :3], np.full((int(mask.sum()), 3), colour, F)))


def _base(srt, pos=(0.0, 0.0, 0.0)):
    cam = mh.camera(srt, pos)
    return _unique(mh.flat_mirror_guides(cam, W3, H3, features=False))


LEFT = np.mgrid[0:H3, 0:W3][1] < 2  # the pixels a case changes; the others are its control


def test_the_control_reuses_its_history(srt):
    g = _base(srt)
    acc, L, mv = _two_frames(srt, g, g)
    assert np.all(g["bounces"] == 1) and _reused(acc, L, np.ones((H3, W3), bool))
    assert np.max(np.abs(mv[..., :2])) < 1e-3 and np.allclose(mv[..., 2], 1.0, atol=1e-3)


def test_a_frame_of_one_pixel(srt):
    g = _unique(mh.flat_mirror_guides(mh.camera(srt, (0.0, 0.0, 0.0)), 1, 1, features=False))
    one = np.ones((1, 1), bool)
    assert g["bounces"][0, 0] == 1
    acc, L, mv = _two_frames(srt, g, g)
    assert _reused(acc, L, one) and abs(mv[0, 0, 2] - 1) < 1e-3
    acc, L, mv = _two_frames(srt, g, dict(g, bounces=np.full((1, 1), 3, np.int32)))
    assert _restarted(acc, L, one) and mv[0, 0, 2] == 0
    acc, L, mv = _two_frames(srt, g, mh.without_mirrors(g))  # seen directly now: tag 0 against a tagged history
    assert _restarted(acc, L, one)


@pytest.mark.parametrize("case", ["J", "m", "terminal_object"])
def test_a_mismatch_of_tag_or_object_restarts(srt, case):
    g = _base(srt)
    b = dict(g)
    if case == "J":
        b["bounces"] = np.where(LEFT, 2, g["bounces"]).astype(np.int32)
    elif case == "m":
        b["obj"] = np.where(LEFT, mh.MIRROR + 1, g["obj"]).astype(np.int32)
    else:
        b["r_obj"] = np.where(LEFT, g["r_obj"] + 500, g["r_obj"]).astype(np.int32)
    acc, L, mv = _two_frames(srt, g, b)
    assert _restarted(acc, L, LEFT) and _reused(acc, L, ~LEFT)
    assert np.all(mv[LEFT][:, 2] == 0)


def test_a_tap_just_inside_and_just_outside_the_radius(srt):
    g = _base(srt)
    r = F(mh.rho(2.0, 55.0, H3)) * g["r_nd"][..., 3]  # r_p as binary32 computes it
    for factor, inside in ((0.99, True), (1.01, False)):
        b = dict(g, r_pos=g["r_pos"].copy())
        b["r_pos"][..., 0] += np.where(LEFT, factor * r, 0.0).astype(F)
        acc, L, _ = _two_frames(srt, g, b)
        assert (_reused if inside else _restarted)(acc, L, LEFT), factor
        assert _reused(acc, L, ~LEFT)


def test_an_infinite_radius_always_passes_the_distance_test(srt):
    g = _base(srt)
    b = dict(g, r_pos=g["r_pos"].copy())
    b["r_pos"][..., 1] += np.where(LEFT, 1000.0, 0.0).astype(F)
    acc, L, _ = _two_frames(srt, g, b)
    assert _restarted(acc, L, LEFT) and _reused(acc, L, ~LEFT)
    acc, L, _ = _two_frames(srt, g, b, radius=INF)
    assert _reused(acc, L, LEFT) and _reused(acc, L, ~LEFT)


def test_a_zero_first_hit_distance_falls_through_to_the_second_candidate(srt):
    g = _base(srt)
    b = dict(g, nd=g["nd"].copy())
    b["nd"][..., 3] = np.where(LEFT, 0.0, g["nd"][..., 3])  # D / t0 = inf: candidate 1 projects nowhere
    acc, L, mv = _two_frames(srt, g, b)
    assert np.isfinite(acc).all() and np.isfinite(mv).all()
    assert _reused(acc, L, LEFT) and _reused(acc, L, ~LEFT)  # (on a still camera the mirror's own surface lands on the pixel)


def test_nan_and_inf_of_another_objects_tap_do_not_reach_a_pixel(srt):
    """The camera moves by 0.4 pixels of the image's depth, so every footprint straddles two columns.  Objects alternate by
    column; the odd columns' history holds NaN and inf in its terminal points and its colours."""
    ys, xs = np.mgrid[0:H3, 0:W3]
    odd = xs % 2 == 1
    px = 2 * np.tan(np.radians(55) / 2) * 13 / H3
    cams = [mh.camera(srt, (0.0, 0.0, 0.0)), mh.camera(srt, (0.4 * px, 0.0, 0.0))]
    a, b = (mh.flat_mirror_guides(c, W3, H3, features=False) for c in cams)
    a, b = (dict(g, r_obj=(100 + xs % 2).astype(np.int32)) for g in (a, b))
    a["r_pos"] = a["r_pos"].copy()
    a["r_pos"][odd, 0], a["r_pos"][odd, 1] = np.nan, np.inf
    first = np.full((H3, W3, 3), 1.0)
    first[odd] = np.nan
    acc, L, mv = _two_frames(srt, a, b, cams=cams, colours=(first, 3.0))
    even = ~odd
    assert np.isfinite(acc).all() and np.isfinite(L).all() and np.isfinite(mv).all()
    assert _restarted(acc, L, odd)  # their own history fails the ball test: a NaN distance
    inner = even & (xs < W3 - 1)    # (the last column's footprint may leave the frame on one side only)
    assert _reused(acc, L, inner) and np.all(mv[inner][:, 2] > 0.3) and np.all(mv[inner][:, 2] < 0.7)


def test_a_point_behind_the_previous_camera_has_no_history(srt):
    g = _base(srt)
    cams = [mh.camera(srt, (0.0, 0.0, 0.0), 180.0), g["cam"]]  # (bound guides are taken on trust: the first camera looks away)
    acc, L, mv = _two_frames(srt, g, g, cams=cams)
    every = np.ones((H3, W3), bool)
    assert _restarted(acc, L, every) and np.all(mv == 0)


def test_a_chain_that_leaves_the_scene_keeps_its_colour_and_is_never_a_tap(srt):
    g = _base(srt)
    sky = dict(g, r_obj=np.where(LEFT, -1, g["r_obj"]).astype(np.int32), r_nd=g["r_nd"].copy(), r_pos=g["r_pos"].copy())
    sky["r_nd"][LEFT] = (0.0, 0.0, 0.0, INF)
    sky["r_pos"][LEFT] = 0.0
    odd_colour = np.full((H3, W3, 3), F(0.1) * F(3))  # (a value whose bits a blend would not reproduce)
    acc, L, mv = _two_frames(srt, g, sky, colours=(1.0, odd_colour))
    assert np.all(L[LEFT] == 1) and _same_bits(acc[LEFT][:, :3], odd_colour[LEFT].astype(F)) and np.all(mv[LEFT] == 0)
    assert np.allclose(L[~LEFT], 2.0, rtol=1e-5)
    # ... and as the history of the next call it is no tap, although the pixel's guides match again
    acc, L, _ = _two_frames(srt, sky, g)
    assert _restarted(acc, L, LEFT) and _reused(acc, L, ~LEFT)


def _cells(coord, spacing, origin):
    """World-anchored cells of one pixel of the first camera: an object index per cell."""
    return (100 + np.rint((coord[..., 0] - origin[0]) / spacing) + 64 * np.rint((coord[..., 1] - origin[1]) / spacing)).astype(np.int32)


@pytest.mark.parametrize("which", [1, 2])
def test_one_candidate_fails_while_the_other_counts(srt, which):
    """which = 1: the terminal objects are cells anchored on the wall and the camera moves by one pixel of the image's depth —
    the virtual point lands on the cell's pixel, the mirror's surface (2.6 pixels away) between two other cells.
    which = 2: D is made inconsistent with the history — objects and terminal points are anchored on the mirror's surface, as
    where a strongly curved mirror keeps its image, and the camera moves by three pixels of the surface's depth: the virtual
    point lands 1.15 pixels away among other cells, the surface point on the cell's pixel."""
    depth = 13.0 if which == 1 else 5.0
    px = 2 * np.tan(np.radians(55) / 2) * depth / H3
    k = 1 if which == 1 else 3
    cams = [mh.camera(srt, (0.0, 0.0, 0.0)), mh.camera(srt, (-k * px, 0.0, 0.0))]
    frames = []
    origin = None
    for c in cams:
        g = mh.flat_mirror_guides(c, W3, H3, features=False)
        anchor = g["r_pos"] if which == 1 else g["pos"]
        if origin is None:
            origin = anchor[0, 0, :2].astype(np.float64)
        g = dict(g, r_obj=_cells(anchor.astype(np.float64), px, origin))
        if which == 2:
            g["r_pos"] = g["pos"].copy()
        frames.append(g)
    acc, L, mv = _two_frames(srt, frames[0], frames[1], cams=cams, radius=2.0)
    xs = np.mgrid[0:H3, 0:W3][1]
    inner = xs >= k  # the camera moved left: pixel x shows what pixel x - k showed
    assert _reused(acc, L, inner), (L, mv[..., 0])
    assert np.allclose(mv[inner][:, 0], -k, atol=1e-3) and np.allclose(mv[inner][:, 1], 0, atol=1e-3) and np.allclose(mv[inner][:, 2], 1, atol=2e-3)
    assert _restarted(acc, L, ~inner)


# ---- 4. no carrying across a reflected edge -----------------------------------------------------------------------------------------
def _codes(robj):
    """A power-of-two colour per terminal object: 1 for the sky and the mirror's rim, 2 ** (1 + object) otherwise."""
    return np.where(robj < 0, 1.0, 2.0 ** (1 + np.maximum(robj, 0))).astype(F)


def _edge_sequence(srt, path, on):
    w, h = 24, 20
    pt, _ = _scene_tracer(srt, path, w, h)
    pt.mirror_history(on)
    worst, mirror_seen = 0.0, 0
    for k in range(4):
        pt.set_camera(mh.camera(srt, (0.25 * k, 0.0, 0.0)))
        pt.render_reflection_gbuffer()
        robj, J = pt.read_reflection("object"), pt.read_reflection("bounces")
        code = _codes(robj)
        pt.write_accumulator(_acc(np.repeat(code[..., None], 3, -1)))
        pt.temporal(samples=1, max_samples=INF)
        got = pt.accumulator()[..., 0]
        m = (J >= 1) & (robj >= 0)
        mirror_seen += int(m.sum())
        if k:
            assert (pt.history_length()[m] > 1).any(), "no mirror pixel reuses its history: the test shows nothing"
        worst = max(worst, float(np.max(np.abs(got[m] - code[m]) / code[m])))
    pt.close()
    assert mirror_seen > 100
    return worst


def test_no_history_is_carried_across_a_reflected_edge(srt, tmp_path):
    path = mh.mirror_box_scene(tmp_path / "mirror_box.json")
    on, off = _edge_sequence(srt, path, True), _edge_sequence(srt, path, False)
    print("largest relative deviation of a mirror pixel from its own code: mode on %.3g, off %.3g" % (on, off))
    assert on <= 4 * 2.0 ** -23  # 4 ulp: a blend of equal colours is the colour up to its roundings
    assert off > 0.01            # first-hit reprojection carries the red sphere's history into the green one's image


# ---- 5. moving objects --------------------------------------------------------------------------------------------------------------
def test_moving_objects_restart_the_mirror_pixels_only(srt, tmp_path):
    import json

    w, h = 24, 20
    path = mh.mirror_box_scene(tmp_path / "mirror_box.json")
    # a fourth object seen directly (J = 0), in front of the mirror's lower part
    scene = json.load(open(path))
    scene["SceneObjects"].append(dict(scene["SceneObjects"][1], Position=[0.0, -0.8, 2.0], Renderer={"Type": "Sphere", "Radius": 0.4}))
    with open(path, "w") as f:
        json.dump(scene, f)
    runs = {}
    for on in (False, True):
        pt, (objs, cnt) = _scene_tracer(srt, path, w, h)
        pt.mirror_history(on)
        out = []
        for k in range(4):
            pt.set_camera(mh.camera(srt, (0.05 * k, 0.0, 0.0)))
            if k == 2:  # a displacement table: the green sphere moves
                objs[2].position[0] += 0.25
                pt.update_scene(objs, cnt)
            pt.render(spp=1, bounces=3, seed=k)
            pt.temporal(samples=1, max_samples=INF)
            pt.render_reflection_gbuffer()
            out.append(dict(acc=pt.accumulator(), L=pt.history_length(), J=pt.read_reflection("bounces"), robj=pt.read_reflection("object"),
                            first=pt.gbuffer("object")))
        runs[on] = out
        pt.close()
    f1, f2, f3 = runs[True][1:]
    through = [(f["J"] >= 1) & (f["first"] >= 0) for f in (f1, f2, f3)]
    direct = [(f["J"] == 0) & (f["first"] >= 0) for f in (f1, f2, f3)]
    assert through[1].sum() > 50 and direct[1].sum() > 10
    ended1 = through[0] & (f1["robj"] >= 0)  # (the rest of the mirror shows the sky: M3, never any history)
    assert ended1.sum() > 30 and (f1["L"][ended1] > 1).sum() > 0.5 * ended1.sum()  # before the edit the mirror pixels do reuse their history
    # the call that uses the table: every pixel that looks through the mirror restarts ...
    assert np.all(f2["L"][through[1]] == 1)
    # ... the pixels seen directly are the mode-off result bit for bit, history included ...
    for k in range(4):
        d = (runs[True][k]["J"] == 0) & (runs[True][k]["first"] >= 0)
        assert _same_bits(runs[True][k]["acc"][d], runs[False][k]["acc"][d]) and _same_bits(runs[True][k]["L"][d], runs[False][k]["L"][d]), k
    assert (f2["L"][direct[1]] > 2).any()
    # ... and the following call, without motion, reuses what that call stored for the mirror pixels
    ended = through[2] & (f3["robj"] >= 0)
    assert ended.sum() > 30 and np.all(f3["L"][ended] <= 2) and (f3["L"][ended] > 1).sum() > 0.5 * ended.sum()


# ---- 6. state and errors ------------------------------------------------------------------------------------------------------------
def test_refusals_of_srt_mirror_history_keep_the_setting(srt):
    pt = srt.PathTracer(W3, H3)
    g = _base(srt)
    keep = _bind(pt, g)
    pt.set_camera(g["cam"])
    pt.mirror_history(True, radius_pixels=3.0)
    P, L, Hd = srt.capi.MirrorHistoryParams, pt.L, pt._h
    for bad in (P(-1, 2.0, 0, 0), P(2, 2.0, 0, 0), P(1, 0.0, 0, 0), P(1, -1.0, 0, 0), P(0, float("nan"), 0, 0), P(1, 2.0, 1, 0), P(1, 2.0, 0, 1),
                P(0, 2.0, 0x80000000, 0)):
        assert L.srt_mirror_history(Hd, C.byref(bad)) == srt.capi.ERR_INVALID_ARG, (bad.enabled, bad.radius_pixels, bad.flags, bad.reserved)
    # the setting stands: the mode is still on (the call needs the reflection outputs) and the history was not dropped
    for c in (1.0, 3.0):
        pt.write_accumulator(_acc(np.full((H3, W3, 3), c)))
        pt.temporal(samples=1, max_samples=INF, gbuffer=False)
        for bad in (P(0, -2.0, 0, 0), P(0, 2.0, 0, 7)):
            assert L.srt_mirror_history(Hd, C.byref(bad)) == srt.capi.ERR_INVALID_ARG
    assert np.allclose(pt.history_length(), 2.0, rtol=1e-5)
    assert L.srt_mirror_history(Hd, C.byref(P(1, INF, 0, 0))) == 0
    pt.close()
    del keep


def test_toggling_drops_the_history_and_the_radius_alone_does_not(srt):
    pt = srt.PathTracer(W3, H3)
    g = _base(srt)
    keep = _bind(pt, g)
    pt.set_camera(g["cam"])
    pt.moments_output(True)

    def frame():
        pt.write_accumulator(_acc(np.full((H3, W3, 3), 1.0)))
        pt.temporal(samples=1, max_samples=INF, gbuffer=False)
        return pt.history_length(), pt.moments()[..., 2]

    pt.mirror_history(True)
    assert np.all(frame()[0] == 1)
    L, lm = frame()
    assert np.allclose(L, 2, rtol=1e-5) and np.allclose(lm, 2, rtol=1e-5)
    pt.mirror_history(True, radius_pixels=8.0)  # the radius alone
    L, lm = frame()
    assert np.allclose(L, 3, rtol=1e-5) and np.allclose(lm, 3, rtol=1e-5)
    pt.mirror_history(True, radius_pixels=8.0)  # the same setting again
    assert np.allclose(frame()[0], 4, rtol=1e-5)
    pt.mirror_history(False)  # on -> off: L = n everywhere on the next call, moments included
    L, lm = frame()
    assert np.all(L == 1) and np.all(lm == 1)
    assert np.allclose(frame()[0], 2, rtol=1e-5)
    pt.mirror_history(True)  # off -> on
    L, lm = frame()
    assert np.all(L == 1) and np.all(lm == 1)
    assert np.allclose(frame()[0], 2, rtol=1e-5)
    pt.close()
    del keep


def test_missing_or_stale_reflection_outputs_are_a_state_error(srt, tmp_path):
    w, h = 24, 20
    bad_state = srt.capi.ERR_STATE
    pt, _ = _scene_tracer(srt, mh.mirror_box_scene(tmp_path / "m.json"), w, h)
    pt.mirror_history(True)
    pt.render(spp=1, bounces=2, seed=0)
    pt.render_gbuffer()
    acc = pt.accumulator()

    def refused(words):
        with pytest.raises(srt.SrtError) as e:
            pt.temporal(gbuffer=False)
        assert e.value.code == bad_state and words in str(e.value), str(e.value)
        assert _same_bits(pt.accumulator(), acc)

    refused("OBJECT")  # nothing bound or written
    for have, missing in (("object", "NORMAL_DEPTH"), (["object", "normal_depth"], "POSITION"), (["object", "normal_depth", "position", "albedo"], "BOUNCES")):
        pt.render_reflection_gbuffer(outputs=have)
        refused("reflection output " + missing)
    with pytest.raises(srt.SrtError):
        pt.history_length()  # nothing was touched: no temporal call has run
    pt.render_reflection_gbuffer(outputs=srt.capi.MIRROR_HISTORY_GUIDES)
    pt.temporal(gbuffer=False)
    # stale: the camera moves, the first hits follow, one reflection output does not
    pt.set_camera(mh.camera(srt, (0.1, 0.0, 0.0)))
    pt.render(spp=1, bounces=2, seed=1)
    pt.render_gbuffer()
    acc = pt.accumulator()
    refused("another camera")
    pt.render_reflection_gbuffer(outputs=["object", "normal_depth", "position"])
    refused("BOUNCES was rendered with another camera")
    pt.render_reflection_gbuffer(outputs="bounces")
    pt.temporal(gbuffer=False)
    # the mode off needs none of them
    pt.mirror_history(False)
    pt.set_camera(mh.camera(srt, (0.2, 0.0, 0.0)))
    pt.render(spp=1, bounces=2, seed=2)
    pt.temporal()
    # temporal() keeps refusing to render first hits into the reflection guides' buffers
    pt.use_reflection_guides(True)
    with pytest.raises(ValueError):
        pt.temporal()
    pt.use_reflection_guides(False)
    pt.close()


def test_nothing_else_is_touched(srt, tmp_path):
    w, h = 24, 20
    pt, _ = _scene_tracer(srt, mh.mirror_box_scene(tmp_path / "m.json"), w, h)
    pt.render(spp=2, bounces=3, seed=5, count_rays=True, count_work=True)
    pt.render_gbuffer()
    pt.render_reflection_gbuffer()
    st, wc, fb = pt.stats(), pt.work_counts().as_dict(), pt.framebuffer()
    gb = {k: pt.gbuffer(k) for k in ("object", "normal_depth", "position", "albedo")}
    rf = {k: pt.read_reflection(k) for k in ("object", "normal_depth", "position", "albedo", "bounces")}
    pt.mirror_history(True)
    pt.mirror_history(True, radius_pixels=4.0)
    for _ in range(2):
        pt.temporal(samples=2, gbuffer=False)
    assert (pt.history_length() > 2).any()
    assert bytes(pt.stats()) == bytes(st) and pt.work_counts().as_dict() == wc and np.array_equal(pt.framebuffer(), fb)
    for k, v in gb.items():
        assert np.array_equal(pt.gbuffer(k).view(np.uint32), v.view(np.uint32)), k
    for k, v in rf.items():
        assert np.array_equal(pt.read_reflection(k).view(np.uint32), v.view(np.uint32)), k
    # ... and with the flag the framebuffer is written (another image, so that the bytes show it)
    pt.write_accumulator(pt.accumulator() * F(0.25))
    pt.temporal(samples=2, gbuffer=False, framebuffer=True, reset=True)
    assert not np.array_equal(pt.framebuffer(), fb)
    pt.close()


# ---- 7. the layers agree ------------------------------------------------------------------------------------------------------------
CAM_RE = re.compile(r"camera((?: +[-+0-9.eE]+){12})")


def _ppm_rgb(path, w, h):
    data = open(path, "rb").read()
    head = b"P6\n%d %d\n255\n" % (w, h)
    assert data.startswith(head)
    return np.frombuffer(data[len(head):], np.uint8).reshape(h, w, 3)


def _rgb(fb):
    return np.stack([(fb >> 16) & 255, (fb >> 8) & 255, fb & 255], -1).astype(np.uint8)


def test_layers_agree(srt, tmp_path):
    w, h, spp, bounces, seed, frames = 24, 20, 2, 3, 3, 3
    path = mh.mirror_box_scene(tmp_path / "mirror_box.json")
    cmd = [CLI, "--scene", path, "--width", str(w), "--height", str(h), "--spp", str(spp), "--bounces", str(bounces), "--seed", str(seed),
           "--temporal", str(frames), "--mirror-history", "--move", "0.2,0.0,0.0", "--out", str(tmp_path / "t.ppm")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    cams = []
    for m in CAM_RE.finditer(r.stderr):
        v = [float(x) for x in m.group(1).split()]
        cams.append((v[0:3], [v[3:6], v[6:9], v[9:12]]))
    assert len(cams) == frames
    # the C calls
    pt, _ = _scene_tracer(srt, path, w, h)
    L, Hd = pt.L, pt._h
    m = srt.capi.MirrorHistoryParams()
    assert L.srt_mirror_history_params_default(C.byref(m)) == 0 and L.srt_mirror_history(Hd, C.byref(m)) == 0
    for k, (p, basis) in enumerate(cams):
        pt.set_camera(mh.camera(srt, p, basis=basis))
        pt.render(spp=spp, bounces=bounces, seed=seed + k)
        pt.render_gbuffer(outputs=srt.capi.TEMPORAL_GUIDES)
        pt.render_reflection_gbuffer(outputs=srt.capi.MIRROR_HISTORY_GUIDES)
        t = srt.capi.temporal_params(samples=spp, max_samples=max(32.0, spp), reset=k == 0, framebuffer=True)
        assert L.srt_temporal_accumulate(Hd, C.byref(t)) == 0
    want = dict(fb=pt.framebuffer(), acc=pt.accumulator(), L=pt.history_length())
    J = pt.read_reflection("bounces")
    pt.close()
    assert (want["L"][J >= 1] > spp).any(), "no mirror pixel reuses its history"
    assert np.array_equal(_ppm_rgb(tmp_path / "t.ppm", w, h), _rgb(want["fb"]))
    # PathTracer
    pt, _ = _scene_tracer(srt, path, w, h)
    pt.mirror_history(True)
    for k, (p, basis) in enumerate(cams):
        pt.set_camera(mh.camera(srt, p, basis=basis))
        pt.render(spp=spp, bounces=bounces, seed=seed + k)
        pt.temporal(samples=spp, reset=k == 0, framebuffer=True)
    assert _same_bits(pt.accumulator(), want["acc"]) and _same_bits(pt.history_length(), want["L"]) and np.array_equal(pt.framebuffer(), want["fb"])
    pt.close()
    # PathTraceRenderer
    hr = srt.host.Renderer(w, h)
    hr.set_scene(srt.host.Scene(path))
    hr.settings(fov=55, max_bounces=bounces, seed=seed)
    hr.mirror_history(True)
    for p, basis in cams:
        hr.move_camera(p, [x for row in basis for x in row])
        hr.render_temporal_frame(spp, False)
    hr.wait()
    assert np.array_equal(hr.framebuffer(), want["fb"]) and _same_bits(hr.accumulator(), want["acc"])
    hr.close()
    # ... and the mode matters in this sequence
    pt, _ = _scene_tracer(srt, path, w, h)
    for k, (p, basis) in enumerate(cams):
        pt.set_camera(mh.camera(srt, p, basis=basis))
        pt.render(spp=spp, bounces=bounces, seed=seed + k)
        pt.temporal(samples=spp, reset=k == 0, framebuffer=True)
    assert not _same_bits(pt.accumulator(), want["acc"])
    pt.close()


def test_host_frame_denoises_with_the_reflection_guides_when_both_are_on(srt, tmp_path):
    """PathTraceRenderer with mirrorHistory and reflectionGuides: the temporal call sees first hits, the frame's denoiser the
    reflection guides — the same frame as the C calls in that order, and another one than with the first-hit guides."""
    w, h, spp, bounces, seed = 24, 20, 2, 3, 7
    path = mh.mirror_box_scene(tmp_path / "mirror_box.json")
    cams = [((0.2 * k, 0.0, 0.0), [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]) for k in range(3)]

    def host(guides):
        hr = srt.host.Renderer(w, h)
        hr.set_scene(srt.host.Scene(path))
        hr.settings(fov=55, max_bounces=bounces, seed=seed)
        hr.reflection_guides(guides)
        hr.mirror_history(True)
        for p, basis in cams:
            hr.move_camera(p, [x for row in basis for x in row])
            hr.render_temporal_frame(spp, True)
        hr.wait()
        res = hr.denoised(), hr.accumulator(), hr.framebuffer()
        hr.close()
        return res

    pt, _ = _scene_tracer(srt, path, w, h)
    pt.mirror_history(True)
    for k, (p, basis) in enumerate(cams):
        pt.set_camera(mh.camera(srt, p, basis=basis))
        pt.render(spp=spp, bounces=bounces, seed=seed + k)
        pt.temporal(samples=spp, reset=k == 0)  # first hits and the reflection outputs
        pt.use_reflection_guides(True)
        pt.denoise(framebuffer=True)            # renders the four reflection guides, then filters with them
        pt.use_reflection_guides(False)
    want = pt.denoised(), pt.accumulator(), pt.framebuffer()
    pt.close()
    got = host(True)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]) and np.array_equal(got[2], want[2])
    first = host(False)
    assert _same_bits(first[1], want[1]) and not _same_bits(first[0], want[0])
