"""The float64 definitions that tests/test_gpu_pass_edges.py holds the kernels to, alone, on the inputs of
tests/pass_edge_inputs.py: they run at every frame shape without an exception and without a NaN from finite inputs, their exact
identities hold, and they leave no more pixels undecided than the GPU tests may leave out.  No GPU."""
import importlib

import numpy as np
import pytest

import pass_edge_inputs as pe
import test_gpu_denoise as dn
import test_gpu_motion as mo
import test_gpu_temporal as tp
import test_gpu_upsample as up
import variance_reference as vr
from antialias_reference import resolve
from pass_edge_inputs import SHAPES


@pytest.fixture(scope="module")
def srt():
    return importlib.import_module("software-raytracer_amd")  # (its ctypes structures only: cameras)


def test_shapes_and_generators():
    assert SHAPES[-1] == (33, 18) and (1, 1) in SHAPES and (300, 1) in SHAPES and (1, 300) in SHAPES
    assert {w * h for w, h in SHAPES + [(255, 1), (16, 16), (257, 1)]} >= {1, 255, 256, 257, 300}
    for w, h in SHAPES:
        acc, obj, nd, pos, alb = pe.guides(w, h, pe.shape_seed(w, h))
        assert obj.shape == (h, w) and acc.shape == nd.shape == pos.shape == alb.shape == (h, w, 4)
        assert obj[0, 0] >= 0 and np.isfinite(acc).all() and np.isfinite(pos).all() and np.isfinite(nd[obj >= 0]).all()
        assert (acc[..., :3] > 0).all()
    assert sum((pe.guides(w, h, pe.shape_seed(w, h))[1] < 0).sum() for w, h in SHAPES) > 50


def test_around_and_upsample_reference_at_every_shape():
    compared = left_out = 0
    for w, h in SHAPES:
        acc, obj, nd, pos, _ = pe.guides(w, h, pe.shape_seed(w, h))
        for steps in pe.UPSAMPLE_STEPS:
            y0, y1, fy = up.around(h, steps, 0)
            assert np.all(y0 <= np.arange(h)) and np.all(y0 % steps == 0) and np.all((y1 < 0) | (y1 > np.arange(h)))
            assert np.all((fy >= 0) & (fy < 1)) and np.all(y1 < h)
            for stripe in dict.fromkeys(pe.upsample_stripes(w)):
                x0, x1, fx = up.around(w, steps, stripe)
                xs = np.arange(w)
                s = stripe if 0 < stripe < w else w
                assert np.all(x0 <= xs) and np.all((x0 - xs // s * s) % steps == 0) and np.all(x0 // s == xs // s)
                assert np.all((x1 < 0) | ((x1 > xs) & (x1 < w))) and np.all((fx >= 0) & (fx < 1))
                for sn, sx in pe.UPSAMPLE_SIGMAS:
                    ref, anchor, solved = up.reference(acc, obj, nd, pos, steps, stripe, sn, sx)
                    fin = np.isfinite(ref[..., :3]).all(-1)
                    compared += int((solved & fin).sum())
                    left_out += int((solved & ~fin).sum())
                    assert anchor[0, 0] and not (anchor & solved).any()
                    assert np.array_equal(ref[~solved], acc[~solved].astype(np.float64))
                    assert np.array_equal(ref[..., 3], acc[..., 3].astype(np.float64))
                    if steps == 1:
                        assert anchor.all() and np.array_equal(ref, acc.astype(np.float64))
                    if steps >= max(w, h) and (stripe == 0 or stripe >= w):
                        assert anchor.sum() == 1  # one block: every pixel takes the one anchor or keeps its colour
    assert left_out == 0 and compared > 50000


def test_upsample_reference_on_the_tie_guides():
    acc, obj, nd, pos = pe.upsample_tie_guides()
    plain, anchor, plain_solved = up.reference(acc, obj, nd, pos, pe.TIE_STEPS, pe.TIE_STRIPE, 0.0, 0.0)
    perp = obj == pe.TIE_PERP
    assert (perp & anchor).sum() >= 6 and (perp & ~anchor).sum() > 40
    assert {float(nd[obj == k][0, 3]) for k in range(pe.TIE_PERP)} == {2.5, 0.0, -2.0, pe.f32(1e-38), pe.INF}
    for sn in pe.TIE_SIGMA_NORMAL:
        for sx in pe.TIE_SIGMA_PLANE:
            with np.errstate(all="raise", under="ignore"):  # (no 0 / 0, inf * 0 or overflow on the way)
                ref, _, solved = up.reference(acc, obj, nd, pos, pe.TIE_STEPS, pe.TIE_STRIPE, sn, sx)
            assert np.isfinite(ref).all(), (sn, sx)
            # every weight is exactly b_q or exactly 0: the plain bilinear mix, and nothing on the perpendicular object
            assert np.array_equal(solved, plain_solved & ~perp), (sn, sx)
            assert np.array_equal(ref[solved], plain[solved]), (sn, sx)
            assert solved.sum() > 300


def test_resolve_at_every_shape():
    compared = 0
    for w, h in SHAPES:
        for k in (1, 2, 3, 4):
            c, obj, sub, _ = pe.antialias_inputs(w, h, k)
            ref, foreign, changed = resolve(c, obj, sub)
            assert np.isfinite(ref).all(), (w, h, k)
            assert np.array_equal(ref[~changed], c[~changed].astype(np.float64))
            assert np.array_equal(ref[..., 3], c[..., 3].astype(np.float64))
            assert not (changed & ~foreign).any()
            if k == 1 or (w, h) == (1, 1):
                assert not changed.any(), (w, h, k)
            compared += int(changed.sum())
    assert compared > 500


def test_variance_definition_at_every_shape():
    for w, h in SHAPES + [(255, 1), (16, 16), (257, 1)]:
        _, obj, _, _, alb = pe.guides(w, h, pe.shape_seed(w, h))
        a, b = pe.halves(w, h, 5, alb)
        for albedo in (False, True):
            v, mean = vr.variance(a, b, obj, alb, albedo)
            assert np.isfinite(v).all() and np.isfinite(mean).all() and (v >= 0).all()
            assert not v[obj < 0].any() and (v[obj >= 0] > 0).any()
            assert not vr.variance(a, a.copy(), obj, alb, albedo)[0].any(), "equal halves"
            assert np.array_equal(vr.variance(b, a, obj, alb, albedo)[0], v), "swapped halves"


def test_filter_definitions_at_every_shape():
    compared = left_out = 0
    for w, h in SHAPES:
        acc, obj, nd, pos, alb = pe.guides(w, h, pe.shape_seed(w, h))
        var = pe.variance_field(w, h, 9)
        hit = obj >= 0
        g = vr.prefilter(np.where(hit, var.astype(np.float64), 0.0), obj)
        assert np.isfinite(g).all() and np.all(g[hit] >= var[hit].min() * (1 - 1e-12)) and np.all(g[hit] <= var[hit].max() * (1 + 1e-12))
        out = {}
        for levels in pe.FILTER_LEVELS + [5]:
            for albedo in (False, True):
                for sl in pe.FILTER_SIGMAS:
                    ref = vr.denoise_variance(acc, var, obj, nd, pos, alb, levels, sl, 32.0, 0.02, albedo)
                    fin = np.isfinite(ref[..., :3]).all(-1)
                    compared += int((hit & fin).sum())
                    left_out += int((hit & ~fin).sum())
                    assert np.array_equal(ref[~hit], acc[~hit].astype(np.float64)) and np.array_equal(ref[..., 3], acc[..., 3].astype(np.float64))
                    out[(levels, albedo, sl)] = ref
                    if sl == 0.0:
                        assert np.array_equal(ref, dn.reference(acc, obj, nd, pos, alb, levels, 0.0, 32.0, 0.02, albedo)), (w, h, levels, albedo)
        if max(w, h) == 300:
            for albedo in (False, True):
                for sl in pe.FILTER_SIGMAS:
                    d = np.abs(out[(8, albedo, sl)] - out[(5, albedo, sl)])[hit][:, :3] / out[(5, albedo, sl)][hit][:, :3]
                    assert d.max() > 1e-3, (w, h, albedo, sl, "levels 6 to 8 change nothing")
    assert left_out == 0 and compared > 40000


def test_seam_inputs_and_their_definition():
    for w, h in pe.SEAM_SHAPES:
        for kind in pe.SEAM_MAPS:
            acc, var, obj, nd, pos, alb = pe.seam_inputs(w, h, kind)
            hit = obj >= 0
            assert hit.sum() > 0.5 * w * h and (hit & (obj % 2 == 1)).sum() > 20 and (hit & (obj % 2 == 0)).sum() > 20
            assert var.max() / var.min() > 1e5
            if kind in ("vertical", "seam misses"):
                for x in (8, 16, 17):
                    if x < w:
                        assert np.all((obj[:, x] != obj[:, x - 1]) | (obj[:, x] < 0)), (kind, x)
            if kind in ("horizontal", "seam misses"):
                for y in (8, 16, 17):
                    if y < h:
                        assert np.all((obj[y, :] != obj[y - 1, :]) | (obj[y, :] < 0)), (kind, y)
            if kind == "seam misses":
                assert (~hit).sum() > 20
            for levels in (1, 3):
                ref = vr.denoise_variance(acc, var, obj, nd, pos, alb, levels, 4.0, 32.0, 0.02, False)
                assert np.isfinite(ref).all(), (w, h, kind, levels)
            # a variance shifted by one pixel (a wrong apron or tile origin) moves the result by far more than the tolerance
            shifted = vr.denoise_variance(acc, np.roll(var, 1, axis=1), obj, nd, pos, alb, 1, 4.0, 32.0, 0.02, False)
            one = vr.denoise_variance(acc, var, obj, nd, pos, alb, 1, 4.0, 32.0, 0.02, False)
            moved = np.abs(shifted - one)[hit][:, :3] / one[hit][:, :3]
            if kind != "checker1":  # (every tap of another object: the filter is the identity there)
                assert (moved.max(-1) > 100 * dn.REL_TOL).mean() > 0.3, (w, h, kind)


def test_extreme_inputs_and_their_definition():
    acc, obj, nd, pos, alb = pe.extreme_inputs()
    hit = obj >= 0
    lum = vr.lum(acc[..., :3].astype(np.float64))
    d = np.abs(lum[:, 1:] - lum[:, :-1])
    assert ((d == 0) | (d >= 0.05)).all() and (d == 0).mean() > 0.3 and (d >= 0.05).mean() > 0.2  # exact ties next to distinct values
    names = [n for n, _ in pe.extreme_variances()]
    assert len(names) == len(pe.EXT_VARIANCES) + 2
    assert pe.variance_opens(pe.INF, 1.0) and pe.variance_opens(1.0, pe.INF) and not pe.variance_opens(0.0, pe.INF)
    assert not pe.variance_opens(1.0, 1.0) and pe.variance_opens(pe.f32(1e30), pe.F32_MAX)
    for name, var in pe.extreme_variances():
        for levels in pe.EXT_LEVELS:
            off = vr.denoise_variance(acc, var, obj, nd, pos, alb, levels, 0.0, 0.0, 0.0, False)
            for sl in pe.EXT_SIGMAS:
                ref = vr.denoise_variance(acc, var, obj, nd, pos, alb, levels, sl, 0.0, 0.0, False)
                assert np.isfinite(ref[hit]).all(), (name, levels, sl)
                rel = lambda a, b: np.max(np.abs(a - b)[..., :3] / np.abs(b[..., :3]), axis=-1)  # noqa: E731
                closed = hit & (var == 0)
                opened = hit & np.vectorize(pe.variance_opens)(var, sl)
                assert rel(ref, acc.astype(np.float64))[closed].max(initial=0.0) <= 1e-12, (name, levels, sl)
                assert rel(ref, off)[opened].max(initial=0.0) <= 1e-12, (name, levels, sl)


def test_motion_reference_at_every_shape(srt):
    hits = checked = blended = 0
    for w, h in SHAPES:
        for params in pe.MOTION_PARAMS:
            n, max_samples, sigma_t, thr = params
            hist = prev = None
            for k, (lists, spheres, cam, (obj, nd, pos), acc) in enumerate(pe.motion_sequence(srt, w, h, seed=w + 7 * h)):
                delta, keep = pe.sphere_table(prev if prev is not None else spheres, spheres)
                assert (k == 0) == (not np.any(delta != 0))
                with np.errstate(all="ignore"):
                    ref, L, sens, scale, sw, _, mv, ok = mo.motion_reference(acc, obj, nd, pos, hist, delta, keep, n, max_samples, sigma_t, thr)
                    if hist is not None:  # an all-zero table is the plain temporal definition
                        zero = mo.motion_reference(acc, obj, nd, pos, hist, np.zeros_like(delta), keep, n, max_samples, sigma_t, thr)
                        plain = tp.reference(acc, obj, nd, pos, hist, n, max_samples, sigma_t, thr)
                        assert all(np.array_equal(a, b) for a, b in zip(zero[:6], plain))
                hit = obj >= 0
                assert np.isfinite(ref).all() and np.isfinite(L).all() and np.isfinite(mv).all(), (w, h, k)
                hits += int(hit.sum())
                checked += int((hit & ~sens).sum())
                blended += int((hit & ~sens & (sw > 0)).sum())
                # the history the next frame reads: the definition's own result
                color = acc.copy()
                color[..., :3] = ref
                hist = dict(cam=cam, color=color, L=L.astype(np.float32), obj=obj, nd=nd, pos=pos)
                prev = spheres
    print("motion reference: %d hit, %d decided, %d blended" % (hits, checked, blended))
    assert hits - checked <= 0.01 * hits and checked > 4000 and blended > 0.3 * checked


def test_motion_reference_beyond_the_table_and_at_extreme_displacements(srt):
    w, h = 37, 21
    cam = tp.camera(srt, (0.0, 0.0, 0.0), 0.0, 55)
    obj, nd, pos = mo._cast(cam, w, h, mo.BASE)
    rng = np.random.default_rng(1)
    acc = rng.uniform(0.02, 3.0, (h, w, 4)).astype(np.float32)
    hist = dict(cam=cam, color=rng.uniform(0.02, 3.0, (h, w, 4)).astype(np.float32), L=np.where(obj >= 0, 1.0, 0.0).astype(np.float32), obj=obj,
                nd=nd, pos=pos)
    zero, keep = np.zeros((4, 3), np.float32), np.ones(4, bool)
    plain = tp.reference(acc, obj, nd, pos, hist, 1, 32.0, 0.02, 0.9)
    # indices beyond the table: delta = 0, keep = 1
    far = obj.copy()
    far[obj == 0] = np.array([4, 9, 2 ** 30], np.int32)[np.arange((obj == 0).sum()) % 3]
    hist_far = dict(hist, obj=far)
    moved = zero.copy()
    moved[1:] = 0.1
    got = mo.motion_reference(acc, far, nd, pos, hist_far, moved, keep, 1, 32.0, 0.02, 0.9)
    ground = obj == 0
    # (the relabelled neighbours of a pixel no longer count as its taps; under a still camera their weights are about 1e-7)
    assert np.allclose(got[0][ground], plain[0][ground], rtol=1e-5) and np.allclose(got[1][ground], plain[1][ground], rtol=1e-5)
    assert (got[4][ground] > 0.99).mean() > 0.9
    # displacements: 1e-30 vanishes, 1e30 and inf leave the object without history and without a motion vector
    for step, same in ((pe.f32(1e-30), True), (pe.f32(1e30), False), (pe.INF, False)):
        delta = zero.copy()
        delta[2, 1] = step
        with np.errstate(all="ignore"):
            out = mo.motion_reference(acc, obj, nd, pos, hist, delta, keep, 1, 32.0, 0.02, 0.9)
        assert np.isfinite(out[0]).all() and np.isfinite(out[6]).all()
        own = obj == 2
        assert all(np.array_equal(a[~own], b[~own]) for a, b in zip(out[:2], plain[:2]))
        if same:
            assert all(np.array_equal(a, b) for a, b in zip(out[:6], plain))
        else:
            assert not out[4][own].any() and not out[7][own].any() and not out[6][own].any()
            assert np.array_equal(out[0][own], acc[own][:, :3].astype(np.float64)) and np.all(out[1][own] == 1)


def _definition_run(frames, params, also_checked=None):
    """motion_reference along `frames` of (obj, nd, pos, cam, acc, delta, keep), each frame's history the definition's own result
    of the frame before.  Returns the last frame's outputs and, over the frames after the first, (left out, hit)."""
    n, max_samples, sigma_t, thr = params
    hist, left, hits, out = None, 0, 0, None
    for k, (obj, nd, pos, cam, acc, delta, keep) in enumerate(frames):
        with np.errstate(all="ignore"):
            out = mo.motion_reference(acc, obj, nd, pos, hist, delta, keep, n, max_samples, sigma_t, thr)
        ref, L, sens = out[0], out[1], out[2]
        assert np.isfinite(ref).all() and np.isfinite(L).all() and np.isfinite(out[6]).all()
        hit = obj >= 0
        if k:
            undecided = hit & sens
            if also_checked is not None:
                undecided &= ~also_checked
            left, hits = left + int(undecided.sum()), hits + int(hit.sum())
        color = acc.copy()
        color[..., :3] = ref
        hist = dict(cam=cam, color=color, L=L.astype(np.float32), obj=obj, nd=nd, pos=pos)
    return out, left, hits


def _edge_frames(srt, relabel=None):
    prev = None
    for lists, spheres, cam, (obj, nd, pos), acc in pe.motion_sequence(srt, pe.EDGE_W, pe.EDGE_H, seed=23, frames=pe.EDGE_FRAMES):
        delta, keep = pe.sphere_table(prev if prev is not None else spheres, spheres)
        yield (relabel(obj, pos) if relabel else obj), nd, pos, cam, acc, delta, keep
        prev = spheres


def test_the_37x21_motion_cases_leave_out_at_most_one_percent(srt):
    """The caps of test_moving_objects_parameter_extremes, test_object_indices_beyond_the_motion_table and
    test_displacement_extremes, on the definition alone."""
    for params in pe.TEMPORAL_EXTREMES:
        out, left, hits = _definition_run(_edge_frames(srt), params)
        assert left <= 0.01 * hits and hits > 800, (params, left, hits)
        obj = list(_edge_frames(srt))[-1][0]
        blended = (obj >= 0) & ~out[2] & (out[4] > 0)
        if params[2] < 1e-30 or params[3] >= 1.0:
            assert blended.sum() > 250 and not blended[obj != 0].any(), params  # the ground's exact ties, nothing else
        else:
            assert blended.sum() > 0.9 * ((obj >= 0) & ~out[2]).sum(), params
    cnt = 4
    out, left, hits = _definition_run(_edge_frames(srt, lambda o, p: pe.relabel_beyond(o, p, cnt)), pe.EDGE_PARAMS)
    obj = pe.relabel_beyond(*[list(_edge_frames(srt))[-1][i] for i in (0, 2)], cnt)
    beyond = obj >= cnt
    assert left <= 0.01 * hits and all((obj == i).sum() > 30 for i in (cnt, cnt + 5, 2 ** 30))
    assert ((out[1] > 1) & beyond & ~out[2]).sum() > 0.8 * (beyond & ~out[2]).sum() > 150
    for step in pe.DISPLACEMENTS:
        cams, guides, accs, moved = pe.displacement_frames(srt, step)
        own = guides[1][0] == 1
        zero = (np.zeros((4, 3), np.float32), np.ones(4, bool))
        frames = [(*guides[0], cams[0], accs[0], *zero), (*guides[1], cams[1], accs[1], *pe.sphere_table(mo.BASE, moved))]
        out, left, hits = _definition_run(frames, pe.EDGE_PARAMS, also_checked=own if step >= 1.0 else None)
        assert left <= 0.01 * hits and hits > 400 and own.sum() > 40, (step, left, hits)
        if step < 1.0:
            assert (out[1][own] == 2).mean() > 0.8, step
        else:  # no history and no motion vector on the object whose history point was thrown out of the window
            assert np.all(out[1][own] == 1) and not out[4][own].any() and not out[6][own].any() and not out[7][own].any(), step
