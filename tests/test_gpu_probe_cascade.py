"""Probe-cascade shading (srt_set_probe_cascade, srt_write_ / srt_bind_ / srt_capture_probe_cascade_level, srt_shade_probe_cascade,
srt_get_probe_cascade_work; ABI 7) on the MI355X.  Every comparison is bit for bit over all four lanes of every pixel, plus the work
record.  One level must be the single-grid calls as the device computes them; a level that holds nothing, or everything, leaves the
other level's single-grid call; synthetic guides put a pixel into every class of rule C2 and tiles on both sides of a trip boundary;
the real frame, the capture, bands, the bound output slot, the order of the errors, and what the call leaves alone go against
tests/probe_cascade_reference.py."""
import ctypes as C
import itertools
import types

import numpy as np
import pytest

import probe_cascade_reference as PC
import probe_grid_reference as PG
import probe_states_reference as PS
from test_gpu_probe_grid import H, SENTINEL, W, check as check_exact, covering_grid, random_coefficients, same, with_albedo
from test_gpu_probe_grid_depth import check as check_depth, synthetic_moments
from test_gpu_probe_grid_states import check as check_states, random_records
from test_gpu_visibility import Frame, scene1

pytestmark = pytest.mark.gpu

F = np.float32
FLAGS = [sum(c) for k in range(3) for c in itertools.combinations((PC.NORMAL_WEIGHT, PC.ALBEDO), k)]  # none, NORMAL_WEIGHT, ALBEDO, both
COUNTS = ("pixels", "evaluations", "blended", "first_level", "corners", "open", "wave_trips")
# test 4: the cascade around the centroid of the frame's hit points.  The 295 hit points of the 24 x 20 Scene1 frame span
# [-22, 22] x [-2, 3.7] x [2.3, 38.6] around the centroid (0.24, -0.57, 6.05); with these levels (half extents 3 x 2 x 3, twice and
# four times that) 42 of them lie in the finest level alone, 73 + 17 in the two bands, 35 in the coarsest level and 16 outside it.
REAL_BASE_SPACING, REAL_COUNTS = (1.0, 1.0, 1.0), (7, 5, 7)


def kwargs(flags):
    return dict(normal_weight=bool(flags & PC.NORMAL_WEIGHT), albedo=bool(flags & PC.ALBEDO), depth=bool(flags & PC.DEPTH), states=bool(flags & PC.STATES))


def parent_flags(flags):
    return (PG.NORMAL_WEIGHT if flags & PC.NORMAL_WEIGHT else 0) | (PG.ALBEDO if flags & PC.ALBEDO else 0)


def load(pt, cas, coeff, rec=None, mom=None):
    """The cascade and its levels' arrays, written from the host."""
    pt.set_probe_cascade([(g.origin, g.spacing, g.counts) for g in cas.grids], cas.resolution, float(cas.blend_cells))
    for l in range(cas.levels):
        pt.write_probe_cascade_level(l, "coefficients", coeff[l])
        if rec is not None:
            pt.write_probe_cascade_level(l, "records", rec[l])
        if mom is not None:
            pt.write_probe_cascade_level(l, "moments", mom[l])


def check(fr, cas, coeff, rec, mom, flags, rows=None, **kw):
    """One counting call on the loaded cascade against the reference; returns (image, work, info)."""
    pt = fr.pt
    want, wwork, info = PC.shade(cas, coeff, fr.obj, fr.nd, fr.pos, records=rec, moments=mom, albedo=getattr(fr, "alb", None), flags=flags, rows=rows, **kw)
    pt.shade_probe_cascade(count_work=True, rows=rows, **kwargs(flags), **{k: v for k, v in kw.items() if k in ("band_weight", "bias", "min_variance")})
    got, work = pt.probe_grid_output(), pt.probe_cascade_work()
    print("flags %d rows %s: work %s" % (flags, rows, work))
    hh = fr.obj.shape[0]
    y0, y1 = (0, hh) if rows is None else (hh - rows[1], hh - rows[0])
    assert same(got[y0:y1], want[y0:y1]), "differs from the reference at %d pixels" % int((got[y0:y1].view(np.uint32) != want[y0:y1].view(np.uint32)).any(axis=-1).sum())
    assert work["valid"] == 1 and work["waves"] > 0 and {k: work[k] for k in COUNTS} == {k: wwork[k] for k in COUNTS}, (work, wwork)
    return got, work, info


@pytest.fixture(scope="module")
def frame1(srt, oracle):
    fr = with_albedo(Frame(srt, oracle, scene1(oracle)))
    assert fr.hits == 295
    yield fr
    fr.close()


# ---- 1. one level is the parent --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
def test_one_level_is_the_single_grid_calls(frame1, flags):
    fr, pt = frame1, frame1.pt
    grid = covering_grid(fr, (4, 3, 5))
    coeff = random_coefficients(grid.probes)
    zero = np.zeros((grid.probes, 4), dtype=F)
    rnd = random_records(fr, grid)
    pf = parent_flags(flags)
    shared = lambda w: (w["pixels"], w["corners"], w["open"], w["wave_trips"])
    for R in (0, 4, 16):
        cas = PC.Cascade([grid], 1.0, R)
        mom = synthetic_moments(grid.probes, R) if R else None
        # without records: srt_shade_probe_grid without the visibility flag, or srt_shade_probe_grid_depth
        parent, pwork = check_exact(fr, grid, coeff, pf) if not R else check_depth(fr, grid, coeff, mom, R, pf)[:2]
        load(pt, cas, [coeff], [zero], [mom] if R else None)
        got, work, _ = check(fr, cas, [coeff], None, [mom] if R else None, flags | (PC.DEPTH if R else 0))
        assert same(got, parent) and shared(work) == shared(pwork) and work["evaluations"] == work["pixels"] and work["blended"] == 0
        assert work["first_level"] == [work["pixels"], 0, 0, 0]
        # zero and random records: srt_shade_probe_grid_states
        for rec in (zero, rnd):
            parent, pwork, _ = check_states(fr, grid, coeff, rec, pf, depth=mom, R=R if R else None)
            pt.write_probe_cascade_level(0, "records", rec)
            got, work, _ = check(fr, cas, [coeff], [rec], [mom] if R else None, flags | PC.STATES | (PC.DEPTH if R else 0))
            assert same(got, parent) and shared(work) == shared(pwork)


# ---- 2. a level that holds nothing, a level that holds everything ----------------------------------------------------------------------
def test_a_level_that_holds_nothing_and_one_that_holds_everything(frame1):
    fr, pt = frame1, frame1.pt
    outer = covering_grid(fr, (4, 3, 5))
    far = PG.Grid((1000.0, 1000.0, 1000.0), (0.5, 0.5, 0.5), (3, 4, 2))  # no hit point lies here
    co_outer, co_far = random_coefficients(outer.probes, 31), random_coefficients(far.probes, 32)
    parent, pwork = check_exact(fr, outer, co_outer, PG.NORMAL_WEIGHT)
    cas = PC.Cascade([far, outer], 1.0, 0)
    load(pt, cas, [co_far, co_outer])
    got, work, info = check(fr, cas, [co_far, co_outer], None, None, PC.NORMAL_WEIGHT)
    assert same(got, parent) and work["first_level"] == [0, fr.hits, 0, 0] and work["evaluations"] == fr.hits and work["corners"] == pwork["corners"]
    # level 0 covers every hit point by more than blend_cells cells: two cells of margin on every side, blend_cells = 0.5
    p = fr.pos[fr.obj != -1][:, :3].astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    counts = (8, 7, 9)
    spacing = (hi - lo) / (np.array(counts) - 5)
    inner = PG.Grid(lo - 2 * spacing, spacing, counts)
    co_inner = random_coefficients(inner.probes, 33)
    assert PC.level_weight(inner, 0.5, p.astype(F)).min() == 1.0  # the condition on the grid
    parent, pwork = check_exact(fr, inner, co_inner, PG.ALBEDO)
    cas = PC.Cascade([inner, far], 0.5, 0)
    load(pt, cas, [co_inner, co_far])
    got, work, info = check(fr, cas, [co_inner, co_far], None, None, PC.ALBEDO)
    assert same(got, parent) and work["first_level"] == [fr.hits, 0, 0, 0] and work["blended"] == 0 and work["corners"] == pwork["corners"]


# ---- 3. every class, synthetic guides --------------------------------------------------------------------------------------------------
def _points(rng, n, lo, hi):
    """n points whose max-norm distance from (0, 0, 4) is uniform in [lo, hi)."""
    v = rng.uniform(-1.0, 1.0, (n, 3))
    v /= np.abs(v).max(axis=1, keepdims=True)
    return (v * rng.uniform(lo, hi, (n, 1)) + np.array([0.0, 0.0, 4.0])).astype(F)


def _cascade3():
    return PC.Cascade([PG.Grid((-2.0 * s, -2.0 * s, 4.0 - 2.0 * s), (s, s, s), (5, 5, 5)) for s in (0.5, 1.0, 2.0)], 1.0, 8)


# per tile (hit pixels, of which blended): Q = hits + blended evaluations
TILES = {0: (0, 0), 1: (1, 0), 8: (5, 3), 9: (6, 3), 64: (40, 24), 65: (33, 32), 127: (64, 63), 128: (64, 64)}


@pytest.mark.parametrize("qs", [(0, 1), (8, 9), (64, 65), (127, 128)])
def test_every_class_on_synthetic_guides_and_tiles_on_both_sides_of_a_trip_boundary(srt, oracle, qs):
    """24 x 8: two tiles with Q = qs evaluations, one or two per hit pixel, scattered over the lanes, and a third tile that holds every
    class: points at max-norm distance d from the cascade's centre in [0, 0.5) (level 0 alone), (0.5, 1) (blended 0 / 1), [1, 2)
    (blended 1 / 2; exactly 1, a face of level 0, is level 1 alone), [2, 4) (the coarsest level alone) and >= 4 (outside), one NaN
    point, one pixel with all sixteen corners buried and one with only its fine level's eight."""
    import torch

    from test_gpu_visibility import one_pixel_scene

    w, h = 24, 8
    rng = np.random.default_rng(60 + sum(qs))
    cas = _cascade3()
    obj = np.full((h, w), -1, np.int32)
    pos = np.zeros((h, w, 4), F)
    for tile, q in enumerate(qs):
        hits, two = TILES[q]
        lanes = 1 + rng.choice(63, hits, replace=False) if hits < 64 else np.arange(64)  # (lane 0 misses: the ranks are not the lanes)
        ys, xs = lanes >> 3, 8 * tile + (lanes & 7)
        obj[ys, xs] = 1
        order = rng.permutation(hits)
        blended, single = order[:two], order[two:]
        pts = np.empty((hits, 3), F)
        pts[blended[::2]] = _points(rng, len(blended[::2]), 0.55, 0.95)
        pts[blended[1::2]] = _points(rng, len(blended[1::2]), 1.05, 1.95)
        for k, (lo_, hi_) in enumerate(((0.0, 0.45), (2.0, 3.9), (4.1, 9.0))):
            pts[single[k::3]] = _points(rng, len(single[k::3]), lo_, hi_)
        pos[ys, xs, :3] = pts
    # the class tile: 8 points of every range, then the special ones
    cls_pts = np.concatenate([_points(rng, 8, lo_, hi_) for lo_, hi_ in ((0.0, 0.45), (0.55, 0.95), (1.05, 1.95), (2.0, 3.9), (4.1, 9.0))])
    special = np.array([(1.0, 0.2, 4.1),        # exactly on a face of level 0
                        (np.nan, 0.0, 4.0),     # a NaN point
                        (0.75, 0.1, 4.1),       # blended 0 / 1: all sixteen corners buried
                        (-0.7, -0.3, 3.8),      # blended 0 / 1: the fine level's eight buried
                        (0.0, 0.0, 1e30)], F)   # far outside
    cls_pts = np.concatenate([cls_pts, special])
    lanes = rng.choice(64, len(cls_pts), replace=False)
    ys, xs = lanes >> 3, 16 + (lanes & 7)
    obj[ys, xs] = 1
    pos[ys, xs, :3] = cls_pts
    both_buried, fine_buried = (ys[-3], xs[-3]), (ys[-2], xs[-2])
    hit = obj != -1
    pos[..., 3] = 1.0
    nrm = rng.normal(size=(h, w, 3))
    nd = np.concatenate([nrm / np.linalg.norm(nrm, axis=2, keepdims=True), np.full((h, w, 1), 3.0)], -1).astype(F)
    alb = np.concatenate([rng.uniform(0.05, 0.9, (h, w, 3)), np.zeros((h, w, 1))], -1).astype(F)
    nd[~hit], pos[~hit], alb[~hit] = np.array([0, 0, 0, np.inf], F), 0, 0
    # arrays: random coefficients, moments at R = 8, records with about 30 % buried and the two special pixels
    coeff = [random_coefficients(g.probes, 70 + l) for l, g in enumerate(cas.grids)]
    mom = [synthetic_moments(g.probes, 8, 80 + l, lo=0.2 * 2 ** l, hi=0.9 * 2 ** l) for l, g in enumerate(cas.grids)]
    rec = []
    for l, g in enumerate(cas.grids):
        r = np.zeros((g.probes, 4), F)
        r[:, :3] = rng.uniform(-0.45, 0.45, (g.probes, 3)) * g.spacing.astype(np.float64)[None, :]
        r[:, 3] = np.where(rng.random(g.probes) < 0.3, PS.BURIED, 0).astype(np.uint32).view(F)
        rec.append(r)
    corner = lambda l, yx: PG.corners(cas.grids[l], pos[yx][None, :3], nd[yx][None, :3])["probe"].reshape(-1)
    bits = [r[:, 3].view(np.uint32) for r in rec]  # (views: the records change with them)
    bits[1][corner(1, fine_buried)] &= ~np.uint32(PS.BURIED)  # its coarse level stays usable ...
    bits[0][corner(0, fine_buried)] |= PS.BURIED
    bits[0][corner(0, both_buried)] |= PS.BURIED
    bits[1][corner(1, both_buried)] |= PS.BURIED
    left = np.setdiff1d(corner(1, fine_buried), corner(1, both_buried))
    assert len(left) > 0 and not (bits[1][left] & PS.BURIED).any()  # ... through corners the other pixel does not share
    # the conditions, asserted on the reference before any comparison
    _, wwork, info = PC.shade(cas, coeff, obj, nd, pos, records=rec, moments=mom, albedo=alb, flags=PC.STATES | PC.DEPTH)
    cls = set(info["cls"].tolist())
    assert {PC.SINGLE + 0, PC.BLENDED + 0, PC.BLENDED + 1, PC.SINGLE + 2, PC.OUTSIDE, PC.SINGLE + 1} <= cls, sorted(cls)
    two = info["evaluations"] == 2
    assert (two & (info["usable"].sum(axis=1) == 1)).any() and (two & ~info["usable"].any(axis=1)).any() and (two & info["usable"].all(axis=1)).any()
    at = lambda yx: int(np.flatnonzero(info["pix"] == yx[0] * w + yx[1])[0])
    assert info["usable"][at(both_buried)].tolist() == [False, False] and info["usable"][at(fine_buried)].tolist() == [False, True]
    for tile, q in enumerate(qs):
        sel = (info["pix"] % w) // 8 == tile
        assert int(info["evaluations"][sel].sum()) == q
    assert wwork["wave_trips"] >= sum((q + 7) // 8 for q in qs)
    oarr, n = oracle.make_objects(one_pixel_scene(oracle)[0])
    pt = srt.PathTracer(w, h)
    keep = {k: torch.from_numpy(v).to("cuda:%d" % pt.device) for k, v in (("object", obj), ("normal_depth", nd), ("position", pos), ("albedo", alb))}
    torch.cuda.synchronize()
    try:
        pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
        for k, t in keep.items():
            pt.bind_gbuffer(k, t)
        fr = types.SimpleNamespace(pt=pt, obj=obj, nd=nd, pos=pos, alb=alb)
        load(pt, cas, coeff, rec, mom)
        got, _, _ = check(fr, cas, coeff, rec, mom, PC.STATES | PC.DEPTH | PC.NORMAL_WEIGHT | PC.ALBEDO)
        assert not got[both_buried].view(np.uint32).any() and not got[~hit].view(np.uint32).any()
        check(fr, cas, coeff, rec, None, PC.STATES)
        check(fr, cas, coeff, None, mom, PC.DEPTH | PC.ALBEDO, bias=0.05)
        plain, _, _ = check(fr, cas, coeff, None, None, 0)
        # garbage guides are inputs the rules define: no index leaves an array (rule C4); run once, the pass works afterwards
        keep["position"].copy_(torch.from_numpy(np.where(rng.random((h, w, 1)) < 0.5, F(np.nan), F(1e30)) * np.ones((h, w, 4), F)).to(keep["position"].device))
        torch.cuda.synchronize()
        pt.shade_probe_cascade(depth=True, states=True, count_work=True)
        assert pt.probe_cascade_work()["first_level"] == [0, 0, int(hit.sum()), 0]
        keep["position"].copy_(torch.from_numpy(pos).to(keep["position"].device))
        torch.cuda.synchronize()
        pt.shade_probe_cascade()
        assert same(pt.probe_grid_output(), plain)
    finally:
        pt.wait()
        for k in keep:
            pt.bind_gbuffer(k, None)
        pt.close()


# ---- 4. the real frame -----------------------------------------------------------------------------------------------------------------
def real_cascade(srt, fr, resolution=0):
    centre = fr.pos[fr.obj != -1][:, :3].astype(np.float64).mean(axis=0)
    k = srt.probe_cascade_grids(centre, REAL_BASE_SPACING, REAL_COUNTS, 3)
    ref = PC.grids(centre, REAL_BASE_SPACING, REAL_COUNTS, 3)
    for l in range(3):
        assert np.array_equal(np.array(k.grid[l].origin[:], F), ref.grids[l].origin) and np.array_equal(np.array(k.grid[l].spacing[:], F), ref.grids[l].spacing)
    ref.resolution = resolution
    return ref


@pytest.mark.parametrize("flags", FLAGS)
def test_the_real_frame_around_the_centroid_of_its_hit_points(srt, frame1, flags):
    fr, pt = frame1, frame1.pt
    cas = real_cascade(srt, fr, 8)
    coeff = [random_coefficients(g.probes, 90 + l) for l, g in enumerate(cas.grids)]
    mom = [synthetic_moments(g.probes, 8, 93 + l, lo=0.3 * 2 ** l, hi=1.5 * 2 ** l) for l, g in enumerate(cas.grids)]
    rec = [random_records(fr, g, 96 + l) for l, g in enumerate(cas.grids)]
    cls = PC.classes(cas, fr.pos[fr.obj != -1][:, :3])
    n_single0, n_blended, n_coarsest = int((cls == PC.SINGLE).sum()), int(((cls >= PC.BLENDED) & (cls < PC.OUTSIDE)).sum()), int(((cls == PC.SINGLE + 2) | (cls == PC.OUTSIDE)).sum())
    print("classes: single finest %d, blended %d, first level coarsest %d of %d" % (n_single0, n_blended, n_coarsest, fr.hits))
    assert min(n_single0, n_blended, n_coarsest) >= 10  # the condition on the cascade
    load(pt, cas, coeff, rec, mom)
    plain, work, _ = check(fr, cas, coeff, None, None, flags)
    assert work["blended"] == n_blended and work["first_level"][2] == n_coarsest
    full, _, _ = check(fr, cas, coeff, rec, mom, flags | PC.STATES | PC.DEPTH)
    check(fr, cas, coeff, rec, None, flags | PC.STATES)
    check(fr, cas, coeff, None, mom, flags | PC.DEPTH)
    assert not same(plain, full)
    # turning COUNT_WORK off changes no output bit, and the same call twice gives the same bits
    for _ in range(2):
        pt.shade_probe_cascade(**kwargs(flags | PC.STATES | PC.DEPTH))
        assert same(pt.probe_grid_output(), full)
    hem, _, _ = check(fr, cas, coeff, rec, mom, flags | PC.STATES | PC.DEPTH, band_weight=PG.HEMISPHERE)
    assert not same(hem, full) and same(hem[..., 3], full[..., 3])


# ---- 5. capture ------------------------------------------------------------------------------------------------------------------------
def test_capture_keeps_what_the_single_grid_calls_would_read(srt, frame1):
    fr, pt = frame1, frame1.pt
    c = srt.capi
    cas = real_cascade(srt, fr, 8)
    pt.set_probe_cascade([(g.origin, g.spacing, g.counts) for g in cas.grids], 8, 1.0)
    coeff, rec, mom = [], [], []
    try:
        for l, g in enumerate(cas.grids):
            pt.set_probe_grid(g.origin, g.spacing, g.counts)
            pt.classify_probes(directions=64, relocate=True, positions=True)
            rec.append(pt.probe_states_output("records"))
            pt.trace_light_probes(pt.probe_states_output("positions"), 64, samples=1, bounces=1, seed=5 + l)
            coeff.append(pt.light_probe_coefficients())
            pt.trace_probe_depth(resolution=8, max_distance=20.0)
            mom.append(pt.probe_depth_output("moments"))
            pt.shade_probe_grid_states(coefficients=coeff[l], states=rec[l], moments=mom[l], resolution=8)  # the single grid's current arrays
            pt.capture_probe_cascade_level(l, "all")
        # the single grid's arrays become garbage: the cascade has its own
        g = cas.grids[2]
        pt.shade_probe_grid_states(coefficients=np.full((g.probes, 9, 4), np.nan, F), states=np.full((g.probes, 4), 1e30, F),
                                   moments=np.full((g.probes, 64, 4), -1.0, F), resolution=8)
        flags = PC.STATES | PC.DEPTH | PC.NORMAL_WEIGHT | PC.ALBEDO
        got, work, _ = check(fr, cas, coeff, rec, mom, flags)
        assert got[..., 3].any()
        # a grid of other counts, or moments of another R: SRT_ERR_STATE, and the level is as it was
        pt.set_probe_grid(g.origin, g.spacing, (5, 5, 4))
        with pytest.raises(srt.SrtError) as e:
            pt.capture_probe_cascade_level(2, "coefficients")
        assert e.value.code == c.ERR_STATE and "counts" in str(e.value)
        pt.set_probe_grid(g.origin, g.spacing, g.counts)
        pt.bind_probe_grid_depth(synthetic_moments(g.probes, 4, 99), 4)
        with pytest.raises(srt.SrtError) as e:
            pt.capture_probe_cascade_level(2, "all")
        assert e.value.code == c.ERR_STATE and "resolution" in str(e.value)
        with pytest.raises(srt.SrtError) as e:
            pt.capture_probe_cascade_level(3, "all")
        assert e.value.code == c.ERR_INVALID_ARG
        with pytest.raises(srt.SrtError) as e:
            pt.capture_probe_cascade_level(0, 0)
        assert e.value.code == c.ERR_INVALID_ARG
        again, _, _ = check(fr, cas, coeff, rec, mom, flags)
        assert same(again, got)
        # a capture ends a binding: bound garbage, then the capture of the real records
        import torch

        junk = torch.full((g.probes, 4), float("nan"), dtype=torch.float32, device="cuda:%d" % pt.device)
        pt.bind_probe_cascade_level(2, "records", junk)
        pt.bind_probe_grid_states(rec[2])
        pt.capture_probe_cascade_level(2, "records")
        assert same(check(fr, cas, coeff, rec, mom, flags)[0], got)
    finally:
        pt.wait()
        pt.bind_probe_grid_states(None)
        pt.bind_probe_grid_depth(None)


# ---- 6. bands, slots, errors -----------------------------------------------------------------------------------------------------------
def test_a_band_and_a_bound_output(srt, frame1):
    import torch

    fr, pt = frame1, frame1.pt
    cas = real_cascade(srt, fr, 4)
    coeff = [random_coefficients(g.probes, 100 + l) for l, g in enumerate(cas.grids)]
    mom = [synthetic_moments(g.probes, 4, 103 + l, lo=0.3 * 2 ** l, hi=1.5 * 2 ** l) for l, g in enumerate(cas.grids)]
    rec = [random_records(fr, g, 106 + l) for l, g in enumerate(cas.grids)]
    flags = PC.STATES | PC.DEPTH | PC.ALBEDO
    load(pt, cas, coeff, rec, mom)
    full, _, _ = check(fr, cas, coeff, rec, mom, flags)
    big = torch.full((W * H + 70, 4), SENTINEL, dtype=torch.float32, device="cuda:%d" % pt.device)
    torch.cuda.synchronize()
    try:
        pt.bind_probe_grid_output(big[:W * H].view(H, W, 4))
        check(fr, cas, coeff, rec, mom, flags, rows=(0, 7))  # (the band's work counts too)
        g = big.cpu().numpy()
        img = g[:W * H].reshape(H, W, 4)
        assert same(img[H - 7:], full[H - 7:]) and np.all(img[:H - 7] == SENTINEL) and np.all(g[W * H:] == SENTINEL)
        check(fr, cas, coeff, rec, mom, flags, rows=(7, 20))
        g = big.cpu().numpy()
        assert same(g[:W * H].reshape(H, W, 4), full) and np.all(g[W * H:] == SENTINEL)
    finally:
        pt.wait()
        pt.bind_probe_grid_output(None)
    assert same(check(fr, cas, coeff, rec, mom, flags)[0], full)  # and the own buffer again


def test_errors_come_in_the_header_s_order_and_leave_the_output_untouched(srt, oracle):
    c = srt.capi
    oarr, n = oracle.make_objects(scene1(oracle)[0])
    pt = srt.PathTracer(W, H)
    L = pt.L
    fptr = C.POINTER(C.c_float)
    nan, inf = float("nan"), float("inf")

    def call(**kw):
        p = c.ProbeCascadeParams()
        assert L.srt_probe_cascade_params_default(C.byref(p)) == c.OK
        p.row_begin, p.row_end = 0, H
        for k, v in kw.items():
            if k in ("band_weight", "reserved"):
                getattr(p, k)[:] = v
            else:
                setattr(p, k, v)
        return L.srt_shade_probe_cascade(pt._h, C.byref(p))

    def why():
        return L.srt_last_error(pt._h)

    def cascade(**kw):
        k = c.probe_cascade([((-4.0, -1.2, 2.0), (2.0, 1.5, 2.0), (5, 3, 5)), ((-8.0, -2.4, 0.0), (4.0, 3.0, 4.0), (5, 3, 4))], 4, 1.0)
        for name, v in kw.items():
            setattr(k, name, v)
        return L.srt_set_probe_cascade(pt._h, C.byref(k))

    try:
        w = c.ProbeCascadeWork()
        buf = np.empty((H, W, 4), F)
        co75, co60 = random_coefficients(75, 18), random_coefficients(60, 19)
        assert call(flags=32) == c.ERR_STATE and b"srt_set_scene" in why()  # 1. before srt_set_scene, whatever the arguments
        pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
        # 2. the arguments come before the cascade
        for kw in (dict(row_begin=-1), dict(row_end=H + 1), dict(row_begin=7, row_end=7), dict(row_begin=9, row_end=3), dict(flags=32), dict(flags=0x80000001),
                   dict(reserved=(1, 0)), dict(reserved=(0, 1)), dict(band_weight=(nan, 1, 1)), dict(band_weight=(1, nan, 1)), dict(band_weight=(1, 1, nan)),
                   dict(flags=c.PROBE_CASCADE_DEPTH, bias=nan), dict(flags=c.PROBE_CASCADE_DEPTH, bias=-1.0), dict(flags=c.PROBE_CASCADE_DEPTH, min_variance=nan),
                   dict(flags=c.PROBE_CASCADE_DEPTH, min_variance=-1e-9)):
            assert call(**kw) == c.ERR_INVALID_ARG, kw
        assert call(bias=nan, min_variance=-1.0) == c.ERR_STATE and b"no cascade" in why()  # (read only with _DEPTH)  3. no cascade
        # cascades that are none are refused and leave none
        for kw in (dict(levels=0), dict(levels=5), dict(resolution=3), dict(blend_cells=0.0), dict(blend_cells=nan), dict(blend_cells=inf), dict(reserved=1)):
            assert cascade(**kw) == c.ERR_INVALID_ARG, kw
        k = c.probe_cascade([((0, 0, 0), (1, 1, 1), (3, 3, 3)), ((0, 0, 0), (1, 0, 1), (3, 3, 3))])
        assert L.srt_set_probe_cascade(pt._h, C.byref(k)) == c.ERR_INVALID_ARG and L.srt_set_probe_cascade(pt._h, None) == c.ERR_INVALID_ARG
        assert call() == c.ERR_STATE and b"no cascade" in why()
        assert L.srt_write_probe_cascade_level(pt._h, 0, 1, co75.ctypes.data_as(fptr), 75) == c.ERR_STATE
        assert L.srt_capture_probe_cascade_level(pt._h, 0, 1) == c.ERR_STATE
        assert cascade() == c.OK
        assert call() == c.ERR_STATE and b"OBJECT" in why()  # 4. the guides come before the levels' arrays
        pt.set_camera(srt.default_camera())
        for have, missing in ((["object"], b"NORMAL_DEPTH"), (["object", "normal_depth"], b"POSITION")):
            pt.render_gbuffer(outputs=have)
            assert call() == c.ERR_STATE and missing in why()
        pt.render_gbuffer(outputs=["object", "normal_depth", "position"])
        assert call(flags=c.PROBE_CASCADE_ALBEDO) == c.ERR_STATE and b"ALBEDO" in why()
        # 5. per level ascending
        assert call() == c.ERR_STATE and b"no coefficients" in why()
        for level, which, probes in ((2, 1, 75), (0, 3, 75), (0, 0, 75), (0, 8, 75), (0, 1, 0), (0, 1, (1 << 30) + 1)):
            assert L.srt_write_probe_cascade_level(pt._h, level, which, co75.ctypes.data_as(fptr), probes) == c.ERR_INVALID_ARG, (level, which, probes)
            assert L.srt_bind_probe_cascade_level(pt._h, level, which, 4096, probes) == c.ERR_INVALID_ARG, (level, which, probes)
        assert L.srt_write_probe_cascade_level(pt._h, 0, 1, None, 75) == c.ERR_INVALID_ARG and L.srt_bind_probe_cascade_level(pt._h, 0, 1, None, 75) == c.ERR_INVALID_ARG
        assert L.srt_write_probe_cascade_level(pt._h, 0, 1, co75.ctypes.data_as(fptr), 74) == c.OK  # one probe short
        assert call() == c.ERR_STATE and b"coefficient count" in why()
        assert L.srt_write_probe_cascade_level(pt._h, 0, 1, co75.ctypes.data_as(fptr), 75) == c.OK
        assert call() == c.ERR_STATE and b"no coefficients" in why()  # level 1
        assert call(flags=c.PROBE_CASCADE_DEPTH | c.PROBE_CASCADE_STATES) == c.ERR_STATE and b"no moments" in why()  # level 0's moments before level 1's coefficients
        mo = synthetic_moments(75, 4, 26)
        assert L.srt_write_probe_cascade_level(pt._h, 0, 2, mo.ctypes.data_as(fptr), 70) == c.OK
        assert call(flags=c.PROBE_CASCADE_DEPTH | c.PROBE_CASCADE_STATES) == c.ERR_STATE and b"moment probe count" in why()
        assert L.srt_write_probe_cascade_level(pt._h, 0, 2, mo.ctypes.data_as(fptr), 75) == c.OK
        assert call(flags=c.PROBE_CASCADE_DEPTH | c.PROBE_CASCADE_STATES) == c.ERR_STATE and b"no records" in why()
        rec = np.zeros((75, 4), F)
        assert L.srt_write_probe_cascade_level(pt._h, 0, 4, rec.ctypes.data_as(fptr), 75) == c.OK
        assert call(flags=c.PROBE_CASCADE_DEPTH | c.PROBE_CASCADE_STATES) == c.ERR_STATE and b"no coefficients" in why()  # level 1
        assert L.srt_write_probe_cascade_level(pt._h, 1, 1, co60.ctypes.data_as(fptr), 60) == c.OK
        assert call(flags=c.PROBE_CASCADE_STATES) == c.ERR_STATE and b"no records" in why()
        assert cascade(resolution=0) == c.OK  # (only the moments go)
        assert call(flags=c.PROBE_CASCADE_DEPTH) == c.ERR_STATE and b"resolution is 0" in why()
        assert L.srt_write_probe_cascade_level(pt._h, 0, 2, mo.ctypes.data_as(fptr), 75) == c.ERR_INVALID_ARG
        # nothing was touched: there is no output and no work record yet
        assert L.srt_read_probe_grid_output(pt._h, buf.ctypes.data_as(fptr)) == c.ERR_STATE and L.srt_get_probe_cascade_work(pt._h, C.byref(w)) == c.ERR_STATE
        assert call() == c.OK
        good = pt.probe_grid_output()
        assert good[..., 3].any() and L.srt_get_probe_cascade_work(pt._h, C.byref(w)) == c.ERR_STATE  # (the call did not count)
        # a refused call leaves the output readable and unchanged
        assert call(flags=32) == c.ERR_INVALID_ARG and call(flags=c.PROBE_CASCADE_STATES) == c.ERR_STATE
        assert same(pt.probe_grid_output(), good)
        assert call(flags=c.PROBE_CASCADE_COUNT_WORK) == c.OK and pt.probe_cascade_work()["pixels"] == int((pt.gbuffer("object") != -1).sum())
        # a level whose probe count changes loses its arrays; the other level keeps them
        k = c.probe_cascade([((-4.0, -1.2, 2.0), (2.0, 1.5, 2.0), (5, 3, 4)), ((-9.0, -2.4, 0.0), (4.5, 3.0, 4.0), (5, 3, 4))], 0, 1.0)
        assert L.srt_set_probe_cascade(pt._h, C.byref(k)) == c.OK
        assert call() == c.ERR_STATE and b"no coefficients" in why()
        assert L.srt_write_probe_cascade_level(pt._h, 0, 1, co60.ctypes.data_as(fptr), 60) == c.OK and call() == c.OK
        assert L.srt_shade_probe_cascade(pt._h, None) == c.ERR_INVALID_ARG and L.srt_get_probe_cascade_work(pt._h, None) == c.ERR_INVALID_ARG
        pt.wait()
    finally:
        pt.close()


# ---- 7. nothing else moved -------------------------------------------------------------------------------------------------------------
def test_the_single_grid_calls_and_their_work_record_stay_what_they_were(srt, frame1):
    fr, pt = frame1, frame1.pt
    c = srt.capi
    grid = covering_grid(fr, (4, 3, 5))
    coeff = random_coefficients(grid.probes, 24)
    depth = synthetic_moments(grid.probes, 8, 30)
    rec = random_records(fr, grid, 44)
    before = [check_exact(fr, grid, coeff, 0)[0], check_depth(fr, grid, coeff, depth, 8, PG.ALBEDO)[0], check_states(fr, grid, coeff, rec, PG.NORMAL_WEIGHT, depth=depth, R=8)[0]]
    work_before = pt.probe_grid_work()
    cas = real_cascade(srt, fr, 4)
    co = [random_coefficients(g.probes, 110 + l) for l, g in enumerate(cas.grids)]
    mo = [synthetic_moments(g.probes, 4, 113 + l) for l, g in enumerate(cas.grids)]
    rc = [random_records(fr, g, 116 + l) for l, g in enumerate(cas.grids)]
    load(pt, cas, co, rc, mo)
    check(fr, cas, co, rc, mo, PC.STATES | PC.DEPTH | PC.NORMAL_WEIGHT)
    assert pt.probe_grid_work() == work_before  # the single-grid record is the last single-grid call's
    # the single grid and its bindings are what they were: the same calls without writing anything give the same bits
    pt.shade_probe_grid_states(depth=True, normal_weight=True)
    assert same(pt.probe_grid_output(), before[2])
    with pytest.raises(srt.SrtError) as e:  # ... and that call did not count, whatever the cascade call did
        pt.probe_grid_work()
    assert e.value.code == c.ERR_STATE
    pt.shade_probe_cascade(count_work=True)
    with pytest.raises(srt.SrtError) as e:
        pt.probe_grid_work()
    assert e.value.code == c.ERR_STATE and pt.probe_cascade_work()["valid"] == 1
    pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
    after = [check_exact(fr, grid, coeff, 0, write=False)[0], check_depth(fr, grid, coeff, depth, 8, PG.ALBEDO, write=False)[0],
             check_states(fr, grid, coeff, rec, PG.NORMAL_WEIGHT, depth=depth, R=8, write=False)[0]]
    assert all(same(a, b) for a, b in zip(before, after))


# ---- the layers above -----------------------------------------------------------------------------------------------------------------
def test_host_library_and_cli_give_the_bytes_of_the_c_calls(srt, frame1, tmp_path):
    import os
    import subprocess

    from conftest import ROOT, scene_path

    fr, pt = frame1, frame1.pt
    k = srt.probe_cascade_grids((0.0, 0.0, 0.0), (1.0, 0.75, 1.0), (7, 5, 7), 3)  # around the default camera's position
    grids = [PG.Grid(k.grid[l].origin[:], k.grid[l].spacing[:], k.grid[l].counts[:]) for l in range(3)]
    coeff, rec, mom = [], [], []
    for g in grids:
        pt.set_probe_grid(g.origin, g.spacing, g.counts)
        pt.classify_probes(directions=64, relocate=True, clearance=0.2, max_offset=0.4, steps=5, positions=True)
        rec.append(pt.probe_states_output("records"))
        pt.trace_light_probes(pt.probe_states_output("positions"), 64, samples=3, bounces=2, seed=13)
        coeff.append(pt.light_probe_coefficients())
        pt.trace_probe_depth(resolution=8, sharpness=4, max_distance=5.0)
        mom.append(pt.probe_depth_output("moments"))
    cas = PC.Cascade(grids, 0.5, 8)
    load(pt, cas, coeff, rec, mom)
    pt.shade_probe_cascade(depth=True, states=True, bias=0.25, normal_weight=True, albedo=True, band_weight=PG.HEMISPHERE, count_work=True)
    want, work = pt.probe_grid_output(), pt.probe_cascade_work()
    assert work["blended"] > 0 and work["first_level"][0] > 0 and work["first_level"][2] > 0 and want[..., 3].any()
    # host.py over PathTraceRenderer::setProbeCascade / captureProbeCascadeLevel / shadeProbeCascade: it renders the guides itself
    r = srt.host.Renderer(W, H)
    try:
        r.set_scene(srt.host.Scene(scene_path("Scene1")))
        r.set_probe_cascade([(g.origin, g.spacing, g.counts) for g in grids], 8, 0.5)
        for l, g in enumerate(grids):
            r.set_probe_grid(g.origin, g.spacing, g.counts)
            r.shade_probe_grid_states(coeff[l], rec[l], mom[l])  # (the single grid's current arrays)
            r.capture_probe_cascade_level(l, "all")
        got = r.shade_probe_cascade(depth=True, states=True, bias=0.25, normal_weight=True, albedo=True, band_weight=PG.HEMISPHERE, count_work=True)
        assert same(got, want) and r.probe_cascade_work() == work
    finally:
        r.close()
    # the command-line tool: the levels around the camera, each traced as --probe-grid traces its grid, captured, then the cascade
    cli = os.path.join(ROOT, "software-raytracer_amd", "srt_render")
    out = tmp_path / "irradiance.f32"
    base = [cli, "--scene", scene_path("Scene1"), "--width", str(W), "--height", str(H), "--probe-grid", "9,9,9,1,0.75,1,7,5,7", "--probe-directions", "64",
            "--radiance", "3", "--bounces", "2", "--seed", "13", "--irradiance-out", str(out), "--probe-albedo", "--probe-hemisphere"]
    run = subprocess.run(base + ["--probe-cascade", "3", "--probe-cascade-blend", "0.5", "--probe-classify", "--probe-relocate", "--probe-clearance", "0.2",
                                 "--probe-max-offset", "0.4", "--probe-steps", "5", "--probe-depth", "8", "--probe-depth-sharpness", "4", "--probe-depth-max", "5",
                                 "--probe-depth-bias", "0.25", "--probe-normal-weight"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert out.read_bytes() == want.tobytes()
    out.unlink()
    for extra in (["--probe-cascade", "0"], ["--probe-cascade", "5"], ["--probe-cascade", "2", "--probe-cascade-blend", "0"], ["--probe-cascade", "2", "--probe-visibility"],
                  ["--probe-cascade", "2", "--probe-tail"], ["--probe-cascade-blend", "1"]):
        run = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert run.returncode == 2 and "--probe-cascade" in run.stderr and not out.exists(), (extra, run.returncode, run.stderr)
    usage = subprocess.run([cli], capture_output=True, text=True, timeout=60).stderr
    assert "--probe-cascade L" in usage and "--probe-cascade-blend" in usage
