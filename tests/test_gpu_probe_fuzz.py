"""Randomized sweep, on the MI355X, of the passes that start rays or take measurements away from the camera — the reflection guides,
the light probes and their depth maps, probe classification, the four probe-grid shading calls, the probe tail and adaptive
rendering — on the scene families of tests/test_gpu_fuzz.py and tests/test_gpu_query_fuzz.py: geometry 50 000 units from the origin
(where a hit point lifted by normal * .00001f rounds back onto the surface), scales of 1e4 and 1e-2, 30x, 300x and negative radii,
probes and path ends inside spheres and far outside the grid, broken triangle soups, OBJ_NONE entries, and the 3400-sphere scene that
is read from memory.  The inputs are tests/probe_fuzz_inputs.py's; tests/test_probe_fuzz_inputs.py shows on the CPU that they are
not vacuous.

Every comparison is bit for bit in all lanes against a CPU expectation built from the oracle and the numpy references, with no
pixel, probe or ray left out (NaNs compare as NaNs); every pass is called a second time from the same state and must give the same
bits.  A failure names the key, the kind, the environment, the pass with its flags and the first ten differing elements:
probe_fuzz_inputs.build(oracle, key) rebuilds the case on the CPU, where the element can be replayed through the references.

Keys: two seeds per kind, "large" and "large-mesh"; SRT_FUZZ_PROBE_N extends the seeds.  The shading and the tail test take five more keys whose
hit points leave the grid (probe_fuzz_inputs.CLAMP_KEYS)."""
import ctypes as C
import itertools
import os
import types

import numpy as np
import pytest

import light_probe_reference as LP
import probe_cascade_reference as PC
import probe_depth_reference as PD
import probe_fuzz_inputs as pf
import probe_grid_reference as PG
import probe_states_reference as PS
import probe_tail_reference as PT
from test_gpu_adaptive import SENT_ACC, Bound, Ref, sentinels
from test_gpu_denoise import tone_map
from test_gpu_light_probes import radiance_of
from test_gpu_probe_cascade import COUNTS as CASCADE_COUNTS, kwargs as cascade_kwargs, load as load_cascade
from test_gpu_probe_tail import COUNTS as TAIL_COUNTS, set_grid, tail
from test_gpu_radiance import srt_camera

pytestmark = pytest.mark.gpu

F = np.float32
W, H, R = pf.W, pf.H, pf.R
KEYS = list(range(int(os.environ.get("SRT_FUZZ_PROBE_N", str(pf.DEFAULT_SEEDS))))) + list(pf.LARGE)
SHADING_KEYS = KEYS + [k for k in pf.CLAMP_KEYS if k not in KEYS]
GUIDES = ("object", "normal_depth", "position", "albedo")
REFLECTION = GUIDES + ("bounces",)
GRID_FLAGS = [sum(s) for k in range(4) for s in itertools.combinations((PG.VISIBILITY, PG.NORMAL_WEIGHT, PG.ALBEDO), k)]  # all eight
DEPTH_FLAGS = [0, PG.NORMAL_WEIGHT, PG.ALBEDO, PG.NORMAL_WEIGHT | PG.ALBEDO]
CASCADE_FLAGS = [0, PC.NORMAL_WEIGHT | PC.ALBEDO, PC.STATES, PC.DEPTH | PC.ALBEDO, PC.STATES | PC.DEPTH | PC.NORMAL_WEIGHT | PC.ALBEDO]
TAIL_FLAGS = {"none": 0, "NORMAL_WEIGHT": PT.NORMAL_WEIGHT, "DEPTH": PT.DEPTH, "STATES": PT.STATES}
GRID_WORK = ("pixels", "corners", "segments", "open", "wave_trips")
SHARPNESS = 3


def _tracer(srt, c):
    pt = srt.PathTracer(W, H)
    pt.set_meshes(C.cast(c.marr, C.POINTER(srt.Mesh)), c.mn)
    pt.set_scene(C.cast(c.oarr, C.POINTER(srt.Object)), c.n)
    pt.set_environment(srt.Environment.from_buffer_copy(bytes(c.env)))
    pt.set_camera(srt_camera(srt, c.cam))
    return pt


def differing(got, want, lanes=1):
    """The elements (pixels, probes, rays: the array without its last `lanes` axes, flattened) at which two arrays differ in a bit;
    NaNs compare as NaNs."""
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype.kind == "f":
        nan = np.isnan(a) | np.isnan(b)
        same = np.where(nan, np.isnan(a) & np.isnan(b), a.view(np.uint32) == b.view(np.uint32))
    else:
        same = a == b
    n = int(np.prod(a.shape[:a.ndim - lanes]))
    return np.flatnonzero(~same.reshape(n, -1).all(axis=1)), n


def check(c, what, got, want, lanes=1):
    bad, n = differing(got, want, lanes)
    assert not len(bad), "%s, %s: %d of %d elements differ from the reference, the first at %s" % (pf.where(c), what, len(bad), n, bad[:10].tolist())


def project(radiance, directions):
    """light_probe_reference.project; a NaN in the radiance (an environment with a NaN colour) is a value like any other."""
    with np.errstate(invalid="ignore", over="ignore"):
        return LP.project(radiance, directions)


def flag_names(flags, table):
    return "|".join(name for name, bit in table if flags & bit) or "0"


GRID_NAMES = (("VISIBILITY", PG.VISIBILITY), ("NORMAL_WEIGHT", PG.NORMAL_WEIGHT), ("ALBEDO", PG.ALBEDO))
CASCADE_NAMES = (("NORMAL_WEIGHT", PC.NORMAL_WEIGHT), ("DEPTH", PC.DEPTH), ("STATES", PC.STATES), ("ALBEDO", PC.ALBEDO))


def check_guides(c, pt):
    """srt_render_gbuffer gives the oracle's guides: the references below are built on the oracle's."""
    pt.render_gbuffer()
    got = {k: pt.gbuffer(k) for k in GUIDES}
    for k, want in zip(GUIDES, (c.obj, c.nd, c.pos, c.alb)):
        check(c, "srt_render_gbuffer %s" % k, got[k], want, lanes=0 if k == "object" else 1)
    return got


# ---- the reflection guides -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_reflection_guides(srt, oracle, key):
    c = pf.case(oracle, key)
    pt = _tracer(srt, c)
    try:
        first = check_guides(c, pt)
        for thr in pf.THRESHOLDS:
            what = "srt_render_reflection_gbuffer min_smoothness = min_specular = %s max_bounces %d" % (thr[0], pf.MAX_BOUNCES)
            want = pf.reflection(oracle, c, thr)
            kw = dict(max_bounces=pf.MAX_BOUNCES, min_smoothness=thr[0], min_specular=thr[1])
            pt.render_reflection_gbuffer(count_work=True, **kw)
            got, work = {k: pt.read_reflection(k) for k in REFLECTION}, pt.reflection_work()
            print("%s, thresholds %s: J histogram %s, work %s" % (pf.where(c), thr[0], np.bincount(want["bounces"].reshape(-1)).tolist(), work))
            for k in REFLECTION:
                check(c, "%s, output %s" % (what, k), got[k], want[k], lanes=0 if k in ("object", "bounces") else 1)
            assert work["valid"] == 1 and work["pixels"] == W * H and work["reflections"] == int(want["bounces"].sum()), (pf.where(c), what, work)
            if thr == (1.0, 1.0):  # nothing is as smooth as that: the first hits
                assert not want["bounces"].any()
                for k in GUIDES:
                    check(c, "%s against srt_render_gbuffer, output %s" % (what, k), got[k], first[k], lanes=0 if k == "object" else 1)
            pt.render_reflection_gbuffer(**kw)
            for k in REFLECTION:
                check(c, "%s, a second call, output %s" % (what, k), pt.read_reflection(k), got[k], lanes=0 if k in ("object", "bounces") else 1)
    finally:
        pt.close()


# ---- light probes and their depth maps ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_light_probes_and_probe_depth(srt, oracle, key):
    c = pf.case(oracle, key)
    pt = _tracer(srt, c)
    seed = c.seeds["probes"]
    try:
        # the probe at the camera, along the frame's camera directions: the oracle's accumulator
        d = c.D4.copy()
        d[:, 3] = F(4.0 * np.pi / (W * H))
        for bounces in (0, 3):
            what = "srt_trace_light_probes at the camera, 3 samples, %d bounces, seed %d" % (bounces, seed)
            _, acc, _ = oracle.render(c.oarr, c.n, c.env, c.cam, W, H, spp=3, bounces=bounces, seed=seed, meshes=(c.marr, c.mn) if c.mn else None, threads=16)
            kw = dict(samples=3, bounces=bounces, seed=seed, radiance=True)
            pt.trace_light_probes(c.probes[:1], d, **kw)
            got, coeff = pt.light_probe_radiance(), pt.light_probe_coefficients()
            check(c, what + ", RADIANCE against the oracle's accumulator", got, acc.reshape(1, W * H, 4))
            check(c, what + ", COEFFICIENTS", coeff, project(got, d))
            pt.trace_light_probes(**kw)
            check(c, what + ", a second call, RADIANCE", pt.light_probe_radiance(), got)
            check(c, what + ", a second call, COEFFICIENTS", pt.light_probe_coefficients(), coeff)
        # the other probe points: srt_trace_radiance on the explicit P * K batch
        rest = c.probes[1:]
        for bounces in (0, 3):
            what = "srt_trace_light_probes at %s, K %d, 3 samples, %d bounces, seed %d" % (pf.PROBE_NAMES[1:], pf.K, bounces, seed)
            kw = dict(samples=3, bounces=bounces, seed=seed, id_base=1000)
            want = radiance_of(pt, rest, c.dirs, **kw)
            pt.trace_light_probes(rest, c.dirs, radiance=True, **kw)
            got, coeff = pt.light_probe_radiance(), pt.light_probe_coefficients()
            check(c, what + ", RADIANCE against srt_trace_radiance", got, want)
            check(c, what + ", COEFFICIENTS", coeff, project(got, c.dirs))
            pt.trace_light_probes(radiance=True, **kw)
            check(c, what + ", a second call, RADIANCE", pt.light_probe_radiance(), got)
            check(c, what + ", a second call, COEFFICIENTS", pt.light_probe_coefficients(), coeff)
        # probe depth: the oracle's closest distance per ray, clamped, and the moments of those distances
        runs = [("unit directions", c.dirs, False, c.dirs), ("NORMALIZE on lengths 0.5 and 3", c.scaled, True, LP.normalized(c.scaled))]
        if c.scaled_unnormalized:  # (not pinned in a scene with triangles: see probe_fuzz_inputs)
            runs.append(("lengths 0.5 and 3 as given", c.scaled, False, c.scaled))
        for label, given, normalize, used in runs:
            what = "srt_trace_probe_depth R %d K %d sharpness %d max_distance %r, %s" % (R, pf.K, SHARPNESS, c.max_distance, label)
            idx, t = pf.closest(oracle, c, c.probes, used)
            r = PD.clamp_distance(t, c.max_distance)
            kw = dict(resolution=R, sharpness=SHARPNESS, max_distance=c.max_distance, normalize=normalize, distances=True)
            pt.trace_probe_depth(c.probes, given, count_work=True, **kw)
            got_r, got, work = pt.probe_depth_output("distances"), pt.probe_depth_output("moments"), pt.probe_depth_work()
            print("%s, %s: hits per probe %s, t <= 0 at %d rays, clamped at %d" % (pf.where(c), label, (idx >= 0).sum(axis=1).tolist(), int((t <= 0).sum()), int((r >= F(c.max_distance)).sum())))
            check(c, what + ", DISTANCES against the oracle", got_r, r, lanes=0)
            check(c, what + ", MOMENTS", got, PD.moments(used, r, R, SHARPNESS, c.max_distance))
            assert (work["probes"], work["rays"], work["far_rays"], work["wave_calls"]) == PD.work_formula(5, pf.K, r, c.max_distance), (pf.where(c), what, work)
            pt.trace_probe_depth(**kw)
            check(c, what + ", a second call, DISTANCES", pt.probe_depth_output("distances"), got_r, lanes=0)
            check(c, what + ", a second call, MOMENTS", pt.probe_depth_output("moments"), got)
    finally:
        pt.close()


# ---- classification --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("way", list(pf.WAYS))
@pytest.mark.parametrize("key", KEYS)
def test_probe_classification(srt, oracle, key, way):
    c = pf.case(oracle, key)
    pt = _tracer(srt, c)
    flags = pf.WAYS[way]
    relocate, normalize = bool(flags & PS.RELOCATE), bool(flags & PS.NORMALIZE)
    try:
        for which in ("grid", "flat"):
            grid = getattr(c, which)
            what = "srt_classify_probes on the %s grid, %s, K %d" % (grid.counts, flag_names(flags, (("RELOCATE", PS.RELOCATE), ("NORMALIZE", PS.NORMALIZE))), pf.K)
            want = pf.classified(c, which, way)
            pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
            kw = dict(directions=(c.scaled if normalize else c.dirs) if relocate else None, relocate=relocate, normalize=normalize, positions=True)
            pt.classify_probes(count_work=True, **kw)
            rec, pos, work = pt.probe_states_output("records"), pt.probe_states_output("positions"), pt.probe_states_work()
            print("%s, %s: work %s, winning steps %s" % (pf.where(c), what, work, np.bincount(want["step"]).tolist()))
            check(c, what + ", RECORDS", rec, want["records"])
            check(c, what + ", POSITIONS", pos, want["positions"])
            assert work["valid"] == 1 and work["waves"] > 0 and {k: work[k] for k in want["work"]} == want["work"], (pf.where(c), what, work, want["work"])
            pt.classify_probes(**kw)
            check(c, what + ", a second call, RECORDS", pt.probe_states_output("records"), rec)
            check(c, what + ", a second call, POSITIONS", pt.probe_states_output("positions"), pos)
    finally:
        pt.close()


# ---- the four shading calls ------------------------------------------------------------------------------------------------------------
def _grid_kwargs(flags):
    return dict(normal_weight=bool(flags & PG.NORMAL_WEIGHT), albedo=bool(flags & PG.ALBEDO))


def _shade_one_grid(oracle, c, pt, which):
    grid = getattr(c, which)
    co, mo, rec = (c.co, c.mo, c.rec) if which == "grid" else (c.flat_co, c.flat_mo, c.flat_rec)
    on = "on the %s grid" % (grid.counts,)
    pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
    occ = pf.grid_segments(oracle, c, which)[4]
    first = True
    for flags in GRID_FLAGS:  # srt_shade_probe_grid; for VISIBILITY the oracle answers the segments
        what = "srt_shade_probe_grid %s, flags %s" % (on, flag_names(flags, GRID_NAMES))
        want = PG.shade(grid, co, c.obj, c.nd, c.pos, albedo=c.alb, flags=flags, occluded=occ)
        counts = PG.work_formula(grid, c.obj, c.nd, c.pos, flags, occ)
        kw = dict(visibility=bool(flags & PG.VISIBILITY), **_grid_kwargs(flags))
        pt.shade_probe_grid(coefficients=co if first else None, count_work=True, **kw)
        first = False
        got, work = pt.probe_grid_output(), pt.probe_grid_work()
        check(c, what, got, want)
        assert work["valid"] == 1 and tuple(work[k] for k in GRID_WORK) == counts, (pf.where(c), what, work, counts)
        pt.shade_probe_grid(**kw)
        check(c, what + ", a second call", pt.probe_grid_output(), got)
    print("%s, %s: %d segments, %d open" % (pf.where(c), on, len(occ), int((occ == 0).sum())))
    first = True
    for flags in DEPTH_FLAGS:  # srt_shade_probe_grid_depth
        what = "srt_shade_probe_grid_depth %s, R %d, flags %s" % (on, R, flag_names(flags, GRID_NAMES))
        want, counts = PD.shade(grid, co, mo, R, c.obj, c.nd, c.pos, albedo=c.alb, flags=flags)
        pt.shade_probe_grid_depth(moments=mo if first else None, resolution=R, count_work=True, **_grid_kwargs(flags))
        first = False
        got, work = pt.probe_grid_output(), pt.probe_grid_work()
        check(c, what, got, want)
        assert {k: work[k] for k in GRID_WORK} == {k: counts[k] for k in GRID_WORK}, (pf.where(c), what, work, counts)
        pt.shade_probe_grid_depth(**_grid_kwargs(flags))
        check(c, what + ", a second call", pt.probe_grid_output(), got)
    first = True
    for depth in (None, mo):  # srt_shade_probe_grid_states
        for flags in DEPTH_FLAGS:
            what = "srt_shade_probe_grid_states %s, %s, flags %s" % (on, "R %d" % R if depth is not None else "no depth", flag_names(flags, GRID_NAMES))
            want, counts = PS.shade(grid, co, rec, c.obj, c.nd, c.pos, albedo=c.alb, flags=flags, depth=depth, R=R if depth is not None else None)
            pt.shade_probe_grid_states(states=rec if first else None, depth=depth is not None, count_work=True, **_grid_kwargs(flags))
            first = False
            got, work = pt.probe_grid_output(), pt.probe_grid_work()
            check(c, what, got, want)
            assert {k: work[k] for k in GRID_WORK} == {k: counts[k] for k in GRID_WORK}, (pf.where(c), what, work, counts)
            pt.shade_probe_grid_states(depth=depth is not None, **_grid_kwargs(flags))
            check(c, what + ", a second call", pt.probe_grid_output(), got)


def _device_chain(c, pt):
    """Classify, trace coefficients and moments at the classified positions, shade by the records: device to device, nothing
    crosses the bus between the calls.  The shading must equal the reference applied to what the buffers hold."""
    import torch

    grid, P = c.grid, c.grid.probes
    dev = "cuda:%d" % pt.device
    t = {k: torch.zeros((n, 4), dtype=torch.float32, device=dev) for k, n in (("records", P), ("positions", P), ("coefficients", 9 * P), ("moments", R * R * P))}
    torch.cuda.synchronize()
    what = "the device-to-device chain on the %s grid" % (grid.counts,)
    try:
        pt.set_probe_grid(grid.origin, grid.spacing, grid.counts)
        pt.bind_probe_states_output("records", t["records"])
        pt.bind_probe_states_output("positions", t["positions"])
        pt.bind_light_probe_output("coefficients", t["coefficients"])
        pt.bind_probe_depth_output("moments", t["moments"])
        for _ in range(2):
            pt.classify_probes(directions=c.dirs, relocate=True, positions=True)
            pt.trace_light_probes(t["positions"], c.dirs, samples=2, bounces=2, seed=c.seeds["chain"])
            pt.trace_probe_depth(resolution=R, sharpness=SHARPNESS, max_distance=c.max_distance)
            pt.shade_probe_grid_states(coefficients=t["coefficients"], states=t["records"], moments=t["moments"], resolution=R, normal_weight=True, albedo=True,
                                       count_work=True)
            got, work = pt.probe_grid_output(), pt.probe_grid_work()
            rec, pos = t["records"].cpu().numpy(), t["positions"].cpu().numpy()
            co, mo = t["coefficients"].cpu().numpy().reshape(P, 9, 4), t["moments"].cpu().numpy().reshape(P, R * R, 4)
            ref = pf.classified(c, "grid", "relocate")
            check(c, what + ", RECORDS", rec, ref["records"])
            check(c, what + ", POSITIONS", pos, ref["positions"])
            want, counts = PS.shade(grid, co, rec, c.obj, c.nd, c.pos, albedo=c.alb, flags=PG.NORMAL_WEIGHT | PG.ALBEDO, depth=mo, R=R)
            check(c, what + ", srt_shade_probe_grid_states against the reference on the read-backs", got, want)
            assert {k: work[k] for k in GRID_WORK} == {k: counts[k] for k in GRID_WORK}, (pf.where(c), what, work, counts)
    finally:
        pt.wait()


@pytest.mark.parametrize("key", SHADING_KEYS)
def test_probe_grid_shading(srt, oracle, key):
    c = pf.case(oracle, key)
    pt = _tracer(srt, c)
    try:
        check_guides(c, pt)
        for which in ("grid", "flat"):
            _shade_one_grid(oracle, c, pt, which)
        # srt_shade_probe_cascade: two levels around the centroid of the hit points
        cas = c.cascade
        load_cascade(pt, cas, c.cas_co, c.cas_rec, c.cas_mo)
        for flags in CASCADE_FLAGS:
            what = "srt_shade_probe_cascade, two levels, blend_cells 1, flags %s" % flag_names(flags, CASCADE_NAMES)
            want, wwork, info = PC.shade(cas, c.cas_co, c.obj, c.nd, c.pos, records=c.cas_rec if flags & PC.STATES else None,
                                         moments=c.cas_mo if flags & PC.DEPTH else None, albedo=c.alb, flags=flags)
            pt.shade_probe_cascade(count_work=True, **cascade_kwargs(flags))
            got, work = pt.probe_grid_output(), pt.probe_cascade_work()
            check(c, what, got, want)
            assert work["valid"] == 1 and {k: work[k] for k in CASCADE_COUNTS} == {k: wwork[k] for k in CASCADE_COUNTS}, (pf.where(c), what, work, wwork)
            pt.shade_probe_cascade(**cascade_kwargs(flags))
            check(c, what + ", a second call", pt.probe_grid_output(), got)
        print("%s: cascade classes %s" % (pf.where(c), dict(zip(*np.unique(info["cls"], return_counts=True)))))
        _device_chain(c, pt)
    finally:
        pt.close()


# ---- the probe tail --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SHADING_KEYS)
def test_probe_tail(srt, oracle, key):
    c = pf.case(oracle, key)
    pt = _tracer(srt, c)
    seed = c.seeds["tail"]
    try:
        set_grid(pt, c.grid, c.co, c.mo, c.rec)
        for bounces in (1, 3):
            colours, terminals = pf.paths(oracle, c, bounces, 2, seed)
            kw = dict(samples=2, bounces=bounces, seed=seed)
            # with the mode off: srt_render's bits, which are the reference loop's without an addend
            what = "srt_trace_radiance on the camera rays, 2 samples, %d bounces, seed %d" % (bounces, seed)
            tail(pt, 0, on=False)
            pt.trace_radiance(c.O4, c.D4, **kw)
            off = pt.radiance()
            pt.render(spp=2, **{k: v for k, v in kw.items() if k != "samples"})
            check(c, what + ", the mode off, against srt_render", off, pt.accumulator().reshape(W * H, 4))
            check(c, what + ", the mode off, against the reference loop", off, PT.radiance(colours))
            for label, flags in TAIL_FLAGS.items():
                mode = what + " under srt_probe_tail, flags %s" % label
                add, adds, work = PT.tails(terminals, c.grid, c.co, flags=flags, depth=c.mo, R=R, records=c.rec)
                want = PT.radiance(colours, add=(add, adds))
                tail(pt, flags)
                pt.trace_radiance(count_work=True, **kw)
                got, tw = pt.radiance(), pt.probe_tail_work()
                print("%s, %d bounces, %s: reference %s" % (pf.where(c), bounces, label, work))
                check(c, mode, got, want)
                assert tw["valid"] == 1 and {k: tw[k] for k in TAIL_COUNTS} == work, (pf.where(c), mode, tw, work)
                pt.trace_radiance(**kw)
                check(c, mode + ", a second call", pt.radiance(), got)
    finally:
        tail(pt, 0, on=False)
        pt.close()


# ---- adaptive rendering ----------------------------------------------------------------------------------------------------------------
ADAPTIVE_BOUNCES, ADAPTIVE_TAIL_BOUNCES, ADAPTIVE_TAIL_FLAGS = 3, 1, PT.DEPTH | PT.STATES | PT.NORMAL_WEIGHT


def _check_frame(c, what, got, want):
    (gfb, gacc), (wfb, wacc) = got, want
    check(c, what + ", accumulator", gacc, wacc)
    check(c, what + ", framebuffer (memory rows)", gfb, wfb, lanes=0)


@pytest.mark.parametrize("key", KEYS)
def test_adaptive_rendering(srt, oracle, key):
    c = pf.case(oracle, key)
    pt = _tracer(srt, c)
    seed, b = c.seeds["adaptive"], c.budget
    try:
        bound = Bound(pt, W, H)
        s = types.SimpleNamespace(oracle=oracle, oarr=c.oarr, n=c.n, env=c.env, w=W, h=H, om=c.om)

        def run(call, **kw):
            pt.write_sample_counts(np.zeros((H, W), np.uint32))
            pt.write_sample_budget(b)
            bound.sentinel()
            call(seed=seed, **kw)
            got = bound.read()
            assert np.array_equal(pt.sample_counts(), b), (pf.where(c), call.__name__)
            return got

        # srt_render_adaptive: per pixel the oracle after its own number of samples
        what = "srt_render_adaptive, counts from %s, %d bounces, seed %d" % (pf.BUDGETS.tolist(), ADAPTIVE_BOUNCES, seed)
        want = Ref(s, c.cam, ADAPTIVE_BOUNCES, seed).at(b, *sentinels(W, H))
        got = run(pt.render_adaptive, bounces=ADAPTIVE_BOUNCES, count_work=True)
        work = pt.adaptive_work()
        _check_frame(c, what, got, want)
        assert (got[1].view(np.uint32)[b == 0] == SENT_ACC).all()  # (the sentinels are still there)
        assert work["valid"] == 1 and work["pixels"] == int((b > 0).sum()) and work["samples"] == int(b.sum()), (pf.where(c), what, work)
        _check_frame(c, what + ", a second call", run(pt.render_adaptive, bounces=ADAPTIVE_BOUNCES), got)

        # srt_render_adaptive_tail: the same composition with the tail reference
        what = "srt_render_adaptive_tail, flags DEPTH|STATES|NORMAL_WEIGHT, %d bounce, seed %d" % (ADAPTIVE_TAIL_BOUNCES, seed)
        n_max = int(b.max())
        colours, terminals = pf.paths(oracle, c, ADAPTIVE_TAIL_BOUNCES, n_max, seed)
        add, adds, _ = PT.tails(terminals, c.grid, c.co, flags=ADAPTIVE_TAIL_FLAGS, depth=c.mo, R=R, records=c.rec)
        wfb, wacc = sentinels(W, H)
        for n in np.unique(b):
            if n == 0:
                continue
            rows = (np.arange(W * H)[:, None] * n_max + np.arange(n)[None, :]).reshape(-1)  # the first n samples of every ray
            rad = PT.radiance(colours[:, :n], add=(add[rows], adds[rows])).reshape(H, W, 4)
            m = b == n  # scene rows; the framebuffer's memory row is H - 1 - y
            wacc[m] = rad[m]
            wfb[m[::-1]] = tone_map(rad)[::-1][m[::-1]]
        set_grid(pt, c.grid, c.co, c.mo, c.rec)
        tail(pt, ADAPTIVE_TAIL_FLAGS)
        got = run(pt.render_adaptive_tail, bounces=ADAPTIVE_TAIL_BOUNCES)
        _check_frame(c, what, got, (wfb, wacc))
        _check_frame(c, what + ", a second call", run(pt.render_adaptive_tail, bounces=ADAPTIVE_TAIL_BOUNCES), got)
    finally:
        tail(pt, 0, on=False)
        pt.bind_output()
        pt.close()
