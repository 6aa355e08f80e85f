"""Randomized sweep of the ray-query entry points on the MI355X, on the scene families that back the culling-bound proofs of
srt_render (tests/test_gpu_fuzz.py): scenes 50 000 units from the origin, at 1e4 and 1e-2 scale, 30x, 300x and negative radii,
origins inside spheres, broken triangle soups and OBJ_NONE entries, and the 3400-sphere scene that is read from memory.
closest_hit's bounds and the separate set of any_hit (srt_occlusion.hip.h) depend on |o|_1 and on the size of t_max; the rays and
t_max sets of tests/query_fuzz_inputs.py push both, and tests/test_query_fuzz_inputs.py shows on the CPU that they are not vacuous.

Every comparison is bit for bit against the oracle's GetClosestObject per ray, with no tolerance and no ray left out (NaNs
compare as NaNs).  A failure names the seed, the kind, the t_max set and the first failing rays with their family and direction
tag: query_fuzz_inputs.build(oracle, seed) rebuilds the batch on the CPU, where the ray can be replayed through the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import query_fuzz_inputs as q
import visibility_reference as VR
from test_gpu_fuzz import _random_environment, _same_bits
from test_gpu_occlusion import _three_way
from test_gpu_radiance import camera_rays, srt_camera
from test_gpu_rays import NAMES, _check, _oracle, _trace, _unit

pytestmark = pytest.mark.gpu

KEYS = list(range(int(os.environ.get("SRT_FUZZ_QUERY_N", str(q.DEFAULT_SEEDS))))) + list(q.LARGE)
FRAME_KEYS = [0, 1, 2, 3, 4, "large"]  # one seed per kind, and the scene that is read from memory (analytic)
W, H = 26, 16  # 26 is no multiple of the 8 x 8 tile


def _tracer(srt, c, w=16, h=16):
    pt = srt.PathTracer(w, h)
    pt.set_meshes(C.cast(c.marr, C.POINTER(srt.Mesh)), c.mn)
    pt.set_scene(C.cast(c.oarr, C.POINTER(srt.Object)), c.n)
    return pt


def _bits(a, b):
    """Per-ray bit equality of two float arrays, NaNs compared as NaNs."""
    a, b = np.asarray(a, np.float32).reshape(len(a), -1), np.asarray(b, np.float32).reshape(len(b), -1)
    nan = np.isnan(a) | np.isnan(b)
    return np.where(nan, np.isnan(a) & np.isnan(b), a.view(np.uint32) == b.view(np.uint32)).all(axis=1)


def _wrong_rays(g, ref, D4):
    """For a failure message only (the assertion is test_gpu_rays._check's): the rays whose outputs differ from the oracle's."""
    idx, nrm, pnt, dist = ref
    hit = idx >= 0
    bad = g["object"] != idx
    bad |= hit & ~(_bits(g["normal_depth"][:, :3], nrm) & _bits(g["normal_depth"][:, 3], dist) & _bits(g["position"][:, :3], pnt))
    with np.errstate(invalid="ignore"):
        bad |= g["occluded"] != (hit & (dist < D4[:, 3]))
    return np.flatnonzero(bad)


def _same_outputs(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in NAMES)


def _closest_matches(c, pt, O4, D4, ref, what, rows=None, **kw):
    """srt_trace_rays, all five outputs, against the oracle through _check; returns the outputs."""
    g = _trace(pt, O4, D4, **kw)
    try:
        _check(g, ref, c.oarr, D4)
    except AssertionError as e:
        wrong = _wrong_rays(g, ref, D4)
        wrong = wrong if rows is None else rows[wrong]
        raise AssertionError("seed %s (%s), %s: %s; rays %s" % (c.key, c.kind, what, e, q.describe(c, wrong))) from e
    return g


def _occlusion_matches(c, pt, O4, D4, want, what, rows=None, **kw):
    """The oracle, srt_trace_rays(OCCLUDED) and srt_trace_occlusion agree on every ray (_three_way)."""
    try:
        return _three_way(pt, O4, D4, want, **kw)
    except AssertionError as e:
        pt.trace_rays(outputs="occluded", normalize=kw.get("normalize", False))
        closest = pt.ray_output("occluded")
        pt.trace_occlusion(**kw)
        wrong = np.flatnonzero((closest != want) | (pt.ray_output("occluded") != want))
        wrong = wrong if rows is None else rows[wrong]
        raise AssertionError("seed %s (%s), %s: %s; rays %s" % (c.key, c.kind, what, e, q.describe(c, wrong))) from e


@pytest.mark.parametrize("key", KEYS)
def test_random_scene_ray_queries(srt, oracle, key):
    c = q.case(oracle, key)
    pt = _tracer(srt, c)
    N = len(c.O4)
    D4 = c.D4.copy()
    # 1. the closest hit, all five outputs, OCCLUDED under the uniform t_max draw; 4. a second call gives the same bits
    D4[:, 3] = c.tmax["uniform"]
    g = _closest_matches(c, pt, c.O4, D4, c.ref, "closest hit, t_max set 'uniform'")
    pt.trace_rays()
    assert _same_outputs(g, {k: pt.ray_output(k) for k in NAMES}), "seed %s (%s): a second srt_trace_rays differs" % (c.key, c.kind)
    # 2. every t_max set, three ways
    for name, tmax in c.tmax.items():
        D4[:, 3] = tmax
        want = q.want(c, name)
        assert not want[c.ref[0] < 0].any()
        _occlusion_matches(c, pt, c.O4, D4, want, "t_max set %r" % name)
        if name in ("NaN", "-inf"):
            assert not want.any()
    # 3. the work record changes no bit and counts the batch; 4. and a second call
    D4[:, 3] = c.tmax["uniform"]
    want = q.want(c, "uniform")
    pt.write_rays(c.O4, D4)
    for count_work in (False, True, True, False):
        pt.trace_occlusion(count_work=count_work)
        got = pt.ray_output("occluded")
        assert np.array_equal(got, want), "seed %s (%s), count_work=%s: rays %s" % (c.key, c.kind, count_work, q.describe(c, np.flatnonzero(got != want)))
        if count_work:
            work = pt.occlusion_work()
            assert (work["valid"], work["rays"], work["occluded"]) == (1, N, int(want.sum())), (c.key, c.kind, work)
    # 3. the NORMALIZE flags on directions of length 0.5 and 3 give the bits of the pre-normalized batch, which are the oracle's
    rows = c.norm_rows
    assert len(rows) > 300 and np.array_equal(_unit(c.norm_D4[:, :3]).view(np.uint32), c.norm_pre[:, :3].view(np.uint32))
    gn = _closest_matches(c, pt, c.norm_O4, c.norm_D4, c.norm_ref, "SRT_RAYS_NORMALIZE on lengths 0.5 and 3", rows, normalize=True)
    gp = _closest_matches(c, pt, c.norm_O4, c.norm_pre, c.norm_ref, "the pre-normalized batch", rows)
    assert _same_outputs(gn, gp)
    with np.errstate(invalid="ignore"):
        want = ((c.norm_ref[0] >= 0) & (c.norm_ref[3] < c.norm_D4[:, 3])).astype(np.int32)
    _occlusion_matches(c, pt, c.norm_O4, c.norm_D4, want, "SRT_OCCLUSION_NORMALIZE on lengths 0.5 and 3", rows, normalize=True)
    pt.close()


def _camera(srt, oracle, c, rng):
    """A camera drawn as test_gpu_fuzz draws it: in front of the scene, turned about the up axis and then about its right axis."""
    cam = oracle.Camera()
    pos = c.off - np.array([0, 0, 6.0]) * c.scale + rng.uniform(-1, 1, 3) * c.scale
    basis = srt.host.rotate_about_axis([1, 0, 0, 0, 1, 0, 0, 0, 1], float(rng.uniform(-0.5, 0.5)), (0, 1, 0))
    basis = srt.host.rotate_about_axis(basis, float(rng.uniform(-0.3, 0.3)), basis[0:3])
    cam.position = oracle.f3(pos)
    cam.right, cam.up, cam.forward = oracle.f3(basis[0:3]), oracle.f3(basis[3:6]), oracle.f3(basis[6:9])
    cam.fov_degrees = int(rng.integers(15, 104))
    return cam


def _pinned_sun(srt, env, triangles):
    """The environment of the visibility call.  A sun_direction that is not unit length is pinned in analytic scenes only (rule 4
    of srt_render_visibility), so in a scene with triangles a finite non-zero one is replaced by its binary32 normalization."""
    env = srt.Environment.from_buffer_copy(bytes(env))
    s = np.array(env.sun_direction[:], np.float32)
    if triangles and np.isfinite(s).all() and s.any() and abs(float(q.dd64(s)) - 1.0) > 0.9e-6:
        env.sun_direction[:] = [float(v) for v in _unit(s)[0]]
    return env


@pytest.mark.parametrize("key", FRAME_KEYS)
def test_random_scene_frames_through_the_query_passes(srt, oracle, key):
    c = q.case(oracle, key)
    index = FRAME_KEYS.index(key)
    rng = np.random.default_rng(q.SEED_BASE + 500 + index)
    cam = _camera(srt, oracle, c, rng)
    env, env_kind = _random_environment(oracle, index, cam, W, H)
    where = "seed %s (%s), environment %s" % (c.key, c.kind, env_kind)
    pt = _tracer(srt, c, W, H)
    pt.set_environment(srt.Environment.from_buffer_copy(bytes(env)))
    pt.set_camera(srt_camera(srt, cam))
    O4, D4 = camera_rays(oracle, cam, W, H)
    assert np.all(np.abs(q.dd64(D4[:, :3]) - 1) < 0.9e-6), where  # (the camera's rays are inside the unit window)

    # the G-buffer against ray queries on the oracle's camera rays, and both against the oracle
    ref = _oracle(oracle, c.oarr, c.n, O4, D4, c.om)
    g = _trace(pt, O4, D4)
    try:
        _check(g, ref, c.oarr, D4)
    except AssertionError as e:
        raise AssertionError("%s: %s; pixels (x + y * %d) %s" % (where, e, W, _wrong_rays(g, ref, D4)[:10])) from e
    pt.render_gbuffer()
    guides = {k: pt.gbuffer(k) for k in NAMES[:4]}
    for k in NAMES[:4]:
        differ = np.flatnonzero((g[k].view(np.uint32).reshape(W * H, -1) != guides[k].view(np.uint32).reshape(W * H, -1)).any(axis=1))
        assert not len(differ), "%s: G-buffer %s differs from srt_trace_rays at pixels %s" % (where, k, differ[:10])
    hits = int((ref[0] >= 0).sum())
    print("%s: %d of %d pixels hit" % (where, hits, W * H))

    # radiance against srt_render and the oracle
    seed = int(rng.integers(0, 2**31))
    for bounces in (0, 3):
        _, acc, _ = oracle.render(c.oarr, c.n, env, cam, W, H, spp=5, bounces=bounces, seed=seed, meshes=(c.marr, c.mn) if c.mn else None, threads=16)
        pt.trace_radiance(O4, D4, samples=5, bounces=bounces, seed=seed)
        got = pt.radiance()
        same = _same_bits(got, acc.reshape(W * H, 4))
        assert same.all(), "%s, bounces %d: srt_trace_radiance differs from the oracle at pixels %s" % (where, bounces, np.flatnonzero(~same)[:10])
        pt.render(spp=5, bounces=bounces, seed=seed)
        same = _same_bits(got, pt.accumulator().reshape(W * H, 4))
        assert same.all(), "%s, bounces %d: srt_trace_radiance differs from srt_render at pixels %s" % (where, bounces, np.flatnonzero(~same)[:10])

    # visibility against its composition: segments built in numpy binary32 from the guides, answered by the oracle
    venv = _pinned_sun(srt, env, c.triangles)
    pt.set_environment(venv)
    sun = [float(v) for v in venv.sun_direction]
    by_oracle = lambda _, SO4, SD4: VR.occluded_by_oracle(oracle, c.oarr, c.n, SO4, SD4, c.om)
    for radius in (2.5 * c.scale, float("inf")):
        first_sample, vseed = int(rng.integers(1, 50)), int(rng.integers(0, 2**31))
        ao_ref, sun_ref, ao_open, sun_open = VR.reference(pt, guides["object"], guides["normal_depth"], guides["position"], sun, 5, first_sample, vseed,
                                                          radius, trace=by_oracle)
        pt.render_visibility(5, radius, first_sample=first_sample, seed=vseed)
        ao, sn = pt.visibility("ao"), pt.visibility("sun")
        print("   radius %s: %d of %d AO segments open, %d sun segments open" % (radius, ao_open, 5 * hits, sun_open))
        for name, got, want in (("AO", ao, ao_ref), ("SUN", sn, sun_ref)):
            differ = np.flatnonzero(got.view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))
            assert got.dtype == want.dtype and got.shape == want.shape and not len(differ), \
                "%s, radius %s, first_sample %d, seed %d: %s differs from the oracle's composition at pixels %s" % (where, radius, first_sample, vseed, name, differ[:10])
    pt.close()
