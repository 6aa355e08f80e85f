"""First-hit buffers (srt_render_gbuffer, ABI 7) on the MI355X: object index, normal + distance, point and albedo of every
pixel's camera ray, bit for bit against the oracle's GetClosestObject (Raytracer.cpp:123-140), against srt_render's own
primary hits and against the brute-force triangle definition; bands, output masks, binding, streams and the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENE_NAMES, scene_path

pytestmark = pytest.mark.gpu

NAMES = ["object", "normal_depth", "position", "albedo"]
CLI = os.path.join(ROOT, "software-raytracer_amd", "srt_render")


def _tracer(srt, oracle, objs, w, h, meshes=None, cam=None):
    oarr, n = oracle.make_objects(objs)
    pt = srt.PathTracer(w, h)
    keep = None
    if meshes:
        marr, mn, keep = oracle.make_meshes(meshes)
        pt.set_meshes(C.cast(marr, C.POINTER(srt.Mesh)), mn)
    pt.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
    pt.set_camera(cam if cam is not None else srt.default_camera())
    return pt, oarr, n, keep


def _gbuffers(pt):
    return {k: pt.gbuffer(k) for k in NAMES}


def _oracle_hits(oracle, oarr, n, cam, w, h, xs, ys, meshes=None):
    """srt_oracle_closest for the camera rays of pixels (xs[i], ys[i]) (scene rows): index, normal, point, distance.  With
    meshes = (oracle mesh array, count): srt_oracle_closest_m, which also hits SRT_OBJ_MESH objects."""
    L = oracle.lib()
    d, nn, pp, t = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)(), C.c_float()
    origin = (C.c_float * 3)(*cam.position)
    k = len(xs)
    idx = np.empty(k, np.int32)
    nrm, pnt, dist = np.zeros((k, 3), np.float32), np.zeros((k, 3), np.float32), np.zeros(k, np.float32)
    for i, (x, y) in enumerate(zip(xs, ys)):
        L.srt_oracle_ray_direction(C.byref(cam), w, h, int(x), int(y), d)
        if meshes:
            idx[i] = L.srt_oracle_closest_m(oarr, n, meshes[0], meshes[1], origin, d, nn, pp, C.byref(t))
        else:
            idx[i] = L.srt_oracle_closest(oarr, n, origin, d, nn, pp, C.byref(t))
        if idx[i] >= 0:
            nrm[i], pnt[i], dist[i] = nn[:], pp[:], t.value
    return idx, nrm, pnt, dist


def _same_bits(a, b):
    """Bit equality, NaNs compared as NaNs (their sign and payload are the processor's)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a) | np.isnan(b)
    return bool(np.all(np.where(nan, np.isnan(a) & np.isnan(b), a.view(np.uint32) == b.view(np.uint32))))


def _check_against_oracle(g, oracle, oarr, n, cam, w, h, xs, ys, meshes=None):
    idx, nrm, pnt, dist = _oracle_hits(oracle, oarr, n, cam, w, h, xs, ys, meshes)
    obj, nd, pos, alb = g["object"][ys, xs], g["normal_depth"][ys, xs], g["position"][ys, xs], g["albedo"][ys, xs]
    assert np.array_equal(obj, idx), "object index differs at %d pixels" % int((obj != idx).sum())
    hit, miss = idx >= 0, idx < 0
    assert _same_bits(nd[hit, :3], nrm[hit]) and _same_bits(nd[hit, 3], dist[hit]), "normal / distance bits differ"
    assert _same_bits(pos[hit, :3], pnt[hit]) and np.all(pos[hit, 3] == 1.0), "point bits differ"
    base = np.array([list(oarr[int(i)].material.base_color) for i in idx[hit]], np.float32).reshape(-1, 3)
    base = np.where(base < 0, np.float32(0), base)  # Color's clamping constructor (Common.hpp:253-262)
    assert _same_bits(alb[hit, :3], base) and np.all(alb[hit, 3].view(np.uint32) == 0), "albedo bits differ"
    miss_nd = np.array([0, 0, 0, np.inf], np.float32).view(np.uint32)
    assert np.all(nd[miss].view(np.uint32) == miss_nd)
    assert np.all(pos[miss].view(np.uint32) == 0) and np.all(alb[miss].view(np.uint32) == 0)
    return int(hit.sum()), int(miss.sum())


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_every_pixel_matches_the_oracle(srt, oracle, name):
    w, h = 256, 144
    pt, oarr, n, _ = _tracer(srt, oracle, oracle.load_scene_json_py(scene_path(name)), w, h)
    pt.render_gbuffer()
    g = _gbuffers(pt)
    ys, xs = np.mgrid[0:h, 0:w]
    hits, misses = _check_against_oracle(g, oracle, oarr, n, oracle.default_camera(), w, h, xs.ravel(), ys.ravel())
    assert hits > 0
    pt.close()


def test_scene1_1080p_on_a_stride_matches_the_oracle(srt, oracle):
    w, h = 1920, 1080
    pt, oarr, n, _ = _tracer(srt, oracle, oracle.load_scene_json_py(scene_path("Scene1")), w, h)
    pt.render_gbuffer()
    g = _gbuffers(pt)
    sel = np.arange(0, w * h, 97)  # 21,378 pixels, every column residue and row of the frame touched
    sel = np.concatenate([sel, [w - 1, w * h - 1, w * (h - 1)]])
    hits, misses = _check_against_oracle(g, oracle, oarr, n, oracle.default_camera(), w, h, sel % w, sel // w)
    assert len(sel) >= 20000 and hits > 1000 and misses > 100
    pt.close()


def test_scene_in_hbm_and_sphere_outside_the_short_sqrt_window(srt, oracle):
    # about 3400 spheres + boxes: the scene image cannot be staged into LDS (the HBM instantiation)
    rng = np.random.default_rng(77)
    objs = []
    for _ in range(3400):
        objs.append(dict(type=oracle.OBJ_SPHERE, position=tuple(float(v) for v in (rng.uniform(-6, 6), rng.uniform(-3, 3), rng.uniform(4, 16))),
                         radius=float(rng.uniform(0.03, 0.25)), base=tuple(float(v) for v in rng.uniform(0, 1, 3))))
    for _ in range(60):
        objs.append(dict(type=oracle.OBJ_BOX, position=tuple(float(v) for v in (rng.uniform(-6, 6), rng.uniform(-3, 3), rng.uniform(4, 16))),
                         half_size=tuple(float(v) for v in rng.uniform(0.05, 0.5, 3)), base=tuple(float(v) for v in rng.uniform(0, 1, 3))))
    objs.append(dict(type=oracle.OBJ_SPHERE, position=(0.0, -1003.5, 8.0), radius=1000.0, base=(0.6, 0.6, 0.6)))
    w, h = 96, 64
    pt, oarr, n, _ = _tracer(srt, oracle, objs, w, h)
    pt.render_gbuffer()
    ys, xs = np.mgrid[0:h, 0:w]
    hits, _ = _check_against_oracle(_gbuffers(pt), oracle, oarr, n, oracle.default_camera(), w, h, xs.ravel(), ys.ravel())
    assert hits > w * h // 2
    pt.close()
    # a sphere of infinite radius (outside the short square root's window: the library-sqrt instantiation); its hits lie at -inf
    objs = oracle.load_scene_json_py(scene_path("Scene1"))
    objs.insert(3, dict(type=oracle.OBJ_SPHERE, position=(0.0, 0.0, 2e19), radius=float("inf"), base=(.9, .2, .1)))
    w, h = 129, 65
    pt, oarr, n, _ = _tracer(srt, oracle, objs, w, h)
    pt.render_gbuffer()
    ys, xs = np.mgrid[0:h, 0:w]
    _check_against_oracle(_gbuffers(pt), oracle, oarr, n, oracle.default_camera(), w, h, xs.ravel(), ys.ravel())
    pt.close()


def test_nan_camera_direction_misses_everywhere(srt, oracle):
    w, h = 64, 40
    cam = srt.default_camera()
    cam.forward = (C.c_float * 3)(float("nan"), 0.0, 1.0)
    pt, oarr, n, _ = _tracer(srt, oracle, oracle.load_scene_json_py(scene_path("Scene1")), w, h, cam=cam)
    pt.render_gbuffer()
    assert np.all(pt.gbuffer("object") == -1)
    assert np.all(pt.gbuffer("normal_depth").view(np.uint32) == np.array([0, 0, 0, np.inf], np.float32).view(np.uint32))
    pt.close()


def _scene1_with_mesh(oracle, stacks=12, slices=16):
    objs = oracle.load_scene_json_py(scene_path("Scene1"))
    big = objs[64]  # the r = 1 ball at (0, 0, 5), as in test_gpu_mesh.py
    objs[64] = dict(type=oracle.OBJ_MESH, position=big["position"], mesh=0, base=big["base"], emissive=big["emissive"],
                    smoothness=big["smoothness"], specular_amount=big["specular_amount"], specular=big["specular"])
    return objs, [oracle.uv_sphere(1.0, stacks, slices)]


@pytest.mark.parametrize("case", ["Scene1", "Scene3", "Scene1 with mesh"])
def test_index_agrees_with_the_path_tracers_primary_hits(srt, oracle, case):
    meshes = None
    if case == "Scene1 with mesh":
        objs, meshes = _scene1_with_mesh(oracle)
    else:
        objs = oracle.load_scene_json_py(scene_path(case))
    for i, o in enumerate(objs):  # every object shines a unique tag: red = list index + 1, green = 1000
        o["emissive"] = (float(i + 1), 1000.0, 0.0)
    w, h = 200, 112
    pt, oarr, n, keep = _tracer(srt, oracle, objs, w, h, meshes=meshes)
    pt.render(spp=1, bounces=0, seed=0, reset=True)
    pt.render_gbuffer(outputs="object")
    acc, idx = pt.accumulator(), pt.gbuffer("object")
    tagged = acc[..., 1] == 1000.0
    assert tagged.sum() > 0 and np.all(idx[tagged] == acc[..., 0][tagged].astype(np.int32) - 1)
    assert not np.any(tagged & (idx < 0))
    assert tagged.sum() == (idx >= 0).sum()
    for y in range(3, h, 13):
        for x in range(5, w, 23):
            assert pt.pick(x, y) == idx[y, x], (x, y)
    pt.close()


def test_mesh_hits_match_the_brute_force_triangle_definition(srt, oracle):
    objs, meshes = _scene1_with_mesh(oracle)
    w, h = 160, 90
    pt, oarr, n, keep = _tracer(srt, oracle, objs, w, h, meshes=meshes)
    pt.render_gbuffer()
    g = _gbuffers(pt)
    ys, xs = np.nonzero(g["object"] == 64)
    assert len(xs) >= 256
    pick = np.linspace(0, len(xs) - 1, 300).astype(int)
    V, T = meshes[0]
    world = (V + np.array(objs[64]["position"], np.float32)).astype(np.float32)  # vertex + position, binary32
    L = oracle.lib()
    L.srt_oracle_triangle.argtypes = [C.POINTER(C.c_float)] * 5 + [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.srt_oracle_triangle.restype = C.c_int
    cam = oracle.default_camera()
    tv = [[(C.c_float * 3)(*world[int(k)]) for k in tri] for tri in T]
    d, nn, pp, t, origin = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)(), C.c_float(), (C.c_float * 3)(*cam.position)
    for i in pick:
        x, y = int(xs[i]), int(ys[i])
        L.srt_oracle_ray_direction(C.byref(cam), w, h, x, y, d)
        best = None
        for v0, v1, v2 in tv:  # in triangle order, strictly closer wins: the lower index keeps a tie
            if L.srt_oracle_triangle(v0, v1, v2, origin, d, nn, pp, C.byref(t)) and (best is None or t.value < best[0]):
                best = (t.value, list(nn), list(pp))
        assert best is not None, (x, y)
        nd, pos = g["normal_depth"][y, x], g["position"][y, x]
        assert _same_bits(nd[3], best[0]) and _same_bits(nd[:3], best[1]) and _same_bits(pos[:3], best[2]), (x, y)
    pt.close()


def test_bands_and_output_masks_with_bound_buffers(srt, oracle):
    import torch

    w, h = 120, 70
    pt, oarr, n, _ = _tracer(srt, oracle, oracle.load_scene_json_py(scene_path("Scene3")), w, h)
    pt.render_gbuffer()
    full = _gbuffers(pt)
    bufs = {"object": torch.full((h, w), -7, dtype=torch.int32, device="cuda:0")}
    for k in NAMES[1:]:
        bufs[k] = torch.full((h, w, 4), 12345.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    for k in NAMES:
        pt.bind_gbuffer(k, bufs[k])
    rb, re = 13, 41  # memory rows -> scene rows [h - 41, h - 13)
    pt.render_gbuffer(rows=(rb, re), outputs=["object", "position"])
    pt.wait()
    got = {k: bufs[k].cpu().numpy() for k in NAMES}
    inside = np.zeros(h, bool)
    inside[h - re:h - rb] = True
    for k in ("object", "position"):
        assert np.array_equal(got[k][inside].view(np.uint32), full[k][inside].view(np.uint32)), k
        sentinel = -7 if k == "object" else 12345.0
        assert np.all(got[k][~inside] == sentinel), k
        assert np.array_equal(pt.gbuffer(k), got[k])  # srt_read_gbuffer reads the bound buffer
    assert np.all(got["normal_depth"] == 12345.0) and np.all(got["albedo"] == 12345.0)
    # errors: bad masks, flags, bands; state
    for kw in (dict(outputs=0), dict(outputs=16), dict(outputs=17), dict(flags=1), dict(rows=(-1, 5)), dict(rows=(5, 5)), dict(rows=(0, h + 1)),
               dict(rows=(9, 3))):
        with pytest.raises(srt.SrtError) as e:
            pt.render_gbuffer(**kw)
        assert e.value.code == srt.capi.ERR_INVALID_ARG, kw
    for bit in (0, 3, 16):
        assert pt.L.srt_bind_gbuffer(pt._h, bit, None) == srt.capi.ERR_INVALID_ARG
    pt.close()
    fresh = srt.PathTracer(w, h)
    with pytest.raises(srt.SrtError) as e:
        fresh.render_gbuffer()
    assert e.value.code == srt.capi.ERR_STATE
    fresh.set_scene(C.cast(oarr, C.POINTER(srt.Object)), n)
    with pytest.raises(srt.SrtError) as e:
        fresh.render_gbuffer()
    assert e.value.code == srt.capi.ERR_STATE
    with pytest.raises(srt.SrtError) as e:
        fresh.gbuffer("albedo")  # neither bound nor rendered
    assert e.value.code == srt.capi.ERR_STATE
    fresh.close()


def test_gbuffer_between_renders_changes_nothing_of_the_render(srt, oracle):
    w, h = 320, 256  # 300 workgroups: cost-ordered dispatch and the launch-shape record take part
    objs = oracle.load_scene_json_py(scene_path("Scene1"))
    fields = ("rays", "sample_chunks", "tile_rows", "chunk_samples", "shape_source", "path_samples")
    runs = []
    for with_gbuffer in (False, True):
        pt, oarr, n, _ = _tracer(srt, oracle, objs, w, h)
        pt.render(spp=64, bounces=4, seed=5, count_rays=True, count_work=True)
        first = pt.stats()
        if with_gbuffer:
            pt.render_gbuffer()
            after = pt.stats()  # still the render's
            assert all(getattr(after, f) == getattr(first, f) for f in fields) and after.kernel_ms == first.kernel_ms
        pt.render(spp=64, first_sample=65, reset=False, bounces=4, seed=5, count_rays=True, count_work=True)
        st = pt.stats()
        runs.append(([getattr(first, f) for f in fields], [getattr(st, f) for f in fields], pt.work_counts().as_dict(),
                     pt.framebuffer(), pt.accumulator()))
        pt.close()
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4].view(np.uint32), b[4].view(np.uint32))


def test_torch_binding_stream_and_camera_capture(srt, oracle):
    import torch

    w, h = 96, 54
    pt, oarr, n, _ = _tracer(srt, oracle, oracle.load_scene_json_py(scene_path("Scene_indirect")), w, h)
    stream = torch.cuda.Stream(device=0)
    pt.set_stream(stream.cuda_stream)
    cam2 = srt.default_camera()
    cam2.position = (C.c_float * 3)(0.3, 0.4, -0.5)
    ocam2 = oracle.default_camera()
    ocam2.position = (C.c_float * 3)(0.3, 0.4, -0.5)
    sets = []
    for cam in (srt.default_camera(), cam2):  # both enqueued before anything is waited for: the camera is taken at enqueue
        t = {"object": torch.empty((h, w), dtype=torch.int32, device="cuda:0")}
        for k in NAMES[1:]:
            t[k] = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
        for k in NAMES:
            pt.bind_gbuffer(k, t[k])
        pt.set_camera(cam)
        pt.render_gbuffer()
        sets.append(t)
    stream.synchronize()
    ys, xs = np.mgrid[0:h, 0:w]
    for t, ocam in zip(sets, (oracle.default_camera(), ocam2)):
        g = {k: t[k].cpu().numpy() for k in NAMES}
        _check_against_oracle(g, oracle, oarr, n, ocam, w, h, xs.ravel(), ys.ravel())
    assert not np.array_equal(sets[0]["object"].cpu().numpy(), sets[1]["object"].cpu().numpy())
    for k in NAMES:  # the last binding is what srt_read_gbuffer reads
        assert np.array_equal(pt.gbuffer(k).view(np.uint32), sets[1][k].cpu().numpy().view(np.uint32))

    class Spy:  # counts native calls of srt_bind_gbuffer
        calls = 0

        def __init__(self, L):
            self._L = L

        def __getattr__(self, name):
            if name == "srt_bind_gbuffer":
                Spy.calls += 1
            return getattr(self._L, name)

    pt.L = Spy(pt.L)
    bad = [("object", torch.empty((h, w), dtype=torch.float32, device="cuda:0")),
           ("albedo", torch.empty((h, w, 3), dtype=torch.float32, device="cuda:0")),
           ("position", torch.empty((w, h, 4), dtype=torch.float32, device="cuda:0")),
           ("normal_depth", torch.empty((h, w, 4), dtype=torch.float32)),
           ("normal_depth", torch.empty((h, w, 4), dtype=torch.float64, device="cuda:0")),
           ("position", torch.empty((h, 2 * w, 4), dtype=torch.float32, device="cuda:0")[:, ::2])]
    for name, tensor in bad:
        with pytest.raises((TypeError, ValueError)):
            pt.bind_gbuffer(name, tensor)
    assert Spy.calls == 0
    pt.L = pt.L._L
    pt.set_stream(0)
    pt.close()


def test_cli_writes_npy_files_and_the_same_ppm(srt, tmp_path):
    w, h = 160, 90
    base = [CLI, "--scene", scene_path("Scene1"), "--width", str(w), "--height", str(h), "--spp", "2", "--bounces", "2"]
    r1 = subprocess.run(base + ["--out", str(tmp_path / "a.ppm")], capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr[-2000:]
    prefix = str(tmp_path / "g")
    r2 = subprocess.run(base + ["--out", str(tmp_path / "b.ppm"), "--gbuffer", prefix], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr[-2000:]
    assert (tmp_path / "a.ppm").read_bytes() == (tmp_path / "b.ppm").read_bytes()
    files = {k: np.load(prefix + "_" + k + ".npy") for k in NAMES}
    assert files["object"].shape == (h, w) and files["object"].dtype == np.int32
    for k in NAMES[1:]:
        assert files[k].shape == (h, w, 4) and files[k].dtype == np.float32
    # the host layer's renderer (same scene file, same camera) through the Python API, flipped to top-down rows
    scene = srt.host.Scene(scene_path("Scene1"))
    r = srt.host.Renderer(w, h)
    r.set_scene(scene)
    r.render_gbuffer()
    for k in NAMES:
        assert np.array_equal(files[k].view(np.uint32), np.flipud(r.gbuffer(k)).view(np.uint32)), k
    r.close()
    # --devices: the whole frame's buffers from the first device
    r3 = subprocess.run(base + ["--devices", "0,0", "--out", str(tmp_path / "c.ppm"), "--gbuffer", str(tmp_path / "m")],
                        capture_output=True, text=True, timeout=300)
    assert r3.returncode == 0, r3.stderr[-2000:]
    for k in NAMES:
        assert np.array_equal(np.load(str(tmp_path / "m") + "_" + k + ".npy").view(np.uint32), files[k].view(np.uint32)), k
