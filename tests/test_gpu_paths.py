"""Every pathtrace_kernel instantiation srt_render ships, and every launch path that reads or writes the accumulator, against the
oracle bit for bit (NaNs compared as NaNs): accumulator, framebuffer and ray count.

srt_render picks one of nine instantiations for analytic scenes and nine for mesh scenes (srt_capi.hip, launch_pathtrace): scene
image in LDS or in HBM (too big, or a sphere's r*r outside the short square root's window), full tiles / small tiles (the multi-sample
hand-out) / sample chunks, with or without the loop counts (TALLY); and, for analytic scenes in LDS, one of three ROWS instantiations
(launch_pathtrace_rows) in place of k_lds / t_lds where srt::fold_from_rows sends the sample colours through rows of the sample
buffer: from two samples on in one chunk of full tiles, at six waves per SIMD where srt::rows_six_waves lets it.  A cell of the
matrix below is named after the instantiation it is meant to reach (the name its launcher gives it in a comment) and asserts that
it did: from the launch's stats and work counts and, as the library does not report rows / six waves (no ABI change), from the
rule's own answer for the launch's request (tests/native/rows_rule_check.cpp --ask, tests/rows_rule.py).  The analytic ring kernels
k_lds / t_lds are what one-sample launches (`loop`) and the preview shader keep.  Every cell runs from a reset and then resumed on
a caller's accumulator that holds what the kernel's clamp elimination must not be fooled by (negatives, -0, 1e-38, a non-zero alpha),
on a ragged band."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import rows_rule
from conftest import ROOT, scene_path
from test_gpu_six_waves import _extra_sphere, threshold_counts

ORACLE_THREADS = 16
NAMES = ["k_lds", "k_lds_multi", "k_lds_defer", "k_hbm", "k_hbm_multi", "k_hbm_defer", "t_lds", "t_lds_multi", "t_lds_defer",
         "k_lds_rows", "k_lds_rows6", "t_lds_rows"]
NASTY = [(-1.0, 0.5, 2.0), (-0.0, 0.0, 1.0), (1e6, 1e-30, -1e6), (3.0, 0.25, -0.0), (1e-38, 1.0, -3.0), (0.0, -0.0, 7.5)]


def _same_bits(a, b):
    """Bit equality, NaNs compared as NaNs (their sign and payload are the processor's)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a) | np.isnan(b)
    return bool(np.all(np.where(nan, np.isnan(a) & np.isnan(b), a.view(np.uint32) == b.view(np.uint32))))


def _big_scene(oracle):
    """test_scene_larger_than_lds's 3400 spheres and 60 boxes: an image too big for LDS"""
    rng = np.random.default_rng(77)
    objs = []
    for _ in range(3400):
        objs.append(dict(type=oracle.OBJ_SPHERE, position=tuple(float(v) for v in (rng.uniform(-6, 6), rng.uniform(-3, 3), rng.uniform(4, 16))),
                         radius=float(rng.uniform(0.03, 0.25)) * (8.0 if rng.uniform() < 0.01 else 1.0),
                         base=tuple(float(v) for v in rng.uniform(0, 1, 3)), emissive=tuple(float(v) for v in rng.uniform(0, 3, 3) * (rng.uniform() < 0.05)),
                         specular_amount=float(rng.uniform(0, 1)), smoothness=float(rng.uniform(0, 1))))
    for _ in range(60):
        objs.append(dict(type=oracle.OBJ_BOX, position=tuple(float(v) for v in (rng.uniform(-6, 6), rng.uniform(-3, 3), rng.uniform(4, 16))),
                         half_size=tuple(float(v) for v in rng.uniform(0.05, 0.5, 3)), base=tuple(float(v) for v in rng.uniform(0, 1, 3)),
                         specular_amount=float(rng.uniform(0, 1)), smoothness=float(rng.uniform(0, 1))))
    objs.append(dict(type=oracle.OBJ_SPHERE, position=(0.0, -1003.5, 8.0), radius=1000.0, base=(0.6, 0.6, 0.6)))
    return objs


def _odd_spheres(oracle, objs, r):
    """spheres of radius r on the centre pixel's ray and next to it (test_spheres_outside_the_short_square_roots_window)"""
    objs.insert(3, dict(type=oracle.OBJ_SPHERE, position=(0.0, 0.0, 2.0) if r < 1e18 else (0.0, 0.0, 2e19), radius=r, base=(.9, .2, .1),
                        emissive=(0.5, 0.5, 0.5)))
    objs.append(dict(type=oracle.OBJ_SPHERE, position=(0.3, 0.1, 3.0), radius=r, base=(.1, .9, .1)))


def _scene(oracle, kind, n_over=0):
    """kind -> dict(objs, meshes, env, cam, hbm): the scene's objects, meshes, environment and camera as oracle structures, and
    whether srt_set_scene must place its image in HBM.  n_over: the spheres of the extra "over" (test_gpu_six_waves's grid)"""
    env, cam, meshes = oracle.default_environment(), oracle.default_camera(), []
    base, _, extra = kind.partition("+")
    if base == "indirect":
        objs = oracle.load_scene_json_py(scene_path("Scene_indirect"))
    elif base == "scene1":
        objs = oracle.load_scene_json_py(scene_path("Scene1"))
    elif base == "big":
        objs = _big_scene(oracle)
    elif base == "mesh":  # test_gpu_chain._scene("mesh")
        objs = oracle.load_scene_json_py(scene_path("Scene_indirect"))
        objs.insert(2, dict(type=oracle.OBJ_MESH, position=(0.4, -0.2, 3.0), mesh=0, base=(.9, .3, .2), specular_amount=0.5, smoothness=0.8))
        objs.append(dict(type=oracle.OBJ_MESH, position=(-0.8, 0.2, 3.6), mesh=0, base=(.2, .8, .3), emissive=(0.4, 0.4, 0.1)))
        meshes = [oracle.uv_sphere(0.7, 10, 14)]
    elif base == "clamps":  # test_colours_that_stress_the_clamps's materials and environment
        objs = oracle.load_scene_json_py(scene_path("Scene_indirect"))
        for i, o in enumerate(objs):
            if o.get("type") in (oracle.OBJ_SPHERE, oracle.OBJ_BOX):
                o["base"] = NASTY[i % len(NASTY)]
                o["emissive"] = NASTY[(i + 2) % len(NASTY)] if i % 3 == 0 else o.get("emissive", (0, 0, 0))
                o["specular"] = NASTY[(i + 4) % len(NASTY)] if i % 4 == 0 else o.get("specular", (1, 1, 1))
        env.sky_color = (C.c_float * 3)(-2.0, 3.5, 10.0)
        env.ground_color = (C.c_float * 3)(0.08, -0.0, 0.03)
        env.sun_color = (C.c_float * 3)(500.0, -500.0, 1e6)
    else:
        raise ValueError(kind)
    hbm = base == "big"
    for e in filter(None, extra.split("+")):
        if e in ("r0", "r1e-12", "rinf"):
            _odd_spheres(oracle, objs, {"r0": 0.0, "r1e-12": 1e-12, "rinf": float("inf")}[e])
            hbm = True
        elif e == "farbox":  # a box beyond the NaN-free slab test's bound (KF_BOXES_FINITE off), out of view
            objs.append(dict(type=oracle.OBJ_BOX, position=(0.0, 0.0, -1e30), half_size=(1.0, 1.0, 1.0), base=(.5, .5, .5)))
        elif e == "over":  # so many small spheres that six rows workgroups' LDS no longer fit into a CU: the five-wave rows kernel
            assert n_over > 0
            for k in range(n_over):
                x, y, z, r = _extra_sphere(k)
                objs.append(dict(type=oracle.OBJ_SPHERE, position=(x, y, z), radius=r, base=(.2 + .05 * (k % 13), .8, .3), smoothness=0.7))
        elif e == "nancam":  # every camera ray NaN: the oracle's alpha is NaN in every pixel
            cam.forward = oracle.f3((float("nan"), 0.0, 1.0))
        else:
            raise ValueError(kind)
    oarr, n = oracle.make_objects(objs)
    marr, mn, keep = oracle.make_meshes(meshes) if meshes else (None, 0, None)
    return dict(objs=(oarr, n), meshes=(marr, mn) if mn else None, env=env, cam=cam, hbm=hbm, keep=keep)


def _tracer(srt, sc, w, h):
    pt = srt.PathTracer(w, h)
    if sc["meshes"]:
        pt.set_meshes(C.cast(sc["meshes"][0], C.POINTER(srt.Mesh)), sc["meshes"][1])
    pt.set_environment(srt.Environment.from_buffer_copy(bytes(sc["env"])))
    pt.set_scene(C.cast(sc["objs"][0], C.POINTER(srt.Object)), sc["objs"][1])
    pt.set_camera(srt.Camera.from_buffer_copy(bytes(sc["cam"])))
    return pt


def _placed_in_lds(srt, sc):
    """where srt_set_scene put the image: a counting launch keeps work counts only with the image in LDS"""
    pt = _tracer(srt, sc, 16, 16)
    pt.render(spp=1, bounces=1, seed=0, count_work=True)
    valid = pt.work_counts().valid
    pt.close()
    return valid == 1


def _caller_accumulator(h, w, seed):
    """what a caller may hand in: values in [0, 5], negatives, -0, 1e-38 and a non-zero alpha"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 5.0, (h, w, 4)).astype(np.float32)
    a[..., 3] = rng.uniform(-1.0, 2.0, (h, w)).astype(np.float32)
    a[::3, ::2, 0] = -rng.uniform(0.1, 3.0, a[::3, ::2, 0].shape).astype(np.float32)
    a[1::5, ::3] = -0.0
    a[2::7, 1::4, 1] = 1e-38
    a[::4, 1::5, 2] = -1e-38
    return a


# launch paths: (first launch, resumed launch) keyword arguments of a cell; a frame size, and the path's expected kernel
#   full:   full tiles, 1..8 spp over the whole frame                 chunks: sample chunks on a short band, tapered sample counts
#   small:  small tiles (multi-sample hand-out), >= 16 spp, short band blocks: progressive blocks, one lane per pixel when resumed
#   bgrid:  block grid, steps 4 (a reset, then one sample)            preview: the preview shader;  loop: five one-sample launches
def _path(path, mesh, w, h):
    band = (3, h - 5)
    return {
        "full": (dict(spp=3), dict(spp=5, rows=band)),
        "small": (dict(spp=16, rows=band), dict(spp=17, rows=band)),
        "chunks": (dict(spp=40 if mesh else 65, rows=band), dict(spp=33 if mesh else 70, rows=band)),
        "blocks": (dict(spp=3, steps=3, stripe_width=w // 4 + 1), dict(spp=3, steps=3, stripe_width=w // 4 + 1, rows=band)),
        "bgrid": (dict(spp=2, steps=4), dict(spp=1, steps=4, rows=band)),
        "preview": (dict(spp=1, preview=True, selected=3), dict(spp=2, preview=True, selected=3, rows=band)),
        "loop": (dict(spp=1, loop=5), dict(spp=1, loop=5, rows=band)),
    }[path]


def _cell_name(in_lds, counting, multi, defer, rows=False, six=False):
    """rows, six: the rule's answer for the launch's request (rows_rule.ask)"""
    if rows:
        assert in_lds and not multi and not defer
        return "t_lds_rows" if counting else "k_lds_rows6" if six else "k_lds_rows"
    return ("t_" if counting and in_lds else "k_") + ("lds" if in_lds else "hbm") + ("_defer" if defer else "_multi" if multi else "")


_LDS_BYTES = {}


def _over_count(six_exe):
    if "over" not in _LDS_BYTES:
        _LDS_BYTES["over"] = threshold_counts(six_exe)
    return _LDS_BYTES["over"]


def _rows_lds_bytes(kind, six_exe, tmp_dir):
    """LDS bytes of a rows workgroup for an analytic scene kind whose image lives in LDS, from six_wave_rule_check --grow: the kind's
    scene file (materials, environment and camera do not enter the image's size), a far box appended to a copy of it, the grid's
    spheres given as the program's input"""
    base, _, extra = kind.partition("+")
    extras = set(filter(None, extra.split("+"))) - {"nancam"}
    key = (base if base != "clamps" else "indirect",) + tuple(sorted(extras))
    if key not in _LDS_BYTES:
        path = scene_path({"indirect": "Scene_indirect", "scene1": "Scene1"}[key[0]])
        if "farbox" in extras:
            doc = json.load(open(path))
            doc["SceneObjects"].append({"Material": doc["SceneObjects"][0]["Material"], "Name": "", "Position": [0.0, 0.0, -1e30],
                                        "Renderer": {"Size": [1.0, 1.0, 1.0], "Type": "Cube"}})
            path = os.path.join(str(tmp_dir), "-".join(key) + ".json")
            json.dump(doc, open(path, "w"))
        assert extras <= {"farbox", "over"}, kind
        n = _over_count(six_exe)["over"] if "over" in extras else 0
        _LDS_BYTES[key] = rows_rule.grow(six_exe, path, [_extra_sphere(k) for k in range(n)])[n][1]
    return _LDS_BYTES[key]


# (name it must reach, scene kind, launch path, frame w, h); mesh cells have "mesh" in the kind
ANALYTIC_LDS, ANALYTIC_HBM = ["indirect", "clamps", "scene1+farbox"], ["scene1+r0", "scene1+r1e-12", "clamps+r0", "scene1+farbox+r0", "scene1+rinf"]
CELLS = []
for kind in ANALYTIC_LDS + ["mesh"]:
    # `full` on an analytic scene in LDS (3 and 5 samples) goes through rows; mesh scenes keep the ring
    full, full_counting = ("k_lds", "t_lds") if kind == "mesh" else ("k_lds_rows6", "t_lds_rows")
    CELLS += [(full, kind, "full", 64, 40), ("k_lds_multi", kind, "small", 160, 24), ("k_lds_defer", kind, "chunks", 160, 24),
              (full_counting, kind, "full", 64, 40), ("t_lds_multi", kind, "small", 160, 24), ("t_lds_defer", kind, "chunks", 160, 24),
              ("k_lds_multi", kind, "blocks", 70, 36), ("k_lds_multi", kind, "bgrid", 70, 36), ("k_lds", kind, "preview", 64, 40),
              ("k_lds", kind, "loop", 64, 40)]
# the analytic ring kernel that counts: one-sample launches and the preview shader with SRT_RENDER_COUNT_WORK
CELLS += [("t_lds", kind, "loop", 64, 40) for kind in ANALYTIC_LDS] + [("t_lds", "indirect", "preview", 64, 40)]
# the five-wave rows kernel: Scene1 with the grid of small spheres that takes six workgroups' LDS over a CU's
CELLS += [("k_lds_rows", "scene1+over", "full", 64, 40), ("t_lds_rows", "scene1+over", "full", 64, 40)]
for kind in ANALYTIC_HBM + ["mesh+r0"]:
    CELLS += [("k_hbm", kind, "full", 64, 40), ("k_hbm_multi", kind, "small", 160, 24), ("k_hbm_defer", kind, "chunks", 160, 24),
              ("k_hbm_multi", kind, "blocks", 70, 36), ("k_hbm_multi", kind, "bgrid", 70, 36), ("k_hbm", kind, "preview", 64, 40),
              ("k_hbm", kind, "loop", 64, 40)]
CELLS += [("k_hbm", "big", "full", 48, 32), ("k_hbm_multi", "big", "small", 64, 24), ("k_hbm_defer", "big", "chunks", 48, 24)]
# a band of 256 blocks: the first launch records its work (the TALLY kernel in any case), the resumed one runs with the recorded shape
CELLS += [("t_lds_defer", "indirect", "chunks", 256, 261)]
# every camera ray NaN
CELLS += [("k_lds_rows6", "indirect+nancam", "full", 64, 40), ("k_lds_multi", "indirect+nancam", "bgrid", 70, 36), ("k_lds", "indirect+nancam", "preview", 64, 40),
          ("k_lds_defer", "indirect+nancam", "chunks", 160, 24), ("k_hbm_multi", "scene1+r0+nancam", "small", 160, 24)]


def _cell_id(c):
    return "%s-%s-%s-%s-%dx%d" % ("mesh" if "mesh" in c[1] else "analytic", c[0], c[1], c[2], c[3], c[4])


def _render_both(srt, oracle, pt, sc, w, h, kw, acc_in, bounces, seed, first_sample, reset, counting):
    """one request (a `loop` is that many one-sample launches) through the library and the oracle; returns the oracle's arrays"""
    kw = dict(kw)
    loop = kw.pop("loop", 1)
    spp = kw.pop("spp")
    rows = kw.get("rows")
    oacc, orays, stats = acc_in, [], []
    for i in range(loop):
        call = dict(kw, spp=spp, bounces=bounces, seed=seed, first_sample=first_sample + i * spp, reset=reset and i == 0)
        pt.render(count_rays=True, count_work=counting, **call)
        st = pt.stats()
        stats.append((int(st.rays), int(st.tile_rows), int(st.sample_chunks), int(st.chunk_samples), int(st.shape_source),
                      int(pt.work_counts().valid) if counting else None))
        ofb, oacc, r = oracle.render(sc["objs"][0], sc["objs"][1], sc["env"], sc["cam"], w, h, accumulator=oacc, meshes=sc["meshes"],
                                     threads=ORACLE_THREADS, **call)
        orays.append(r)
    return ofb, oacc, orays, stats, rows


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    return rows_rule.rows_rule_exe(tmp_path_factory)


@pytest.fixture(scope="module")
def six_exe(tmp_path_factory):
    return rows_rule.six_wave_rule_exe(tmp_path_factory)


@pytest.fixture(scope="module")
def cu_count():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS, ids=[_cell_id(c) for c in CELLS])
def test_launch_path_equals_the_oracle(srt, oracle, rule, six_exe, cu_count, tmp_path, cell):
    name, kind, path, w, h = cell
    mesh = "mesh" in kind
    sc = _scene(oracle, kind, _over_count(six_exe)["over"] if "over" in kind else 0)
    in_lds = _placed_in_lds(srt, sc)
    assert in_lds == (not sc["hbm"]), (kind, in_lds)
    counting = name.startswith("t_")
    first, resumed = _path(path, mesh, w, h)
    bounces = 4 if kind == "big" else 6
    pt = _tracer(srt, sc, w, h)
    acc = np.zeros((h, w, 4), np.float32)
    spp1 = first["spp"] * first.get("loop", 1)
    for run, (kw, reset, fs) in enumerate([(first, True, 1), (resumed, False, spp1 + 1)]):
        if not reset:
            acc = _caller_accumulator(h, w, 1000 + len(name) + w)
            pt.write_accumulator(acc)
        ofb, oacc, orays, stats, rows = _render_both(srt, oracle, pt, sc, w, h, kw, acc, bounces, 31 + run, fs, reset, counting)
        # the rule's answer for this request (w x rows: the pixels; a block grid has fewer lanes, and never rows)
        steps = kw.get("steps", 1)
        ans = rows_rule.ask(rule, [dict(w=w, rows=rows[1] - rows[0] if rows is not None else h, spp=kw["spp"], cu_count=cu_count, mesh=mesh,
                                        preview=kw.get("preview", False), steps=steps, block_grid=steps > 1 and (reset or kw["spp"] == 1),
                                        scene_in_lds=in_lds, lds_bytes=_rows_lds_bytes(kind, six_exe, tmp_path) if in_lds and not mesh else 0)])[0]
        for st in stats:
            rays, tile_rows, chunks, chunk_samples, source, valid = st
            multi = tile_rows < 8 or (steps > 1 and not kw.get("preview"))
            defer = chunks >= 2
            print("%s %s %s run %d: tile_rows %d sample_chunks %d chunk_samples %d shape_source %d work_valid %s; rule: rows %d six %d" %
                  (name, kind, path, run, tile_rows, chunks, chunk_samples, source, valid, ans.rows, ans.six))
            if ans.rows:  # (the rule plans a first launch; a recorded band changes only the chunks of 32 samples and more)
                assert (tile_rows, chunks) == (ans.tile_h, ans.chunks) == (8, 1), (st, ans)
            assert _cell_name(in_lds, counting, multi, defer, ans.rows, ans.six) == name, (st, kw, ans)
            assert (chunk_samples > 0) == defer and (tile_rows == 8 or not defer)
            if counting:
                assert valid == 1
        if kw.get("steps", 1) == 1:  # (progressive blocks trace a block's ray once; the oracle's default walk once per pixel)
            assert [s[0] for s in stats] == orays, ("rays", [s[0] for s in stats], orays)
        gacc = pt.accumulator()
        bad = ~np.all(np.where(np.isnan(gacc) | np.isnan(oacc), np.isnan(gacc) & np.isnan(oacc), gacc.view(np.uint32) == oacc.view(np.uint32)), -1)
        assert not bad.any(), (run, int(bad.sum()), np.argwhere(bad)[:8].tolist())
        rb, re_ = rows if rows is not None else (0, h)
        assert np.array_equal(pt.framebuffer(rows=(rb, re_)), ofb[rb:re_]), run
        if "nancam" in kind:
            ys = slice(h - re_, h - rb)
            assert np.isnan(oacc[ys, :, 3]).all() and np.isnan(gacc[ys, :, 3]).all()
        acc = oacc
    if name == "t_lds_defer" and w * h > 60000:
        assert stats[0][4] == 1, "the resumed launch must run with the recorded shape"
    pt.close()


# ---- frame numbers: the running mean's weight is a float divide up to 2^24 and a double divide above (accumulate_sample)
FRAMES = [("full", 2**24 - 2, 5), ("chunks", 2**24 - 2, 65), ("bgrid", 2**24 - 2, 1), ("loop", 2**24 - 2, 1),
          ("full", 2**31 - 1 - 5, 5), ("chunks", 2**31 - 1 - 65, 65)]


@pytest.mark.gpu
@pytest.mark.parametrize("path,first_sample,spp", FRAMES, ids=["%s-%d-%dspp" % f for f in FRAMES])
def test_frame_numbers_past_2_24_and_at_the_limit(srt, oracle, path, first_sample, spp):
    """first_sample = 2^24 - 2 crosses from the float to the double divide inside the launch (loop: five launches across it);
    2^31 - 1 - spp is the largest request srt_render accepts and 2^31 - spp is refused.  Each resumes a caller's accumulator."""
    sc = _scene(oracle, "indirect")
    w, h = (160, 24) if path == "chunks" else (70, 36)
    band = (3, h - 5)
    kw = dict(bounces=5, seed=8, rows=band, reset=False)
    if path == "bgrid":
        kw.update(steps=4)
    pt = _tracer(srt, sc, w, h)
    acc = _caller_accumulator(h, w, first_sample % 1000)
    pt.write_accumulator(acc)
    loop = 5 if path == "loop" else 1
    for i in range(loop):
        pt.render(spp=spp, first_sample=first_sample + i, count_rays=True, **kw)
        st = pt.stats()
        assert (st.sample_chunks >= 2) == (path == "chunks"), path
        ofb, acc, orays = oracle.render(sc["objs"][0], sc["objs"][1], sc["env"], sc["cam"], w, h, spp=spp, first_sample=first_sample + i,
                                        accumulator=acc, threads=ORACLE_THREADS, **kw)
        assert st.rays == orays or path == "bgrid"  # (the block grid traces a block's ray once, the oracle's walk once per pixel)
    assert _same_bits(pt.accumulator(), acc)
    assert np.array_equal(pt.framebuffer(rows=band), ofb[band[0]:band[1]])
    if first_sample + spp == 2**31 - 1:
        with pytest.raises(srt.SrtError) as e:
            pt.render(spp=spp, first_sample=first_sample + 1, **kw)
        assert e.value.code == srt.capi.ERR_INVALID_ARG
        assert _same_bits(pt.accumulator(), acc)  # (a refused request changes nothing)
    pt.close()


# ---- the matrix covers every shipped instantiation
def _shipped_instantiations():
    """(kind, cell name, template arguments) of every pathtrace_kernel<...> that srt_render's shipped (non-SRT_DEV) code launches:
    the cells of launch_pathtrace<MIN_WAVES, MESH>, each named by its comment, for every <MIN_WAVES, MESH> the shipped code calls,
    and the three of launch_pathtrace_rows, which spell their <MIN_WAVES, MESH> out"""
    src = open(os.path.join(ROOT, "software-raytracer_amd", "csrc", "srt_capi.hip")).read()
    shipped, skip = [], 0
    for line in src.split("\n"):  # drop #ifdef SRT_DEV ... #endif blocks
        t = line.strip()
        if t.startswith("#if"):
            skip += 1 if (skip or "SRT_DEV" in t) else 0
            continue
        if t.startswith("#endif") and skip:
            skip -= 1
            continue
        if not skip:
            shipped.append(line)
    src = "\n".join(shipped)
    start = src.index("static void launch_pathtrace(")
    helper = src[start:src.index("\n}\n", start)]
    cells = []
    for line in helper.split("\n"):
        if "pathtrace_kernel<" not in line:
            continue
        m = re.search(r"pathtrace_kernel<MIN_WAVES, MESH, ([^>]*)>.*//\s*(\w+)\s*$", line)
        assert m, "a launch_pathtrace cell without a name: " + line
        cells.append((m.group(1).replace(" ", ""), m.group(2)))
    calls = re.findall(r"\blaunch_pathtrace<(\d+), (true|false)>\(", src)
    assert calls, "srt_render launches no launch_pathtrace<MIN_WAVES, MESH>"
    found = [("mesh" if mesh == "true" else "analytic", name, "%s,%s,%s" % (waves, mesh, args))
             for waves, mesh in calls for args, name in cells]
    start = src.index("static void launch_pathtrace_rows(")
    helper = src[start:src.index("\n}\n", start)]
    for line in helper.split("\n"):
        if "pathtrace_kernel<" not in line:
            continue
        m = re.search(r"pathtrace_kernel<(\d+), (true|false), ([^>]*)>.*//\s*(\w+)\s*$", line)
        assert m, "a launch_pathtrace_rows cell without a name: " + line
        assert m.group(3).replace(" ", "").endswith(",true") and m.group(3).count(",") == 5, "not a ROWS instantiation: " + line
        found.append(("mesh" if m.group(2) == "true" else "analytic", m.group(4), "%s,%s,%s" % (m.group(1), m.group(2), m.group(3).replace(" ", ""))))
    assert re.search(r"\blaunch_pathtrace_rows\(tally, six,", src), "srt_render does not call launch_pathtrace_rows"
    return found


def test_matrix_covers_every_launch_pathtrace_instantiation():
    found = _shipped_instantiations()
    assert len(found) == 21, found
    assert len({f[2] for f in found}) == 21, "an instantiation is named twice"
    assert sorted(n for _, n, _ in found if "rows" in n) == ["k_lds_rows", "k_lds_rows6", "t_lds_rows"]
    shipped = {(k, n) for k, n, _ in found}
    covered = {("mesh" if "mesh" in c[1] else "analytic", c[0]) for c in CELLS}
    assert covered == shipped, ("not covered", sorted(shipped - covered), "not shipped", sorted(covered - shipped))
    assert set(NAMES) == {n for _, n, _ in found}
