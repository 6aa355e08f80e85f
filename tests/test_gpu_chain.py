"""Chained sample chunks at every hand-off point, bit for bit.

In a sample-chunked launch chunk z of a tile either folds its samples straight into the tile's running mean (when the tile's counter
in KernelParams.tile_chain shows chunks 0..z-1 folded) or leaves them in the sample buffer for fold_kernel, which resumes the tile at
the counter's final value.  Which one happens depends on when the hardware runs the workgroups.  The development library
(-DSRT_DEV) can cut chains short (srt_debug_set_chain), force the chunk size and the taper per handle (srt_debug_set_shape) and read
every tile's final counter back (srt_debug_read_chain), so that these tests reach the hand-offs that otherwise only scheduling luck
reaches and can say which ones they did reach."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path
from test_gpu_fuzz import _random_scene

pytestmark = pytest.mark.gpu

NATURAL, OFF, CUT, TILES = 0, 1, 2, 3  # srt_debug_set_chain modes (srt::DEV_CHAIN_*)
ORACLE_THREADS = 16


@pytest.fixture(scope="session")
def dev(srt):
    """libsrt_pathtrace_dev.so, built once (make dev) and opened next to the shipped library."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "software-raytracer_amd", "csrc"), "-s", "dev"], check=True, timeout=900)
    L = srt.capi.open_library(os.path.join(ROOT, "software-raytracer_amd", "libsrt_pathtrace_dev.so"))
    L.srt_debug_set_chain.argtypes = [C.c_void_p, C.c_int, C.c_uint]
    L.srt_debug_set_shape.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.srt_debug_read_chain.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_int)]
    return L


def _scene(oracle, kind):
    """(objects, meshes, camera) as oracle arrays: Scene1, Scene_indirect, a mesh scene, a "far" fuzz scene; "hbm" and "hbm mesh":
    Scene1 and the mesh scene with a sphere of radius 0, which sends the scene image to HBM (outside the short square root's window)."""
    cam, meshes = oracle.default_camera(), []
    if kind in ("mesh", "hbm mesh"):
        objs = oracle.load_scene_json_py(scene_path("Scene_indirect"))
        objs.insert(2, dict(type=oracle.OBJ_MESH, position=(0.4, -0.2, 3.0), mesh=0, base=(.9, .3, .2), specular_amount=0.5, smoothness=0.8))
        objs.append(dict(type=oracle.OBJ_MESH, position=(-0.8, 0.2, 3.6), mesh=0, base=(.2, .8, .3), emissive=(0.4, 0.4, 0.1)))
        meshes = [oracle.uv_sphere(0.7, 10, 14)]
    elif kind == "far":
        objs, meshes, off, scale = _random_scene(oracle, np.random.default_rng(4242), "far")
        cam.position = oracle.f3(off - np.array([0, 0, 6.0]) * scale)
    else:
        objs = oracle.load_scene_json_py(scene_path("Scene1" if kind == "hbm" else kind))
    if kind.startswith("hbm"):
        objs.insert(3, dict(type=oracle.OBJ_SPHERE, position=(0.0, 0.0, 2.0), radius=0.0, base=(.9, .2, .1), emissive=(0.5, 0.5, 0.5)))
    oarr, n = oracle.make_objects(objs)
    marr, mn, keep = oracle.make_meshes(meshes) if meshes else (None, 0, None)
    return dict(objs=(oarr, n), meshes=(marr, mn) if mn else None, cam=cam, keep=keep)


def _tracer(srt, sc, w, h, lib=None):
    pt = srt.PathTracer(w, h, lib=lib)
    if sc["meshes"]:
        pt.set_meshes(C.cast(sc["meshes"][0], C.POINTER(srt.Mesh)), sc["meshes"][1])
    pt.set_scene(C.cast(sc["objs"][0], C.POINTER(srt.Object)), sc["objs"][1])
    pt.set_camera(srt.Camera.from_buffer_copy(bytes(sc["cam"])))
    return pt


def _read_chain(L, pt):
    info = (C.c_int * 6)()
    assert L.srt_debug_read_chain(pt._h, None, None, 0, info) == 0
    tiles = info[3]
    at, cut = np.zeros(tiles, np.uint32), np.zeros(tiles, np.uint32)
    P = C.POINTER(C.c_uint32)
    assert L.srt_debug_read_chain(pt._h, at.ctypes.data_as(P), cut.ctypes.data_as(P), tiles, info) == 0
    return dict(layers=info[0], chunk=info[1], chunk_full=info[2], tiles=tiles, wg_x=info[4], chained=info[5], at=at, cut=cut)


def _layers_tile_the_samples(ch, spp):
    """Layer z traces [first(z), first(z) + count(z)) (srt::chunk_first / chunk_count): together exactly [0, spp), none empty."""
    S, zf, nxt = ch["chunk"], ch["chunk_full"], 0
    for z in range(ch["layers"]):
        first = z * S if z < zf else zf * S + (z - zf) * (S >> 1)
        count = min(spp - first, S if z < zf else S >> 1)
        assert first == nxt and count > 0, (z, first, count, ch)
        nxt = first + count
    assert nxt == spp, ch


def _histogram(ch):
    pairs, counts = np.unique(np.stack([ch["cut"], ch["at"]], 1), axis=0, return_counts=True)
    return {(int(c), int(a)): int(k) for (c, a), k in zip(pairs, counts)}


# (scene, width, height, rows, spp, chunk, taper, resume): the full, half and last chunks differ where the sample count allows
CASES = [
    ("Scene1", 13, 7, None, 65, 24, True, False),              # a frame smaller than one workgroup; chunk 24: the smallest that tapers
    ("Scene1", 96, 64, None, 97, 25, True, False),             # odd chunk (half 12); tiles of nothing but sky
    ("Scene_indirect", 160, 64, (5, 42), 257, 33, True, True),  # 37 rows from row 5; resumed onto a non-zero accumulator
    ("Scene_indirect", 120, 40, (9, 40), 130, 64, True, False),
    ("mesh", 120, 72, (3, 58), 130, 33, True, True),
    ("mesh", 72, 48, None, 97, 24, False, False),               # untapered
    ("far", 100, 60, (0, 45), 130, 25, True, True),
    ("hbm", 96, 64, (2, 61), 97, 25, True, True),               # scene images in HBM
    ("hbm mesh", 120, 72, (3, 58), 130, 33, True, True),
]


@pytest.mark.parametrize("case", CASES, ids=["%s-%dx%d-%s-%dspp-c%d%s%s" % (c[0], c[1], c[2], "band" if c[3] else "frame", c[4], c[5], "" if c[6] else "-untapered",
                                                                          "-resume" if c[7] else "") for c in CASES])
def test_forced_cuts_equal_the_oracle(srt, oracle, dev, case):
    """Every hand-off point of one launch shape against the oracle, bit for bit: no chain (cut 0), a chain cut after each layer
    (k = 1 .. layers: k = chunk_full and k inside the half chunks among them), a cut of its own for every tile, the natural
    schedule and no chain buffer at all.  The counters read back must respect every cut."""
    kind, w, h, rows, spp, chunk, taper, resume = case
    sc = _scene(oracle, kind)
    kw = dict(spp=spp, bounces=6, seed=77, rows=rows)
    acc0 = None
    if resume:
        acc0 = np.random.default_rng(spp).uniform(0, 2, (h, w, 4)).astype(np.float32)
        acc0[..., 3] = 0
        kw.update(first_sample=9, reset=False)
    ofb, oacc, orays = oracle.render(sc["objs"][0], sc["objs"][1], oracle.default_environment(), sc["cam"], w, h, accumulator=acc0,
                                     meshes=sc["meshes"], threads=ORACLE_THREADS, **kw)
    if kind.startswith("hbm"):  # (a counting launch keeps work counts only with the image in LDS)
        probe = _tracer(srt, sc, 16, 16, lib=dev)
        probe.render(spp=1, bounces=1, seed=0, count_work=True)
        assert probe.work_counts().valid == 0, "the scene image must be in HBM"
        probe.close()
    pt = _tracer(srt, sc, w, h, lib=dev)
    assert dev.srt_debug_set_shape(pt._h, chunk, 0 if taper else 1) == 0

    def run(mode, arg=0):
        assert dev.srt_debug_set_chain(pt._h, mode, arg) == 0
        if acc0 is not None:
            pt.write_accumulator(acc0)
        pt.render(count_rays=True, **kw)
        ch = _read_chain(dev, pt)
        what = (mode, arg, _histogram(ch))
        assert pt.stats().rays == orays, what
        acc = pt.accumulator()
        bad = (acc.view(np.uint32) != oacc.view(np.uint32)).any(-1)
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:8].tolist())
        assert np.array_equal(pt.framebuffer(), ofb), what
        assert ch["chunk"] == chunk and ch["layers"] >= 2, ch
        assert ch["chained"] == (mode != OFF)
        at, cut = ch["at"], ch["cut"]
        assert (at <= cut).all() and (at <= ch["layers"]).all() and (cut <= ch["layers"]).all(), what
        return ch

    first = run(CUT, 0)
    layers, zf = first["layers"], first["chunk_full"]
    _layers_tile_the_samples(first, spp)
    assert (first["at"] == 0).all() and (first["cut"] == 0).all()
    if taper:
        assert zf < layers  # (the half chunks exist)
    else:
        assert zf == layers
    # cut 1: chunk 0 of every tile chains (nothing runs before it) and nothing after it: the tiles left at 0 are the ones without a
    # traced pixel (their chunks never touch the counter) — the same tiles under every cut from 1 on
    one = run(CUT, 1)
    assert set(np.unique(one["at"])) <= {0, 1}
    untraced = one["at"] == 0
    assert (~untraced).any()
    if (kind, w, h) == ("Scene1", 96, 64):
        assert untraced.sum() >= 12  # (memory rows 0..15: three blocks of 16 x 16 pixels of sky)
    for k in range(2, layers + 1):
        ch = run(CUT, k)
        assert (ch["cut"] == k).all()
        assert ((ch["at"] == 0) == untraced).all() and (ch["at"] >= 1).sum() == (~untraced).sum()
    for seed in (1, 2, 3):
        ch = run(TILES, seed)
        if ch["tiles"] >= 8:
            assert len(np.unique(ch["cut"])) > 1
        assert (ch["at"][untraced] == 0).all() and (ch["at"][ch["cut"] == 0] == 0).all()
        assert (ch["at"][(ch["cut"] >= 1) & ~untraced] >= 1).all()
    nat = run(NATURAL)
    assert (nat["cut"] == layers).all() and ((nat["at"] == 0) == untraced).all()
    off = run(OFF)
    assert (off["at"] == 0).all()
    pt.close()


def test_wide_band_reaches_every_hand_off(srt, oracle, dev):
    """A 1920-wide launch of many more workgroups per layer than the chip holds at once: a chunk of a tile starts rounds of workgroups
    after the tile's previous chunk, so chains form and the cuts decide where they stop.  Tiles must be seen stopping exactly at the
    cut for k = chunk_full, a k inside the half chunks and a k in the full region — and every launch must equal the launch without a
    chain buffer, bit for bit."""
    sc = _scene(oracle, "Scene1")
    w, h, spp = 1920, 1080, 130
    kw = dict(spp=spp, bounces=4, seed=3, rows=(0, 1080))
    pt = _tracer(srt, sc, w, h, lib=dev)
    assert dev.srt_debug_set_shape(pt._h, 24, 0) == 0
    assert dev.srt_debug_set_chain(pt._h, OFF, 0) == 0
    pt.render(**kw)
    ref_fb, ref_acc = pt.framebuffer(), pt.accumulator()
    base = _read_chain(dev, pt)
    layers, zf = base["layers"], base["chunk_full"]
    assert (layers, zf) == (7, 4)  # 4 x 24 + 12 + 12 + 10
    _layers_tile_the_samples(base, spp)
    seen = {}
    for k in (2, zf, zf + 1, layers - 1):
        assert dev.srt_debug_set_chain(pt._h, CUT, k) == 0
        pt.render(**kw)
        ch = _read_chain(dev, pt)
        assert np.array_equal(pt.accumulator().view(np.uint32), ref_acc.view(np.uint32)) and np.array_equal(pt.framebuffer(), ref_fb), k
        assert (ch["at"] <= k).all()
        hist = _histogram(ch)
        print("wide band, cut %d: (cut, at) -> tiles %s" % (k, sorted(hist.items())))
        seen[k] = int((ch["at"] == k).sum())
    print("wide band: tiles stopping exactly at the cut: %s (of %d tiles)" % (seen, base["tiles"]))
    for k, n in seen.items():
        assert n >= 1000, (k, seen)
    pt.close()


# bands whose layers run side by side: config 3's rows (945, 1080) and (744, 816), a 48-row band, a mesh band.  `handoffs`: the band
# is wide enough for chunks to find their predecessors done (1080 blocks a layer on an MI355X's ~1280 slots: counters at 1..14 were
# seen); in the narrower ones every layer is resident at once and no chain gets past a tile's first chunk (all counters at 0 or 1)
BANDS = [("Scene1", (945, 1080), 512, True), ("Scene1", (744, 816), 512, False), ("Scene1", (500, 548), 384, False), ("mesh", (520, 580), 256, False)]


@pytest.mark.parametrize("kind,rows,spp,handoffs", BANDS, ids=["%s-%d-%d-%dspp" % (b[0], b[1][0], b[1][1], b[2]) for b in BANDS])
def test_natural_hand_offs_equal_no_hand_offs(srt, oracle, dev, kind, rows, spp, handoffs):
    """The shipped library's natural schedule — chains that form and break wherever the hardware puts the workgroups — three times
    over in fresh contexts, against the development library without a chain buffer; the development library's natural schedule
    gives the same bits, and its counters show chains that broke (and, in the band wide enough for it, that went past a tile's
    first chunk: a running mean handed from one workgroup to another)."""
    sc = _scene(oracle, kind)
    w, h = 1920, 1080
    kw = dict(spp=spp, bounces=8, seed=21, rows=rows)

    def frame(lib, mode=None):
        pt = _tracer(srt, sc, w, h, lib=lib)
        if mode is not None:
            assert dev.srt_debug_set_chain(pt._h, mode, 0) == 0
        pt.render(**kw)
        pt.render(**kw)  # (the second launch of a band runs with the recorded work's shape)
        out = pt.framebuffer(), pt.accumulator(), int(pt.stats().sample_chunks), _read_chain(dev, pt) if mode is not None else None
        pt.close()
        return out

    ref_fb, ref_acc, chunks, off = frame(dev, OFF)
    assert chunks >= 2 and off["chained"] == 0
    for _ in range(3):
        fb, acc, c, _ = frame(None)
        assert c == chunks
        assert np.array_equal(acc.view(np.uint32), ref_acc.view(np.uint32)) and np.array_equal(fb, ref_fb)
    fb, acc, c, nat = frame(dev, NATURAL)
    assert c == chunks and nat["layers"] == chunks
    assert np.array_equal(acc.view(np.uint32), ref_acc.view(np.uint32)) and np.array_equal(fb, ref_fb)
    at, layers = nat["at"], nat["layers"]
    print("%s rows %s, %d spp, %d layers (chunk %d, %d full): natural at -> tiles %s" % (kind, rows, spp, layers, nat["chunk"], nat["chunk_full"],
                                                                                       sorted(_histogram(nat).items())))
    assert (at <= layers).all()
    assert ((at > 0) & (at < layers)).any(), "no chain broke"
    if handoffs:
        assert (at > 1).any(), "no chain went past a tile's first chunk"
