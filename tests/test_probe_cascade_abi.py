"""The probe cascade (srt_probe_cascade_params_default, srt_probe_cascade_grids, srt_probe_cascade_weights, srt_set_probe_cascade,
srt_write_ / srt_bind_ / srt_capture_probe_cascade_level, srt_shade_probe_cascade, srt_get_probe_cascade_work; ABI 7 additions)
through ctypes on the built library: the entries are declared and exported inside their own block, the three structs are 160, 40
and 112 bytes in ctypes and in a compiled C program, the constants agree, the header block promises ABI 7 and states rules C1 - C8,
the defaults, srt_probe_cascade_grids against numpy bit for bit, srt_probe_cascade_weights against the reference's rule C2 on a few
thousand random points bit for bit, NULL arguments and bad cascades refused before a device is touched.  No compute: runs without
a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import probe_cascade_reference as PC
import probe_grid_reference as PG
from conftest import ROOT

F = np.float32
ENTRIES = ["srt_probe_cascade_params_default", "srt_probe_cascade_grids", "srt_probe_cascade_weights", "srt_set_probe_cascade",
           "srt_write_probe_cascade_level", "srt_bind_probe_cascade_level", "srt_capture_probe_cascade_level", "srt_shade_probe_cascade",
           "srt_get_probe_cascade_work"]
HEAD = "/* ---- probe cascades:"
NEXT = "/* ---- scrolling probe grids:"
DEFINES = {"SRT_PROBE_CASCADE_NORMAL_WEIGHT": "1", "SRT_PROBE_CASCADE_DEPTH": "2", "SRT_PROBE_CASCADE_STATES": "4", "SRT_PROBE_CASCADE_ALBEDO": "8",
           "SRT_PROBE_CASCADE_COUNT_WORK": "16", "SRT_PROBE_CASCADE_COEFFICIENTS": "1", "SRT_PROBE_CASCADE_MOMENTS": "2", "SRT_PROBE_CASCADE_RECORDS": "4"}
STRUCTS = {"srt_probe_cascade": (160, [("levels", 0), ("resolution", 4), ("blend_cells", 8), ("reserved", 12), ("grid", 16)]),
           "srt_probe_cascade_params": (40, [("row_begin", 0), ("row_end", 4), ("flags", 8), ("band_weight", 12), ("bias", 24), ("min_variance", 28), ("reserved", 32)]),
           "srt_probe_cascade_work": (112, [("valid", 0), ("reserved", 4), ("pixels", 8), ("evaluations", 16), ("blended", 24), ("first_level", 32), ("corners", 64),
                                            ("open", 72), ("wave_trips", 80), ("waves", 88), ("spare", 96)])}


def _header():
    return open(os.path.join(ROOT, "include", "srt_pathtrace.h")).read()


def test_header_declares_and_library_exports_the_entries_in_their_block(srt):
    h = _header()
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    text = strip(h)
    syms = subprocess.run(["nm", "-D", srt.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (srt_[a-z_0-9]+)", syms))
    for n in ENTRIES:
        assert len(re.findall(r"\bint\s+%s\s*\(" % n, text)) == 1, n
        assert srt.capi.EXPORTS.count(n) == 1 and n in exported, n
        assert re.fullmatch(r"srt_[a-z_]+", n)
    a, b = h.index(HEAD), h.index(NEXT)
    assert h.index("/* ---- diagnostics") < a < b  # (in front of the scroll block, whose test pins what follows it)
    assert set(re.findall(r"\b(srt_[a-z_]+)\s*\(", strip(h[a:b]))) == set(ENTRIES)


def test_the_header_block_promises_abi_7_and_states_the_rules(srt):
    h = _header()
    assert C.CDLL(srt.lib_path()).srt_abi_version() == 7 == srt.capi.ABI_VERSION and re.search(r"#define SRT_ABI_VERSION 7\b", h)
    sec = re.search(re.escape(HEAD) + r".*?\*/", h, re.S).group(0)
    assert "(ABI 7, backward compatible)" in sec and "SRT_ABI_VERSION stays 7" in sec
    assert all(("\n * C%d. " % k) in sec for k in range(1, 9))
    block = h[h.index(HEAD):h.index(NEXT)]
    assert dict(re.findall(r"#define (\w+) +(\d+)u\b", block)) == DEFINES
    assert re.search(r"#define SRT_PROBE_CASCADE_MAX_LEVELS 4\b", block) and len(re.findall(r"#define ", block)) == len(DEFINES) + 1


def test_struct_sizes_layouts_and_constants(srt):
    c = srt.capi
    mirrors = {"srt_probe_cascade": c.ProbeCascade, "srt_probe_cascade_params": c.ProbeCascadeParams, "srt_probe_cascade_work": c.ProbeCascadeWork}
    assert srt.ProbeCascade is c.ProbeCascade and srt.ProbeCascadeParams is c.ProbeCascadeParams and srt.ProbeCascadeWork is c.ProbeCascadeWork
    assert srt.probe_cascade_grids is c.probe_cascade_grids and srt.probe_cascade_weights is c.probe_cascade_weights
    assert [C.sizeof(m) for m in mirrors.values()] == [160, 40, 112]
    for name, mirror in mirrors.items():
        size, fields = STRUCTS[name]
        assert C.sizeof(mirror) == size and [(n, getattr(mirror, n).offset) for n, _ in mirror._fields_] == fields, name
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), re.S)
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        names = [x.strip().split("[")[0] for decl in re.findall(r"(?:u?int(?:32|64)_t|float|srt_probe_grid) ([\w, \[\]]+);", body) for x in decl.split(",")]
        assert names == [n for n, _ in mirror._fields_], name
    assert c.PROBE_CASCADE_MAX_LEVELS == PC.MAX_LEVELS == 4
    assert (c.PROBE_CASCADE_NORMAL_WEIGHT, c.PROBE_CASCADE_DEPTH, c.PROBE_CASCADE_STATES, c.PROBE_CASCADE_ALBEDO, c.PROBE_CASCADE_COUNT_WORK) == \
        (PC.NORMAL_WEIGHT, PC.DEPTH, PC.STATES, PC.ALBEDO, PC.COUNT_WORK) == (1, 2, 4, 8, 16)
    assert (c.PROBE_CASCADE_COEFFICIENTS, c.PROBE_CASCADE_MOMENTS, c.PROBE_CASCADE_RECORDS) == (1, 2, 4)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_layout_in_c(tmp_path):
    src = tmp_path / "layout.c"
    fields, want = [], []
    for name, (size, offs) in STRUCTS.items():
        fields.append("sizeof(%s)" % name)
        want.append(str(size))
        for f, o in offs:
            fields.append("offsetof(%s, %s)" % (name, f))
            want.append(str(o))
    consts = sorted(DEFINES) + ["SRT_PROBE_CASCADE_MAX_LEVELS"]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "srt_pathtrace.h"\nint main(void) { printf("%s%s\\n", %s, %s); return 0; }\n' %
                   ("%zu " * len(fields), "%u " * len(consts), ", ".join(fields), ", ".join("(unsigned)" + k for k in consts)))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert got == want + [DEFINES[k] for k in sorted(DEFINES)] + ["4"]


def test_defaults_and_refusals_without_a_gpu(srt):
    L = srt.load_library()
    c = srt.capi
    bad = c.ERR_INVALID_ARG
    p = c.ProbeCascadeParams(7, 7, 0xFFFFFFFF, (C.c_float * 3)(7, 7, 7), 7.0, 7.0, (C.c_uint32 * 2)(7, 7))
    assert L.srt_probe_cascade_params_default(C.byref(p)) == c.OK
    assert (p.row_begin, p.row_end, p.flags, tuple(p.reserved)) == (0, 0, 0, (0, 0))
    g = c.ProbeGridParams()
    d = c.ProbeGridDepthParams()
    assert L.srt_probe_grid_params_default(C.byref(g)) == c.OK and L.srt_probe_grid_depth_params_default(C.byref(d)) == c.OK
    assert np.array_equal(np.array(p.band_weight[:], F).view(np.uint32), np.array(PG.IRRADIANCE, F).view(np.uint32)) and p.band_weight[:] == g.band_weight[:]
    assert (p.bias, p.min_variance) == (d.bias, d.min_variance) == (0.0, float(F(1e-4)))  # srt_probe_grid_depth_params_default is the authority
    assert L.srt_probe_cascade_params_default(None) == bad
    w = c.ProbeCascadeWork()
    k = c.probe_cascade([((0, 0, 0), (1, 1, 1), (3, 3, 3))])
    f3, i3 = (C.c_float * 3)(0, 0, 0), (C.c_int32 * 3)(3, 3, 3)
    one, two, beta = C.c_int32(), C.c_int32(), C.c_float()
    assert L.srt_set_probe_cascade(None, C.byref(k)) == bad and L.srt_shade_probe_cascade(None, C.byref(p)) == bad
    assert L.srt_get_probe_cascade_work(None, C.byref(w)) == bad and L.srt_capture_probe_cascade_level(None, 0, 1) == bad
    assert L.srt_write_probe_cascade_level(None, 0, 1, f3, 1) == bad and L.srt_bind_probe_cascade_level(None, 0, 1, None, 0) == bad
    s3 = (C.c_float * 3)(1, 1, 1)
    for args in ((None, s3, i3, 1, C.byref(k)), (f3, None, i3, 1, C.byref(k)), (f3, s3, None, 1, C.byref(k)), (f3, s3, i3, 1, None), (f3, s3, i3, 0, C.byref(k)),
                 (f3, s3, i3, 5, C.byref(k))):
        assert L.srt_probe_cascade_grids(*args) == bad
    for args in ((None, f3, C.byref(one), C.byref(two), C.byref(beta)), (C.byref(k), None, C.byref(one), C.byref(two), C.byref(beta)),
                 (C.byref(k), f3, None, C.byref(two), C.byref(beta)), (C.byref(k), f3, C.byref(one), None, C.byref(beta)), (C.byref(k), f3, C.byref(one), C.byref(two), None)):
        assert L.srt_probe_cascade_weights(*args) == bad
    # cascades srt_set_probe_cascade refuses are refused here too
    nan, inf = float("nan"), float("inf")
    for kw in (dict(levels=0), dict(levels=5), dict(resolution=5), dict(blend_cells=0.0), dict(blend_cells=-1.0), dict(blend_cells=nan), dict(blend_cells=inf),
               dict(reserved=1)):
        k2 = c.probe_cascade([((0, 0, 0), (1, 1, 1), (3, 3, 3))])
        for name, v in kw.items():
            setattr(k2, name, v)
        assert L.srt_probe_cascade_weights(C.byref(k2), f3, C.byref(one), C.byref(two), C.byref(beta)) == bad, kw
    for grid in (((0, 0, 0), (1, 1, 1), (0, 3, 3)), ((0, 0, 0), (1, 0, 1), (3, 3, 3)), ((0, nan, 0), (1, 1, 1), (3, 3, 3)), ((0, 0, 0), (1, 1, inf), (3, 3, 3))):
        k2 = c.probe_cascade([((0, 0, 0), (1, 1, 1), (3, 3, 3)), grid])
        assert L.srt_probe_cascade_weights(C.byref(k2), f3, C.byref(one), C.byref(two), C.byref(beta)) == bad, grid
        with pytest.raises(srt.SrtError):
            srt.probe_cascade_weights(k2, (0, 0, 0))


CASES = [((0.3, -1.7, 4.0), (0.5, 0.5, 0.25), (5, 4, 1), 3),        # a negative centre, an even count, an axis of one probe
         ((-0.37, 0.9, 4.6), (0.4, 0.3, 0.7), (6, 5, 8), 4),        # spacings that are no powers of two
         ((-123.456, 77.7, -0.001), (1.25, 0.8, 1.5), (2, 2, 2), 2),
         ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 1, 1), 1),
         ((1e30, -1e30, float("nan")), (1e-3, 1e3, 3.0), (67, 5, 2), 4)]  # the clamp at +-1048576 and the NaN


@pytest.mark.parametrize("case", CASES)
def test_grids_against_numpy_bit_for_bit(srt, case):
    centre, base, counts, levels = case
    got = srt.probe_cascade_grids(centre, base, counts, levels)
    want = PC.grids(centre, base, counts, levels)
    assert (got.levels, got.resolution, got.blend_cells, got.reserved) == (levels, 0, 1.0, 0)
    for l in range(levels):
        g, w = got.grid[l], want.grids[l]
        assert np.array_equal(np.array(g.origin[:], F).view(np.uint32), w.origin.view(np.uint32)), (l, g.origin[:], w.origin)
        assert np.array_equal(np.array(g.spacing[:], F).view(np.uint32), w.spacing.view(np.uint32)) and tuple(g.counts[:]) == tuple(counts)
        assert np.array_equal(w.spacing, np.ldexp(np.asarray(base, F), l))
    for l in range(levels, 4):
        assert tuple(got.grid[l].counts[:]) == (0, 0, 0)


def test_grids_by_hand(srt):
    got = srt.probe_cascade_grids((0.3, -1.7, 4.0), (0.5, 0.5, 0.25), (5, 4, 1), 3)
    # level 0: k = floor(0.6), floor(-3.4), floor(16) = 0, -4, 16 and (n - 1) / 2 = 2, 1, 0
    assert got.grid[0].origin[:] == [-1.0, -2.5, 4.0] and got.grid[2].origin[:] == [-4.0, -4.0, 4.0] and got.grid[2].spacing[:] == [2.0, 2.0, 1.0]
    # the origin is a whole number of cells of the level's own spacing
    for l in range(3):
        g = got.grid[l]
        assert all(float(g.origin[a] / g.spacing[a]).is_integer() for a in range(3))


def _cascade_of(ref, c):
    return c.probe_cascade([(g.origin, g.spacing, g.counts) for g in ref.grids], ref.resolution, float(ref.blend_cells))


@pytest.mark.parametrize("seed,blend,counts", [(1, 1.0, (5, 5, 5)), (2, 0.5, (6, 4, 7)), (3, 2.5, (5, 1, 4)), (4, 0.75, (2, 2, 2))])
def test_weights_against_the_reference_on_random_points(srt, seed, blend, counts):
    """Four thousand points around a cascade of three levels: uniform over twice the coarsest level's box, plus points exactly on
    faces and band edges of every level, NaN and +-inf.  first_level, evaluations and beta, bit for bit."""
    c = srt.capi
    L = srt.load_library()
    rng = np.random.default_rng(seed)
    ref = PC.grids((0.1, -0.2, 4.0), (0.5, 0.25, 0.4), counts, 3)
    ref.blend_cells = F(blend)
    k = _cascade_of(ref, c)
    top = ref.grids[2]
    lo = top.origin.astype(np.float64)
    hi = lo + (np.array(top.counts) - 1) * top.spacing.astype(np.float64)
    mid, half = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1.0)
    pts = (mid + rng.uniform(-2.0, 2.0, (3600, 3)) * half).astype(F)
    near = (mid + rng.uniform(-1.0, 1.0, (360, 3)) * (half / 4)).astype(F)  # the finest level
    edge = []
    for g in ref.grids:
        for a in range(3):
            for cells in (0.0, float(blend), g.counts[a] - 1 - float(blend), g.counts[a] - 1.0):
                p = mid.astype(F).copy()
                p[a] = F(g.origin[a] + F(F(cells) * g.spacing[a]))
                edge.append(p)
    wild = [np.array(v, F) for v in ((np.nan, 0, 4), (0, np.inf, 4), (0, 0, -np.inf), (np.nan, np.nan, np.nan), (3e38, -3e38, 0))]
    pts = np.concatenate([pts, near, np.array(edge, F), np.array(wild, F)])
    f, n, beta = PC.weights(ref, pts)
    one, two, b = C.c_int32(), C.c_int32(), C.c_float()
    for i, p in enumerate(pts):
        assert L.srt_probe_cascade_weights(C.byref(k), (C.c_float * 3)(*p.tolist()), C.byref(one), C.byref(two), C.byref(b)) == c.OK
        got = (one.value, two.value, np.array([b.value], F).view(np.uint32)[0])
        assert got == (f[i], n[i], beta[i:i + 1].view(np.uint32)[0]), (p, got, f[i], n[i], beta[i])
    assert srt.probe_cascade_weights(k, pts[0]) == (f[0], n[0], beta[0])
    # the condition on the points: every first level, both evaluation counts, points no level holds
    cls = PC.classes(ref, pts)
    # (a level whose narrowest axis is less than two bands wide has no point a whole band from every face: it is blended everywhere)
    roomy = (min(n_ for n_ in counts if n_ > 1) - 1) / 2 >= blend
    want = {PC.BLENDED + 0, PC.BLENDED + 1, PC.SINGLE + 2, PC.OUTSIDE} | ({PC.SINGLE + 0, PC.SINGLE + 1} if roomy else set())
    assert want <= set(cls.tolist()), sorted(set(cls.tolist()))


def test_the_reference_by_hand():
    """Rule C2 on three levels of 5 x 5 x 5 probes centred on (0, 0, 4), spacings 0.5 / 1 / 2, and rule C3 on two made-up levels."""
    ref = PC.Cascade([PG.Grid((-2.0 * s, -2.0 * s, 4.0 - 2.0 * s), (s, s, s), (5, 5, 5)) for s in (0.5, 1.0, 2.0)])
    pts = np.array([(0, 0, 4), (0.75, 0, 4), (1, 0, 4), (1.5, 0, 4), (2, 0, 4), (3, 0, 4), (4, 0, 4), (9, 0, 4), (np.nan, 0, 4)], F)
    f, n, beta = PC.weights(ref, pts)
    assert f.tolist() == [0, 0, 1, 1, 2, 2, 2, 2, 2] and n.tolist() == [1, 2, 1, 2, 1, 1, 1, 1, 1]
    assert beta.tolist() == [1.0, 0.5, 1.0, 0.5, 1.0, 0.5, 0.0, 0.0, 0.0]
    assert PC.classes(ref, pts).tolist() == [PC.SINGLE, PC.BLENDED, PC.SINGLE + 1, PC.BLENDED + 1, PC.SINGLE + 2, PC.SINGLE + 2, PC.OUTSIDE, PC.OUTSIDE, PC.OUTSIDE]


def test_python_layer_has_the_new_entries(srt):
    for n in ("set_probe_cascade", "write_probe_cascade_level", "bind_probe_cascade_level", "capture_probe_cascade_level", "shade_probe_cascade",
              "probe_cascade_work"):
        assert callable(getattr(srt.PathTracer, n)), n
