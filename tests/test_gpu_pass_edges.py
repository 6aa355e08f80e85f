"""The upsample, anti-aliasing, variance and moving-object passes at the edges of their contracts on the MI355X: frames of one
pixel, one row or one column, sizes around the 8 x 8 tile and the 16 x 16 workgroup and the 256-thread block, block sizes and
stripes larger than the frame, sigmas, depths, variances and displacements at 0, a subnormal, FLT_MAX and inf on inputs with
exact ties, row bands at the tile boundary, object borders on the seams of the variance filter's LDS tile, and object indices
beyond the motion table.  The float64 definitions are the existing ones (test_gpu_upsample.reference, antialias_reference,
variance_reference, test_gpu_motion.motion_reference, the oracle); tests/test_pass_references.py checks on the CPU that they
survive these inputs and how many pixels they leave undecided."""
import ctypes as C
import json

import numpy as np
import pytest

import pass_edge_inputs as pe
import test_gpu_antialias as aa
import test_gpu_denoise as dn
import test_gpu_filter_edges as fe
import test_gpu_motion as mo
import test_gpu_temporal as tp
import test_gpu_upsample as up
import test_gpu_variance as tv
import variance_reference as vr
from antialias_reference import resolve
from pass_edge_inputs import F32_MAX, INF, SHAPES

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _rel(got, ref):
    """Per pixel: the largest relative error of the rgb channels."""
    g, r = np.asarray(got)[..., :3].astype(np.float64), np.asarray(ref)[..., :3].astype(np.float64)
    with np.errstate(all="ignore"):
        return np.max(np.abs(g - r) / np.maximum(np.abs(r), 1e-6), axis=-1)


def _error_lines(test, case, w, h, by_level):
    """The maxima per level count, as lines of profiles/denoise/variance_error.jsonl (the schema tests/test_gpu_variance.py prints)."""
    for levels, err in sorted(by_level.items()):
        print("variance_error " + json.dumps({"test": test, "case": case, "width": w, "height": h, "iterations": levels, "max_rel_err": err,
                                              "bound": dn.REL_TOL}))


# ---- a. srt_upsample at every shape -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES)
def test_upsample_at_every_shape(srt, w, h):
    acc, obj, nd, pos, _ = pe.guides(w, h, pe.shape_seed(w, h))
    pt = srt.PathTracer(w, h)
    keep = up._bind(pt, obj, nd, pos)
    pt.write_accumulator(acc)
    worst, compared, left_out = 0.0, 0, 0
    for steps in pe.UPSAMPLE_STEPS:
        for stripe in dict.fromkeys(pe.upsample_stripes(w)):
            for sn, sx in pe.UPSAMPLE_SIGMAS:
                case = (w, h, steps, stripe, sn, sx)
                pt.upsample(steps=steps, stripe_width=stripe, sigma_normal=sn, sigma_plane=sx, gbuffer=False)
                got = pt.upsampled()
                ref, anchor, solved = up.reference(acc, obj, nd, pos, steps, stripe, sn, sx)
                chk = solved & np.isfinite(ref[..., :3]).all(-1)
                left_out += int((solved & ~chk).sum())
                compared += int(chk.sum())
                err = _rel(got, ref)
                if chk.any():
                    worst = max(worst, float(err[chk].max()))
                    assert err[chk].max() <= up.REL_TOL, (case, float(err[chk].max()))
                assert _same_bits(got[..., 3], acc[..., 3]), ("alpha is not the input's", case)
                assert _same_bits(got[anchor], acc[anchor]), ("an anchor pixel changed", case)
                assert _same_bits(got[~solved], acc[~solved]), ("a pixel without a counting tap changed", case)
                if steps == 1:
                    assert _same_bits(got, acc), ("steps = 1 is not the identity", case)
    print("pass_edges upsample %dx%d: max relative error %.3g over %d compared pixels, %d left out" % (w, h, worst, compared, left_out))
    assert left_out <= 0.01 * (compared + left_out)
    if w * h > 1:
        assert compared >= w * h, "hardly any pixel was compared"
    else:
        assert compared == 0  # the one pixel is an anchor at every block size
    # the in-place form: only the rgb of non-anchor pixels may change, and a second call gives the same bits
    kw = dict(steps=2, stripe_width=0, sigma_normal=32.0, sigma_plane=0.02, gbuffer=False)
    pt.upsample(**kw)
    out = pt.upsampled()
    _, anchor, solved = up.reference(acc, obj, nd, pos, 2, 0, 32.0, 0.02)
    pt.upsample(in_place=True, **kw)
    one = pt.accumulator()
    assert _same_bits(one[anchor], acc[anchor]) and _same_bits(one[..., 3], acc[..., 3]) and _same_bits(one[~solved], acc[~solved])
    assert _same_bits(one[..., :3], out[..., :3])
    pt.upsample(in_place=True, **kw)
    assert _same_bits(pt.accumulator(), one), "a second in-place call changed the accumulator"
    if (w, h) in ((1, 1), (17, 15), (300, 1)):
        pt.write_accumulator(acc)
        pt.upsample(framebuffer=True, **kw)
        assert _same_bits(pt.upsampled(), out)
        assert np.array_equal(pt.framebuffer(), up.tone_map(out)[::-1])
    pt.close()
    del keep


# ---- b. srt_upsample parameter extremes on exact ties -----------------------------------------------------------------------
@pytest.mark.parametrize("sx", pe.TIE_SIGMA_PLANE, ids=["x%g" % v for v in pe.TIE_SIGMA_PLANE])
@pytest.mark.parametrize("sn", pe.TIE_SIGMA_NORMAL, ids=["n%g" % v for v in pe.TIE_SIGMA_NORMAL])
def test_upsample_parameter_extremes(srt, sn, sx):
    """Every weight is exactly 0 or b_q, in binary32 and in float64: the result is the plain bilinear mix of the counted anchors
    whatever the sigmas and whatever d_p (2.5, 0, -2, 1e-38 and inf per object), no pixel is left out, and the object whose
    anchors are perpendicular to its other pixels keeps its bits."""
    w, h, steps, stripe = pe.TIE_W, pe.TIE_H, pe.TIE_STEPS, pe.TIE_STRIPE
    acc, obj, nd, pos = pe.upsample_tie_guides()
    pt = srt.PathTracer(w, h)
    keep = up._bind(pt, obj, nd, pos)
    pt.write_accumulator(acc)
    pt.upsample(steps=steps, stripe_width=stripe, sigma_normal=sn, sigma_plane=sx, gbuffer=False)
    got = pt.upsampled()
    ref, anchor, solved = up.reference(acc, obj, nd, pos, steps, stripe, sn, sx)
    plain, _, plain_solved = up.reference(acc, obj, nd, pos, steps, stripe, 0.0, 0.0)
    perp = obj == pe.TIE_PERP
    assert np.isfinite(ref).all(), "the definition is not finite on the tie guides"
    assert np.array_equal(solved, plain_solved & ~perp) and np.allclose(ref[solved], plain[solved], rtol=1e-12)
    assert np.isfinite(got).all(), (int((~np.isfinite(got)).any(-1).sum()), np.unique(obj[(~np.isfinite(got)).any(-1)]).tolist())
    err = _rel(got, ref)
    print("pass_edges upsample ties sigma_normal %g sigma_plane %g: max relative error %.3g over %d pixels" % (sn, sx, err[solved].max(), solved.sum()))
    assert solved.sum() > 300 and all((solved & (obj == k)).sum() > 20 for k in range(-1, pe.TIE_PERP))
    assert err[solved].max() <= up.REL_TOL
    assert (perp & ~anchor).sum() > 40 and _same_bits(got[perp], acc[perp]), "a weight sum of exactly 0 changed the pixel"
    assert _same_bits(got[~solved], acc[~solved]) and _same_bits(got[..., 3], acc[..., 3])
    pt.close()
    del keep


@pytest.mark.parametrize("sx", [F32_MAX, INF], ids=["xmax", "xinf"])
@pytest.mark.parametrize("which", ["denoise", "denoise_variance"])
def test_filters_with_an_infinite_sigma_plane_on_the_tie_guides(srt, which, sx):
    """srt_denoise and srt_denoise_variance take the same clamped plane scale: on the tie guides (d_p of 2.5, 0, -2, 1e-38 and
    inf) with sigma_normal = 128 and sigma_plane at FLT_MAX or inf every tap of the pixel's object weighs exactly h(dx) h(dy),
    so the result is that of both terms off, bit for bit, on every object but the one with perpendicular normals — in
    particular finite at d_p = 0, where 1 / (inf * 0) would be NaN."""
    w, h = pe.TIE_W, pe.TIE_H
    acc, obj, nd, pos = pe.upsample_tie_guides()
    alb = np.zeros((h, w, 4), np.float32)
    hit = obj >= 0
    pt = srt.PathTracer(w, h)
    keep = tv._bind(pt, obj, nd, pos, alb)
    keep["variance"] = tv._cuda(np.full((h, w), 0.125, np.float32))
    pt.bind_variance(keep["variance"])
    pt.write_accumulator(acc)
    for levels in (1, 3):
        def run(sn, sp):
            if which == "denoise":
                pt.denoise(iterations=levels, sigma_color=0.0, sigma_normal=sn, sigma_plane=sp, albedo=False, gbuffer=False)
            else:
                pt.denoise_variance(iterations=levels, sigma_luminance=0.0, sigma_normal=sn, sigma_plane=sp, albedo=False, gbuffer=False)
            return pt.denoised()

        off = run(0.0, 0.0)
        ref = dn.reference(acc, obj, nd, pos, alb, levels, 0.0, 0.0, 0.0, False)
        assert _rel(off, ref)[hit].max() <= dn.REL_TOL and not _same_bits(off[hit], acc[hit])
        got = run(128.0, sx)
        assert np.isfinite(got[hit]).all(), (levels, "non-finite on objects", np.unique(obj[hit & ~np.isfinite(got).all(-1)]).tolist())
        same = hit & (obj != pe.TIE_PERP)
        assert same.sum() > 500 and _same_bits(got[same], off[same]), (levels, "an exact tie does not weigh 1")
        assert _same_bits(got[~hit], acc[~hit]) and _same_bits(got[..., 3], acc[..., 3])
    pt.close()
    del keep


# ---- c. srt_render_subsamples against the oracle at every shape -------------------------------------------------------------
def oracle_subsamples(oracle, sc, w, h, k):
    """The (K, H, W) planes by definition, as test_gpu_antialias._expected computes them: srt_oracle_closest_m along
    srt_oracle_ray_direction of the 2kW x 2kH virtual frame, default camera."""
    L = oracle.lib()
    ocam = oracle.default_camera()
    marr, mn = sc["meshes"] if sc["meshes"] else (None, 0)
    d, nn, pp, t = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)(), C.c_float()
    origin = (C.c_float * 3)(*ocam.position)
    out = np.empty((k * k, h, w), np.int32)
    for s in range(k * k):
        i, j = s % k, s // k
        for y in range(h):
            for x in range(w):
                L.srt_oracle_ray_direction(C.byref(ocam), 2 * k * w, 2 * k * h, 2 * k * x + 2 * i - (k - 1), 2 * k * y + 2 * j - (k - 1), d)
                out[s, y, x] = L.srt_oracle_closest_m(sc["oarr"], sc["n"], marr, mn, origin, d, nn, pp, C.byref(t))
    return out


@pytest.mark.parametrize("kind,ks", [("Scene1", (1, 2, 3, 4)), ("Scene1 mesh", (2, 4)), ("Scene1 inside", (2, 4))])
def test_subsamples_equal_the_oracle_at_every_shape(srt, oracle, kind, ks):
    sc = fe._scene(oracle, kind)
    compared = hits = foreign = 0
    for w, h in SHAPES:
        pt = fe._tracer(srt, sc, w, h)
        pt.render_gbuffer(outputs=srt.capi.GBUF_OBJECT)
        obj = pt.gbuffer("object")
        for k in ks:
            if w * h >= 300 and max(w, h) == 300 and k not in (1, 4):
                continue  # (the cap on the oracle loop)
            want = oracle_subsamples(oracle, sc, w, h, k)
            pt.render_subsamples(k)
            got = pt.subsamples()
            assert np.array_equal(got, want), (kind, w, h, k, "%d of %d sub-samples differ" % (int((got != want).sum()), want.size))
            if k in (1, 3):
                assert np.array_equal(got[(k * k) // 2], obj), (kind, w, h, k)
            compared += want.size
            hits += int((want >= 0).sum())
            foreign += int((got != obj[None]).sum())
        pt.close()
    print("pass_edges subsamples %s: %d compared, %d hits, %d see another object than their pixel" % (kind, compared, hits, foreign))
    assert compared > 20000 and hits > compared // 4
    if kind == "Scene1 inside":  # every ray ends on the sphere around the camera
        assert hits == compared and foreign == 0
    else:
        assert foreign > 100


@pytest.mark.parametrize("k", [2, 3])
def test_subsample_bands_at_the_tile_boundary(srt, oracle, k):
    import torch

    w, h, sentinel = 37, 21, -77
    sc = fe._scene(oracle, "Scene1")
    want = oracle_subsamples(oracle, sc, w, h, k)
    pt = fe._tracer(srt, sc, w, h)
    for r0, r1 in ((0, 1), (7, 8), (8, 9), (7, 9), (h - 1, h), (0, h)):
        buf = torch.full((k * k, h, w), sentinel, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        pt.bind_subsamples(buf)
        pt.render_subsamples(k, rows=(r0, r1))
        pt.wait()
        band = buf.cpu().numpy()
        y0, y1 = h - r1, h - r0
        assert np.array_equal(band[:, y0:y1], want[:, y0:y1]), (r0, r1)
        assert np.all(band[:, :y0] == sentinel) and np.all(band[:, y1:] == sentinel), (r0, r1, "a row outside the band was written")
        pt.bind_subsamples(None)
        del buf
    assert len(np.unique(want)) > 5
    pt.close()


# ---- d. srt_antialias at every shape ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["accumulator", "denoised"])
def test_antialias_at_every_shape(srt, source):
    den = source == "denoised"
    worst, compared, left_out = 0.0, 0, 0
    for w, h in SHAPES:
        for k in (1, 2, 3, 4):
            c, obj, sub, other = pe.antialias_inputs(w, h, k)
            pt, keep = aa._bound_tracer(srt, other if den else c, obj, sub, denoised=c if den else other)
            pt.antialias(k, denoised=den, guides=False)
            got = pt.antialiased()
            ref, foreign, changed = resolve(c, obj, sub)
            chk = changed & np.isfinite(ref[..., :3]).all(-1)
            left_out += int((changed & ~chk).sum())
            compared += int(chk.sum())
            if chk.any():
                err = float(_rel(got, ref)[chk].max())
                worst = max(worst, err)
                assert err <= aa.REL_TOL, (w, h, k, err)
            assert _same_bits(got[~changed], c[~changed]), (w, h, k, "an unchanged pixel lost its bits")
            assert _same_bits(got[..., 3], c[..., 3]), (w, h, k, "alpha is not the input's")
            if k == 1 or (w, h) == (1, 1):  # the footprint is the pixel itself / every tap lies outside the frame
                assert not changed.any() and _same_bits(got, c), (w, h, k)
            if (w, h) in ((1, 1), (17, 15), (300, 1)) and k in (1, 3):
                pt.antialias(k, denoised=den, framebuffer=True, guides=False)
                assert _same_bits(pt.antialiased(), got)
                assert np.array_equal(pt.framebuffer(), up.tone_map(got)[::-1]), (w, h, k)
            pt.close()
            del keep
    print("pass_edges antialias %s: max relative error %.3g over %d changed pixels, %d left out" % (source, worst, compared, left_out))
    assert left_out <= 0.01 * (compared + left_out) and compared > 500


# ---- e. srt_variance at every shape -----------------------------------------------------------------------------------------
def test_variance_at_every_shape(srt):
    worst, compared = 0.0, 0
    bound = 2 * tv.EST_ROUNDINGS * tv.U
    for w, h in SHAPES + [(255, 1), (16, 16), (257, 1)]:  # pixel counts 1 .. 300 with 255, 256 and 257: the ends of the 256-thread blocks
        _, obj, nd, pos, alb = pe.guides(w, h, pe.shape_seed(w, h))
        hit = obj >= 0
        a, b = pe.halves(w, h, 5, alb)
        pt = srt.PathTracer(w, h)
        keep = tv._bind(pt, obj, nd, pos, alb)

        def run(a_, b_, albedo, merge):
            tb = tv._cuda(b_)
            pt.bind_half(tb)
            pt.write_accumulator(a_)
            pt.variance(albedo=albedo, merge=merge, gbuffer=False)
            v, acc = pt.variance_map(), pt.accumulator()
            assert _same_bits(tb.cpu().numpy(), b_), "half B was written"
            return v, acc

        for albedo in (False, True):
            what = (w, h, albedo)
            v, acc = run(a, a.copy(), albedo, True)
            assert not _bits(v).any() and _same_bits(acc, a), (what, "equal halves")
            v0, acc = run(a, b, albedo, False)
            assert _same_bits(acc, a), (what, "the accumulator was written without MERGE")
            v1, acc = run(a, b, albedo, True)
            mean32 = np.float32(0.5) * a[..., :3] + np.float32(0.5) * b[..., :3]
            assert _same_bits(acc[..., :3], mean32) and _same_bits(acc[..., 3], a[..., 3]) and _same_bits(v0, v1), what
            v2, acc2 = run(b, a, albedo, True)
            assert _same_bits(v2, v1) and _same_bits(acc2[..., :3], acc[..., :3]) and _same_bits(acc2[..., 3], b[..., 3]), (what, "swapped halves")
            assert not _bits(v1[~hit]).any(), (what, "a miss has a variance")
            ref, _ = vr.variance(a, b, obj, alb, albedo)
            m = vr.demod(alb, albedo)
            s = 0.5 * vr.lum(a[..., :3].astype(np.float64) / m) + 0.5 * vr.lum(b[..., :3].astype(np.float64) / m)
            assert np.isfinite(ref).all()
            err = np.abs(v1.astype(np.float64) - ref) / (s * s)
            worst = max(worst, float(err[hit].max()))
            compared += int(hit.sum())
            assert err[hit].max() <= bound, (what, float(err[hit].max()))
        pt.bind_half(None)
        pt.close()
        del keep
    print("pass_edges variance estimate: max |v - v_ref| / S^2 = %.3g (bound %.3g) over %d pixels" % (worst, bound, compared))
    assert compared > 4000


# ---- f. srt_denoise_variance at every shape ---------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES)
def test_denoise_variance_at_every_shape(srt, w, h):
    acc, obj, nd, pos, alb = pe.guides(w, h, pe.shape_seed(w, h))
    var = pe.variance_field(w, h, 9)
    hit = obj >= 0
    pt = srt.PathTracer(w, h)
    keep = tv._bind(pt, obj, nd, pos, alb)
    keep["variance"] = tv._cuda(var)
    pt.bind_variance(keep["variance"])
    pt.write_accumulator(acc)
    worst, compared, left_out = 0.0, 0, 0
    results, by_level = {}, {}
    for levels in pe.FILTER_LEVELS + [5]:
        for albedo in (False, True):
            for sl in pe.FILTER_SIGMAS:
                case = (w, h, levels, albedo, sl)
                pt.denoise_variance(iterations=levels, sigma_luminance=sl, sigma_normal=32.0, sigma_plane=0.02, albedo=albedo, gbuffer=False)
                got = pt.denoised()
                results[(levels, albedo, sl)] = got
                ref = vr.denoise_variance(acc, var, obj, nd, pos, alb, levels, sl, 32.0, 0.02, albedo)
                chk = hit & np.isfinite(ref[..., :3]).all(-1)
                left_out += int((hit & ~chk).sum())
                compared += int(chk.sum())
                err = float(_rel(got, ref)[chk].max())
                worst = max(worst, err)
                by_level[levels] = max(by_level.get(levels, 0.0), err)
                assert err <= dn.REL_TOL, (case, err)
                assert _same_bits(got[..., 3], acc[..., 3]), (case, "alpha is not the input's")
                assert _same_bits(got[~hit], acc[~hit]), (case, "miss pixels are not the input")
                if sl == 0.0:
                    pt.denoise(iterations=levels, sigma_color=0.0, sigma_normal=32.0, sigma_plane=0.02, albedo=albedo, gbuffer=False)
                    assert _same_bits(pt.denoised(), got), (case, "sigma_luminance = 0 is not srt_denoise(sigma_color = 0)")
    assert _same_bits(keep["variance"].cpu().numpy(), var), "the variance buffer was written"
    _error_lines("test_denoise_variance_at_every_shape", "synthetic guides", w, h, by_level)
    print("pass_edges denoise_variance %dx%d: max relative error %.3g over %d compared pixels, %d left out" % (w, h, worst, compared, left_out))
    assert left_out <= 0.01 * (compared + left_out) and compared >= 24 * hit.sum() > 0
    if max(w, h) == 300:  # steps 32, 64 and 128 have taps inside the frame here
        for albedo in (False, True):
            for sl in pe.FILTER_SIGMAS:
                assert not _same_bits(results[(8, albedo, sl)], results[(5, albedo, sl)]), (albedo, sl, "levels 6 to 8 changed nothing")
    pt.close()
    del keep


# ---- g. the apron at the seams ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", pe.SEAM_MAPS)
@pytest.mark.parametrize("w,h", pe.SEAM_SHAPES)
def test_apron_at_the_seams(srt, w, h, kind):
    acc, var, obj, nd, pos, alb = pe.seam_inputs(w, h, kind)
    hit = obj >= 0
    pt = srt.PathTracer(w, h)
    keep = tv._bind(pt, obj, nd, pos, alb)
    keep["variance"] = tv._cuda(var)
    pt.bind_variance(keep["variance"])
    pt.write_accumulator(acc)
    worst, compared, left_out, by_level = 0.0, 0, 0, {}
    for levels in (1, 3):
        for albedo in (False, True):
            pt.denoise_variance(iterations=levels, sigma_luminance=4.0, sigma_normal=32.0, sigma_plane=0.02, albedo=albedo, gbuffer=False)
            got = pt.denoised()
            ref = vr.denoise_variance(acc, var, obj, nd, pos, alb, levels, 4.0, 32.0, 0.02, albedo)
            chk = hit & np.isfinite(ref[..., :3]).all(-1)
            left_out += int((hit & ~chk).sum())
            compared += int(chk.sum())
            err = _rel(got, ref)
            worst = max(worst, float(err[chk].max()))
            by_level[levels] = max(by_level.get(levels, 0.0), float(err[chk].max()))
            assert err[chk].max() <= dn.REL_TOL, (w, h, kind, levels, albedo, float(err[chk].max()), np.argwhere(chk & (err > dn.REL_TOL))[:8].tolist())
            assert _same_bits(got[~hit], acc[~hit]) and _same_bits(got[..., 3], acc[..., 3])
    _error_lines("test_apron_at_the_seams", "seams: " + kind, w, h, by_level)
    print("pass_edges seams %dx%d %s: max relative error %.3g over %d compared pixels, %d left out" % (w, h, kind, worst, compared, left_out))
    assert left_out <= 0.01 * (compared + left_out) and compared >= 4 * hit.sum() > 0.5 * w * h
    # isolation: NaN variance and colour on every pixel of every second object (across each seam) reach no pixel of the others
    params = dict(iterations=3, sigma_luminance=4.0, sigma_normal=32.0, sigma_plane=0.02, albedo=False, gbuffer=False)
    pt.denoise_variance(**params)
    base = pt.denoised()
    poisoned = hit & (obj % 2 == 1)
    clean = hit & ~poisoned
    assert poisoned.sum() > 20 and clean.sum() > 20
    bad_c, bad_v = acc.copy(), var.copy()
    bad_c[poisoned] = np.nan
    bad_v[poisoned] = np.nan
    pt.write_accumulator(bad_c)
    keep["bad"] = tv._cuda(bad_v)
    pt.bind_variance(keep["bad"])
    pt.denoise_variance(**params)
    got = pt.denoised()
    assert _same_bits(got[~poisoned], base[~poisoned]), "NaN on one object reached %d pixels of another" % int(
        (_bits(got) != _bits(base)).any(-1)[~poisoned].sum())
    pt.close()
    del keep


# ---- h. variance and sigma_luminance extremes -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,var", pe.extreme_variances(), ids=[n for n, _ in pe.extreme_variances()])
def test_variance_and_sigma_luminance_extremes(srt, name, var):
    w, h = pe.EXT_W, pe.EXT_H
    acc, obj, nd, pos, alb = pe.extreme_inputs()
    hit = obj >= 0
    pt = srt.PathTracer(w, h)
    keep = tv._bind(pt, obj, nd, pos, alb)
    keep["variance"] = tv._cuda(var)
    pt.bind_variance(keep["variance"])
    pt.write_accumulator(acc)
    worst, compared, by_level = 0.0, 0, {}
    for levels in pe.EXT_LEVELS:
        kw = dict(iterations=levels, sigma_normal=0.0, sigma_plane=0.0, albedo=False, gbuffer=False)
        pt.denoise_variance(sigma_luminance=0.0, **kw)
        off = pt.denoised()
        assert not _same_bits(off[hit], acc[hit])
        for sl in pe.EXT_SIGMAS:
            case = (name, levels, sl)
            pt.denoise_variance(sigma_luminance=sl, **kw)
            got = pt.denoised()
            assert np.isfinite(got[hit]).all(), (case, "a non-finite result on %d hit pixels" % int((~np.isfinite(got[hit])).any(-1).sum()))
            assert _same_bits(got[~hit], acc[~hit]) and _same_bits(got[..., 3], acc[..., 3]), case
            # what the header fixes: a zero variance closes the stop at every sigma; a scale that underflows opens it
            closed = hit & (var == 0)
            opened = hit & np.vectorize(pe.variance_opens)(var, sl)
            assert _rel(got, acc)[closed].max(initial=0.0) <= dn.REL_TOL, (case, "a zero variance did not close the stop")
            assert _rel(got, off)[opened].max(initial=0.0) <= dn.REL_TOL, (case, "an underflowing scale did not open the stop")
            ref = vr.denoise_variance(acc, var, obj, nd, pos, alb, levels, sl, 0.0, 0.0, False)
            assert np.isfinite(ref[hit]).all(), (case, "the definition is not finite")
            err = float(_rel(got, ref)[hit].max())
            worst = max(worst, err)
            by_level[levels] = max(by_level.get(levels, 0.0), err)
            compared += int(hit.sum())
            assert err <= dn.REL_TOL, (case, err)
    _error_lines("test_variance_and_sigma_luminance_extremes", "extremes: variance " + name, w, h, by_level)
    print("pass_edges extremes %s: max relative error %.3g over %d compared pixels" % (name, worst, compared))
    assert compared == len(pe.EXT_LEVELS) * len(pe.EXT_SIGMAS) * hit.sum() > 5000
    pt.close()
    del keep


# ---- i. moving objects ------------------------------------------------------------------------------------------------------
def _check_motion_frame(pt, srt, mv_on, acc, guides, hist, delta, keep, params, what):
    """One srt_temporal_accumulate against motion_reference with the bounds of test_moved_objects_match_the_definition.
    Returns (got, L, motion or None, dict of counts and masks)."""
    obj, nd, pos = guides
    n, max_samples, sigma_t, thr = params
    pt.write_accumulator(acc)
    pt.temporal(samples=n, max_samples=max_samples, plane_tolerance=sigma_t, normal_threshold=thr, gbuffer=False)
    got, L = pt.accumulator(), pt.history_length()
    with np.errstate(all="ignore"):
        ref, refL, sens, scale, sw, _, rmv, mv_ok = mo.motion_reference(acc, obj, nd, pos, hist, delta, keep, n, max_samples, sigma_t, thr)
    hit = obj >= 0
    assert _same_bits(got[~hit], acc[~hit]) and np.all(L[~hit] == 0), what
    assert _same_bits(got[..., 3], acc[..., 3]), (what, "alpha was written")
    chk = hit & ~sens
    err = np.max(np.abs(got[..., :3].astype(np.float64) - ref), axis=2)
    bad = chk & ~(err <= mo.REL_TOL * scale)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:8].tolist())
    assert np.all(np.abs(L[chk] - refL[chk]) <= mo.REL_TOL * refL[chk]), what
    kept = chk & (sw == 0)
    assert _same_bits(got[kept], acc[kept]) and np.all(L[kept] == n), what
    mv = None
    worst = 0.0
    if mv_on:
        mv = pt.motion()
        assert not mv[~hit].any() and not mv[..., 3].any(), what
        e = np.max(np.abs(mv[..., :2].astype(np.float64) - rmv), axis=2)
        worst = float(e[chk].max(initial=0.0))
        assert worst <= mo.MV_TOL, (what, worst)
        assert np.all(np.abs(mv[..., 2] - sw)[chk] <= mo.WSUM_TOL), what
        assert not mv[chk & ~mv_ok][:, :3].any(), (what, "a pixel without previous coordinates has a motion vector")
        if hist is None:
            assert not mv.any(), what
    return got, L, mv, dict(hit=hit, chk=chk, sw=sw, sens=sens, mv_ok=mv_ok, rmv=rmv, worst_mv=worst)


def _set(pt, srt, oracle, spheres, update):
    oarr, cnt = mo._objects(oracle, spheres)
    (pt.update_scene if update else pt.set_scene)(C.cast(oarr, C.POINTER(srt.Object)), cnt)
    return cnt


@pytest.mark.parametrize("mv_on", [True, False])
def test_moving_objects_at_every_shape(srt, oracle, mv_on):
    hits = checked = blended = moved_blended = 0
    worst_mv = 0.0
    for w, h in SHAPES:
        for params in pe.MOTION_PARAMS:
            pt = srt.PathTracer(w, h)
            pt.motion_output(mv_on)
            hist = prev = keepalive = None
            for k, (lists, spheres, cam, guides, acc) in enumerate(pe.motion_sequence(srt, w, h, seed=w + 7 * h)):
                if k == 0:
                    _set(pt, srt, oracle, spheres, update=False)
                for s in lists:
                    _set(pt, srt, oracle, s, update=True)
                keepalive = tp._bind(pt, guides)
                pt.set_camera(cam)
                delta, keep = pe.sphere_table(prev if prev is not None else spheres, spheres)
                got, L, mv, r = _check_motion_frame(pt, srt, mv_on, acc, guides, hist, delta, keep, params, (w, h, k, params))
                obj = guides[0]
                hits += int(r["hit"].sum())
                checked += int(r["chk"].sum())
                blended += int((r["chk"] & (r["sw"] > 0)).sum())
                moved_blended += int((r["chk"] & (r["sw"] > 0) & (obj > 0)).sum())
                worst_mv = max(worst_mv, r["worst_mv"])
                if not mv_on:
                    with pytest.raises(srt.SrtError) as ex:
                        pt.motion()
                    assert ex.value.code == srt.capi.ERR_STATE
                hist = dict(cam=cam, color=got, L=L, obj=obj, nd=guides[1], pos=guides[2])
                prev = spheres
            pt.close()
            del keepalive
    print("pass_edges moving objects (motion output %d): %d hit, %d checked, %d blended (%d on moved objects), worst motion error %.3g px"
          % (mv_on, hits, checked, blended, moved_blended, worst_mv))
    assert hits - checked <= 0.01 * hits, "the definition leaves more than 1 % of the hit pixels undecided"
    assert checked > 4000 and blended > 0.3 * checked and moved_blended > 100


def _left_out(r, also_checked=None):
    """(hit pixels the definition leaves undecided, hit pixels) of one frame; `also_checked`: pixels the test holds to the header
    directly although the definition's mask leaves them out."""
    out = r["hit"] & r["sens"]
    if also_checked is not None:
        out &= ~also_checked
    return int(out.sum()), int(r["hit"].sum())


def test_object_indices_beyond_the_motion_table(srt, oracle):
    """A bound OBJECT guide with the indices count, count + 5 and 2^30 on ground pixels (labelled by where their point lies, so
    that a point keeps its label from frame to frame) while the spheres move, so that the table is in play: those pixels
    behave as delta = 0, keep = 1 and blend with their history."""
    w, h, params = pe.EDGE_W, pe.EDGE_H, pe.EDGE_PARAMS
    for mv_on in (True, False):
        pt = srt.PathTracer(w, h)
        pt.motion_output(mv_on)
        hist = prev = keepalive = None
        left = hits = blended_beyond = checked_beyond = 0
        for k, (lists, spheres, cam, (obj, nd, pos), acc) in enumerate(pe.motion_sequence(srt, w, h, seed=23, frames=pe.EDGE_FRAMES)):
            if k == 0:
                cnt = _set(pt, srt, oracle, spheres, update=False)
            for s in lists:
                _set(pt, srt, oracle, s, update=True)
            obj = pe.relabel_beyond(obj, pos, cnt)
            beyond = obj >= cnt
            assert beyond.sum() > 200 and all((obj == i).sum() > 30 for i in (cnt, cnt + 5, 2 ** 30))
            keepalive = tp._bind(pt, (obj, nd, pos))
            pt.set_camera(cam)
            delta, keep = pe.sphere_table(prev if prev is not None else spheres, spheres)
            got, L, mv, r = _check_motion_frame(pt, srt, mv_on, acc, (obj, nd, pos), hist, delta, keep, params, (mv_on, k))
            if k:
                assert np.any(delta != 0)
                lo, n_hit = _left_out(r)
                left, hits = left + lo, hits + n_hit
                checked_beyond += int((r["chk"] & beyond).sum())
                blended_beyond += int((r["chk"] & beyond & (L > 1)).sum())
                if mv_on:
                    assert np.all(mv[r["chk"] & beyond & (L > 1)][:, 2] > 0)
            hist = dict(cam=cam, color=got, L=L, obj=obj, nd=nd, pos=pos)
            prev = spheres
        pt.close()
        del keepalive
        print("pass_edges beyond the table (motion output %d): %d hit, %d left out, %d of %d pixels beyond the table kept their history"
              % (mv_on, hits, left, blended_beyond, checked_beyond))
        assert left <= 0.01 * hits
        assert blended_beyond > 0.8 * checked_beyond > 300, "pixels whose object lies beyond the table lost their history"


@pytest.mark.parametrize("step", pe.DISPLACEMENTS, ids=["zero", "1e-30", "1e30", "inf"])
def test_displacement_extremes(srt, oracle, step):
    """The list position of the first sphere (object 1, whose y is 0) changes by `step` between two frames while the bound guides
    stay where they are.  -0 for +0 is no displacement: the plain kernel, bit for bit.  1e-30 vanishes in x - delta: the table
    kernel gives the plain kernel's bits.  1e30 and inf throw the history point far outside the window: the object's pixels
    have motion (0, 0) and no history."""
    params = pe.EDGE_PARAMS
    w, h = pe.EDGE_W, pe.EDGE_H
    cams, guides, accs, moved = pe.displacement_frames(srt, step)
    own = guides[1][0] == 1
    runs = {}
    for how in ("plain", "update"):
        pt = srt.PathTracer(w, h)
        pt.motion_output(True)
        _set(pt, srt, oracle, mo.BASE, update=False)
        zero = (np.zeros((4, 3), np.float32), np.ones(4, bool))
        keepalive = tp._bind(pt, guides[0])
        pt.set_camera(cams[0])
        got, L, mv, _ = _check_motion_frame(pt, srt, True, accs[0], guides[0], None, *zero, params, (how, 0))
        hist = dict(cam=cams[0], color=got, L=L, obj=guides[0][0], nd=guides[0][1], pos=guides[0][2])
        table = zero
        if how == "update":
            _set(pt, srt, oracle, moved, update=True)
            table = pe.sphere_table(mo.BASE, moved)
            assert not np.isnan(table[0]).any() and (step == 0.0) == (not np.any(table[0] != 0))
        keepalive = tp._bind(pt, guides[1])
        pt.set_camera(cams[1])
        runs[how] = _check_motion_frame(pt, srt, True, accs[1], guides[1], hist, *table, params, (how, 1))
        pt.close()
        del keepalive
    (g0, L0, m0, r0), (g1, L1, m1, r1) = runs["plain"], runs["update"]
    assert own.sum() > 40 and (L0[own] == 2).mean() > 0.8
    assert _same_bits(g0[~own], g1[~own]) and _same_bits(L0[~own], L1[~own]) and _same_bits(m0[~own], m1[~own])
    if step < 1.0:
        assert _same_bits(g0, g1) and _same_bits(L0, L1) and _same_bits(m0, m1)
        left, hits = _left_out(r1)
    else:
        # whether g is positive is within rounding of the huge x~, so the definition's mask leaves the object's pixels out;
        # what the header fixes either way is checked on every one of them here
        assert _same_bits(g1[own], accs[1][own]) and np.all(L1[own] == 1) and not m1[own].any()
        left, hits = _left_out(r1, also_checked=own)
    print("pass_edges displacement %g: %d hit, %d left out" % (step, hits, left))
    assert left <= 0.01 * hits and hits > 400


@pytest.mark.parametrize("params", pe.TEMPORAL_EXTREMES, ids=["n%d-max%g-t%g-thr%g" % p for p in pe.TEMPORAL_EXTREMES])
@pytest.mark.parametrize("mv_on", [True, False])
def test_moving_objects_parameter_extremes(srt, oracle, mv_on, params):
    w, h = pe.EDGE_W, pe.EDGE_H
    pt = srt.PathTracer(w, h)
    pt.motion_output(mv_on)
    hist = prev = keepalive = None
    hits = left = checked = blended = ground_blended = 0
    for k, (lists, spheres, cam, guides, acc) in enumerate(pe.motion_sequence(srt, w, h, seed=23, frames=pe.EDGE_FRAMES)):
        if k == 0:
            _set(pt, srt, oracle, spheres, update=False)
        for s in lists:
            _set(pt, srt, oracle, s, update=True)
        keepalive = tp._bind(pt, guides)
        pt.set_camera(cam)
        delta, keep = pe.sphere_table(prev if prev is not None else spheres, spheres)
        got, L, mv, r = _check_motion_frame(pt, srt, mv_on, acc, guides, hist, delta, keep, params, (k, params))
        if k:
            lo, n_hit = _left_out(r)
            left, hits = left + lo, hits + n_hit
            checked += int(r["chk"].sum())
            blended += int((r["chk"] & (r["sw"] > 0)).sum())
            ground_blended += int((r["chk"] & (r["sw"] > 0) & (guides[0] == 0)).sum())
        hist = dict(cam=cam, color=got, L=L, obj=guides[0], nd=guides[1], pos=guides[2])
        prev = spheres
    pt.close()
    del keepalive
    n, max_samples, sigma_t, thr = params
    print("pass_edges moving objects %r: %d hit, %d left out, %d blended (%d on the ground)" % (params, hits, left, blended, ground_blended))
    assert left <= 0.01 * hits and hits > 800
    if sigma_t < 1e-30 or thr >= 1.0:
        # only exact ties count, and only the ground has them: its normals are exactly (0, 1, 0) and its points share y = -1
        # bit for bit, so n.(x'_q - x~_p) == 0 and n.n'_q == 1 in binary32 and in float64, wherever the camera stands
        assert ground_blended > 500 and blended == ground_blended
    else:
        assert blended > 0.9 * checked
    if max_samples == INF:
        assert float(L.max()) > 2 * n
