"""Properties of the mirror history's float64 definition alone (tests/mirror_history_reference.py): on the flat-mirror guides the
virtual point lands on the pixel of the previous frame that sees the same terminal point, a frame without mirrors reduces to
tests/moments_reference.py exactly, and the tags round-trip.  No compute: runs without a GPU."""
import math

import numpy as np

import mirror_history_reference as mh
import moments_reference as mr

SYNTH_MOVES, camera = mh.SYNTH_MOVES, mh.camera


def test_the_generator_shows_every_kind_of_pixel(srt):
    w, h = 37, 21
    g = mh.flat_mirror_guides(camera(srt, (0.0, 0.0, 0.0)), w, h)
    J, obj, ro = g["bounces"], g["obj"], g["r_obj"]
    assert (obj < 0).any() and (obj == mh.PATCH).any() and ((J == 1) & (ro < 0)).any()
    assert all(((J == 1) & (ro == mh.WALL0 + k)).any() for k in range(3))
    assert np.all(J[obj != mh.MIRROR] == 0) and np.all(J[obj == mh.MIRROR] == 1)
    plain = J == 0  # the identity of the reflection pass
    assert np.array_equal(ro[plain], obj[plain]) and np.array_equal(g["r_nd"][plain], g["nd"][plain]) and np.array_equal(g["r_pos"][plain], g["pos"][plain])
    # the path length is the distance to the mirror image of the terminal point
    m = (J == 1) & (ro >= 0)
    image = g["r_pos"][..., :3].astype(np.float64) * [1, 1, -1] + [0, 0, 10]
    assert np.allclose(np.linalg.norm(image[m], axis=1), g["r_nd"][..., 3][m], rtol=1e-6)


def test_candidate_one_lands_where_the_previous_frame_saw_the_same_point(srt):
    w, h = 37, 21
    cams = [camera(srt, (dx, dy, 0.0)) for dx, dy in SYNTH_MOVES] + [camera(srt, (0.2, -0.1, 0.3), 4.0), camera(srt, (-0.3, 0.2, -0.4), -6.0)]
    checked = 0
    for prev, cur in zip(cams[:-1], cams[1:]):
        g = mh.flat_mirror_guides(cur, w, h, dtype=np.float64)
        m = (g["bounces"] == 1) & (g["r_obj"] >= 0)
        Cc = np.array(cur.position[:], np.float64)
        x0 = g["pos"][..., :3]
        with np.errstate(all="ignore"):
            y = Cc + (x0 - Cc) * (g["r_nd"][..., 3] / g["nd"][..., 3])[..., None]
        u, v, ok, _ = mh.project(y, prev, w, h, exact=True)
        sel = m & ok & (u >= 0) & (u <= w - 1) & (v >= 0) & (v <= h - 1)
        assert sel.sum() > 0.2 * m.sum()
        # what the previous camera sees at exactly (u, v): the same terminal point, through the mirror, on the same object
        seen = mh.flat_mirror_guides(prev, w, h, xs=np.where(sel, u, 0.0), ys=np.where(sel, v, 0.0), dtype=np.float64)
        # (the patch and the miss bands lie on the mirror, at another depth than the image: where the previous ray meets one of
        # them the image was hidden, a disocclusion)
        sel = sel & (seen["bounces"] == 1)
        assert sel.sum() > 0.15 * m.sum()
        # |delta| in pixels: the terminal point's offset over the size of a pixel at the path length
        px = 2 * math.tan(math.radians(55) / 2) / h * g["r_nd"][..., 3]
        delta = np.linalg.norm(seen["r_pos"][..., :3] - g["r_pos"][..., :3], axis=-1) / px
        assert np.max(delta[sel]) < 1e-6, float(np.max(delta[sel]))
        assert np.array_equal(seen["r_obj"][sel], g["r_obj"][sel])
        checked += int(sel.sum())
    assert checked > 500


def test_without_mirrors_it_is_the_moments_reference_exactly(srt):
    w, h = 37, 21
    n, max_samples, sigma_t, thr = 2, 5.0, 0.02, 0.9
    rng = np.random.default_rng(3)
    prev = mom = None
    for k, (dx, dy) in enumerate(SYNTH_MOVES):
        cam = camera(srt, (dx, dy, 0.0))
        g = mh.without_mirrors(mh.flat_mirror_guides(cam, w, h))
        acc = rng.uniform(0.02, 3.0, (h, w, 3))
        res = mh.accumulate(acc, g, prev, n, max_samples, sigma_t, thr)
        assert np.all(res["store"]["tag"] == 0) and np.all(res["candidate"] == 0)
        mu = mr.frame_luminance(acc)
        want_taps = None
        if prev is not None:
            want_taps, edge = mr.taps(g["obj"], g["nd"], g["pos"], dict(cam=prev["cam"], obj=prev["obj"], nd=prev["nrm"], pos=prev["pos"]), sigma_t, thr)
            for (a, ay, ax), (b, by, bx) in zip(res["taps"], want_taps):
                assert np.array_equal(a, b) and np.array_equal(ay, by) and np.array_equal(ax, bx)
            assert np.array_equal(res["edge"][g["obj"] >= 0], edge[g["obj"] >= 0])
            assert (res["L"] > n).any()
        got = mr.blend(mu, g["obj"], res["taps"], mom, n, max_samples)
        assert np.array_equal(got, mr.blend(mu, g["obj"], want_taps, mom, n, max_samples))
        # the colour blend is the moments blend's rule: a grey image's history length is the moments' length
        assert np.array_equal(res["L"], got[..., 2])
        prev, mom = res["store"], got
    # ... and the stored guides are the first hits
    assert np.array_equal(prev["obj"], g["obj"]) and np.array_equal(prev["pos"][..., :3], np.where((g["obj"] >= 0)[..., None], g["pos"][..., :3], 0))


def test_tag_packing_round_trips():
    J, m = np.meshgrid(np.arange(1, 65), np.arange(0, 32767), indexing="ij")
    t = mh.tag(J, m)
    assert t.min() > 0 and t.max() < 2 ** 31 and np.unique(t).size == t.size
    j2, m2 = mh.untag(t)
    assert np.array_equal(j2, J) and np.array_equal(m2, m)
    assert np.all(mh.tag(np.zeros(5, int), np.arange(5)) == 0)


def test_rho_is_the_angle_of_the_radius(srt):
    assert mh.rho(2.0, 55.0, 21) == float(np.float32(2.0 * 2.0 * math.tan(55.0 * math.pi / 360.0) / 21))
    assert mh.rho(float("inf"), 55.0, 21) == float("inf")
