"""tests/probe_update_reference.py on hand-made records and buffers: the list's layout, and rules U1 - U5 of the blend — a restart by
a zero history, by an offset change, by a BURIED flip and by an IDLE flip, changed and unchanged probes, h = 0 gives N, H == N stays
N, unlisted probes keep their bits.  No GPU."""
import numpy as np

import probe_update_reference as PU

F, U = np.float32, np.uint32


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(U)


def test_the_list_is_ascending_behind_its_header_and_padded():
    st = np.array([0, PU.BURIED | PU.INSIDE, PU.MOVED, PU.IDLE, PU.MOVED | PU.INSIDE, 0, PU.BURIED | PU.INSIDE], U)
    rec = PU.records_of(st)
    w = PU.probe_list(rec)
    assert w.dtype == U and w.tolist() == [4, 7, 0, 0, 0, 2, 4, 5, PU.NONE, PU.NONE, PU.NONE]
    assert PU.probe_list(rec, 0).tolist() == [7, 7, 0, 0, 0, 1, 2, 3, 4, 5, 6]
    assert PU.probe_list(rec, PU.STATE_BITS).tolist() == [2, 7, 0, 0, 0, 5] + [PU.NONE] * 5
    assert PU.probe_list(rec, PU.INSIDE).tolist() == [4, 7, 0, 0, 0, 2, 3, 5] + [PU.NONE] * 3
    assert PU.probe_list(PU.records_of([PU.BURIED])).tolist() == [0, 1, 0, 0, PU.NONE]
    assert PU.listed(w).tolist() == [0, 2, 4, 5]
    bad = w.copy()
    bad[5] = 7  # an index >= P is skipped; a count beyond P is clamped
    bad[0] = 99
    assert PU.listed(bad).tolist() == [0, 4, 5]


def _buffers(P=8, R2=16, seed=1):
    rng = np.random.default_rng(seed)
    H = rng.uniform(0.1, 2.0, (P, 9, 4)).astype(F)
    N = rng.uniform(0.1, 2.0, (P, 9, 4)).astype(F)
    DH = rng.uniform(0.1, 5.0, (P, R2, 4)).astype(F)
    DN = rng.uniform(0.1, 5.0, (P, R2, 4)).astype(F)
    return H, N, DH, DN


def test_restarts_by_zero_history_offset_change_and_buried_or_idle_flip():
    H, N, DH, DN = _buffers()
    H[1, 0, 3] = 0.0  # the reset history: the bits of H[p][0].w are 0
    cur = PU.records_of([0, 0, PU.MOVED, 0, PU.IDLE, PU.MOVED | PU.INSIDE, 0, PU.BURIED | PU.INSIDE],
                        [(0, 0, 0), (0, 0, 0), (0.1, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0.2, 0), (0, 0, 0), (0, 0, 0)])
    prev = cur.copy()
    prev[2, 0] = F(0.1000001)                        # an offset lane differs bitwise
    prev[3, 3] = U(PU.BURIED | PU.INSIDE).view(F)   # BURIED flip
    prev[4, 3] = U(0).view(F)                        # IDLE flip
    prev[5, 3] = U(PU.MOVED).view(F)                 # INSIDE alone is not looked at
    prev[6, 2] = F(-0.0)                             # +0 against -0: bitwise different
    r = PU.blend(H, N, DH, DN, states=cur, previous=prev, hysteresis=F(0.9), fast_hysteresis=F(0.5), change_threshold=F(100.0))  # (nothing counts as changed)
    assert r["restart"].tolist() == [False, True, True, True, True, False, True, False]
    for p in (1, 2, 3, 4, 6):
        assert np.array_equal(bits(r["history"][p]), bits(N[p])) and np.array_equal(bits(r["depth_history"][p]), bits(DN[p]))
    for p in (0, 5, 7):
        assert np.array_equal(bits(r["history"][p]), bits(N[p] + (H[p] - N[p]) * F(0.9)))
        assert np.array_equal(bits(r["depth_history"][p]), bits(DN[p] + (DH[p] - DN[p]) * F(0.9)))
    assert r["work"] == dict(probes=8, restarted=5, changed=0)
    # without PREVIOUS_STATES only the zero history restarts
    r = PU.blend(H, N)
    assert r["restart"].tolist() == [False, True] + [False] * 6 and r["depth_history"] is None


def test_changed_probes_take_the_fast_hysteresis():
    H, N, _, _ = _buffers(P=4)
    H[:, 0, :3] = (1.0, 1.0, 1.0)
    N[0, 0, :3] = (1.2, 1.2, 1.2)    # d = 0.2, m = 1.2: 0.2 > 0.25 * 1.2 = 0.3 is false
    N[1, 0, :3] = (1.5, 1.5, 1.5)    # d = 0.5, m = 1.5: 0.5 > 0.375
    N[2, 0, :3] = (0.5, 0.5, 0.5)    # d = 0.5, m = 1: changed
    N[3, 0, :3] = (1.0, 1.0, 1.0)    # d = 0: not changed, even with threshold 0
    r = PU.blend(H, N, hysteresis=F(0.9), fast_hysteresis=F(0.5), change_threshold=F(0.25))
    assert r["changed"].tolist() == [False, True, True, False] and r["work"] == dict(probes=4, restarted=0, changed=2)
    for p, h in ((0, 0.9), (1, 0.5), (2, 0.5), (3, 0.9)):
        assert np.array_equal(bits(r["history"][p]), bits(N[p] + (H[p] - N[p]) * F(h))), p
    assert PU.blend(H, N, change_threshold=F(0.0))["changed"].tolist() == [True, True, True, False]
    y = PU.luminance(np.array([0.5, 0.25, 2.0], F))
    assert y.dtype == F and y == (F(0.2126) * F(0.5) + F(0.7152) * F(0.25)) + F(0.0722) * F(2.0)


def test_h_zero_gives_the_new_data_and_equal_data_stay():
    H, N, DH, DN = _buffers()
    r = PU.blend(H, N, DH, DN, hysteresis=F(0.0), fast_hysteresis=F(0.0), depth_hysteresis=F(0.0))
    assert np.array_equal(r["history"], N) and np.array_equal(r["depth_history"], DN) and not r["restart"].any()
    r = PU.blend(N, N, DN, DN)
    assert np.array_equal(r["history"], N) and np.array_equal(r["depth_history"], DN) and not r["changed"].any()


def test_a_listed_blend_leaves_the_other_probes_alone():
    H, N, DH, DN = _buffers()
    words = PU.probe_list(PU.records_of([0, PU.BURIED, 0, PU.IDLE, 0, 0, PU.BURIED, 0]))
    r = PU.blend(H, N, DH, DN, words=words)
    for p in (1, 3, 6):
        assert np.array_equal(bits(r["history"][p]), bits(H[p])) and np.array_equal(bits(r["depth_history"][p]), bits(DH[p]))
    full = PU.blend(H, N, DH, DN)
    for p in (0, 2, 4, 5, 7):
        assert np.array_equal(bits(r["history"][p]), bits(full["history"][p])) and np.array_equal(bits(r["depth_history"][p]), bits(full["depth_history"][p]))
    assert r["work"]["probes"] == 5 and full["work"]["probes"] == 8
    shuffled = words.copy()
    shuffled[4:9] = words[4:9][::-1]
    assert np.array_equal(bits(PU.blend(H, N, DH, DN, words=shuffled)["history"]), bits(r["history"]))
    empty = words.copy()
    empty[0] = 0
    assert np.array_equal(bits(PU.blend(H, N, words=empty)["history"]), bits(H))
