"""numpy float32 reference of the per-frame probe updates (include/srt_pathtrace.h, the block "per-frame probe updates"): the list of
active probes (srt_list_probes) and rules U1 - U5 and U7 of the hysteresis blend (srt_blend_probes).  Every operation is a single
binary32 operation on binary32 operands, in the header's order, so the GPU tests compare bit for bit."""
import numpy as np

F = np.float32
U = np.uint32

MOVED, BURIED, INSIDE, IDLE = 1, 2, 4, 8
STATE_BITS = MOVED | BURIED | INSIDE | IDLE
HEADER = 4
NONE = 0xFFFFFFFF
LIST_COUNT_WORK = 1
HISTORY_COEFFICIENTS, HISTORY_MOMENTS = 1, 2
BLEND_MOMENTS, BLEND_LISTED, BLEND_PREVIOUS_STATES, BLEND_COUNT_WORK = 1, 2, 4, 8
DEFAULT_SKIP = BURIED | IDLE
DEFAULTS = dict(hysteresis=F(0.9), fast_hysteresis=F(0.5), depth_hysteresis=F(0.9), change_threshold=F(0.25))
COEFFS = 9


def state_bits(records):
    """The uint32 state of every (P, 4) float32 record."""
    return np.ascontiguousarray(records, dtype=F).reshape(-1, 4)[:, 3].copy().view(U)


def records_of(states, offsets=None):
    """(P, 4) float32 records with the given uint32 states in w and the offsets (default 0) in xyz."""
    st = np.asarray(states, dtype=U)
    rec = np.zeros((st.shape[0], 4), F)
    if offsets is not None:
        rec[:, :3] = np.asarray(offsets, dtype=F)
    rec[:, 3] = st.view(F)
    return rec


def probe_list(records, skip_mask=DEFAULT_SKIP):
    """SRT_PROBE_LIST of the records: n, P, 0, 0, the indices with (state & skip_mask) == 0 ascending, then 0xFFFFFFFF."""
    st = state_bits(records)
    P = st.shape[0]
    idx = np.flatnonzero((st & U(skip_mask)) == 0).astype(U)
    out = np.full(HEADER + P, NONE, U)
    out[0], out[1], out[2], out[3] = idx.shape[0], P, 0, 0
    out[HEADER:HEADER + idx.shape[0]] = idx
    return out


def listed(words, probes=None):
    """The probe indices a kernel takes from a list: the first min(n, P) words behind the header, those >= P skipped."""
    w = np.asarray(words, dtype=U)
    P = int(probes) if probes is not None else w.shape[0] - HEADER
    n = min(int(w[0]), P)
    idx = w[HEADER:HEADER + n]
    return idx[idx < P].astype(np.int64)


def luminance(v):
    v = np.asarray(v, dtype=F)
    return (F(0.2126) * v[..., 0] + F(0.7152) * v[..., 1]) + F(0.0722) * v[..., 2]


def mix(H, N, h):
    """Rule U4: H = N + ((H - N) * h), element by element; h broadcasts over the probe axis."""
    H, N = np.asarray(H, dtype=F), np.asarray(N, dtype=F)
    h = np.asarray(h, dtype=F).reshape((-1,) + (1,) * (H.ndim - 1))
    with np.errstate(invalid="ignore", over="ignore"):
        return (N + ((H - N) * h)).astype(F)


def blend(history, fresh, depth_history=None, depth_fresh=None, words=None, states=None, previous=None, hysteresis=DEFAULTS["hysteresis"],
          fast_hysteresis=DEFAULTS["fast_hysteresis"], depth_hysteresis=DEFAULTS["depth_hysteresis"], change_threshold=DEFAULTS["change_threshold"]):
    """srt_blend_probes on numpy arrays: history / fresh (P, 9, 4); depth_* (P, R*R, 4) or None (no _MOMENTS); words: a list (with
    _LISTED) or None; states / previous: (P, 4) records (with _PREVIOUS_STATES) or None.  Returns a dict: history, depth_history
    (new arrays), restart, changed (bool per probe, False where the probe was not blended), work."""
    H = np.array(history, dtype=F).reshape(-1, COEFFS, 4)
    N = np.asarray(fresh, dtype=F).reshape(-1, COEFFS, 4)
    P = H.shape[0]
    assert N.shape == H.shape
    idx = listed(words, P) if words is not None else np.arange(P, dtype=np.int64)  # U1
    h0, n0 = H[idx, 0], N[idx, 0]
    restart = h0[:, 3].copy().view(U) == 0  # U2
    if previous is not None:
        a = np.ascontiguousarray(states, dtype=F).reshape(P, 4)[idx].view(U)
        b = np.ascontiguousarray(previous, dtype=F).reshape(P, 4)[idx].view(U)
        restart = restart | (a[:, :3] != b[:, :3]).any(axis=1) | (((a[:, 3] ^ b[:, 3]) & U(BURIED | IDLE)) != 0)
    with np.errstate(invalid="ignore", over="ignore"):
        yh, yn = luminance(h0), luminance(n0)  # U3
        d = np.abs((yn - yh).astype(F))
        ah, an = np.abs(yh), np.abs(yn)
        m = np.where(ah > an, ah, an).astype(F)
        changed = d > (F(change_threshold) * m).astype(F)
    h = np.where(changed, F(fast_hysteresis), F(hysteresis)).astype(F)
    out = mix(H[idx], N[idx], h)  # U4
    out[restart] = N[idx][restart]
    H[idx] = out  # (a duplicate index gets the same bits each time)
    DH = None
    if depth_history is not None:  # U5
        DH = np.array(depth_history, dtype=F)
        DH = DH.reshape(P, -1, 4)
        DN = np.asarray(depth_fresh, dtype=F).reshape(DH.shape)
        dout = mix(DH[idx], DN[idx], np.full(idx.shape[0], F(depth_hysteresis)))
        dout[restart] = DN[idx][restart]
        DH[idx] = dout
    full_restart, full_changed = np.zeros(P, bool), np.zeros(P, bool)
    full_restart[idx], full_changed[idx] = restart, changed & ~restart
    work = dict(probes=int(idx.shape[0]), restarted=int(restart.sum()), changed=int((changed & ~restart).sum()))
    return dict(history=H, depth_history=DH, restart=full_restart, changed=full_changed, work=work)
