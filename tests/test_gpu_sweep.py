"""Threshold sweep: ONE event stream under B adaptive gates in one launch (kf_run_sweep through
BatchedKF.run_sweep, kfmi.ref15.AdaptiveSweep and the façade) — needs an MI355X.

The margin rule.  One flipped gate changes every later record, so a threshold is compared only
where the reference itself is not on the fence: before any launch the smallest |logdet(P_pred) -
threshold| over the run is computed on the CPU with the NumPy oracle's matrices (a
covariance-only recursion: the gate never reads the state).  Flags and records are compared for
thresholds whose margin is >= 1e-5 in f64 (the device agrees with the oracle to ~1e-10) and >=
1e-2 in f32 (GateBand's f32 band is 1e-4); each test states how many thresholds the rule may
exclude, a condition on its inputs.
"""
import gzip
import os

import numpy as np
import pytest
import torch

import kfmi
from golden_events import unpack_events
from kfmi import _lib, ref15
from kfmi import kf_workers as kfw
from oracle import ref_kf

pytestmark = pytest.mark.gpu
TOL = 1e-6            # against the oracle (north_star, fp64), tests/test_gpu_ref15.py's normalisation
KERNELS = 1e-9        # between two kernels of the engine (test_gated_route_equals_single_filter)
MARGIN = {'f64': 1e-5, 'f32': 1e-2}
INF = float('inf')
GRID = [-40 + 0.65 * k for k in range(70)]
# stream 4's thresholds (margins >= 4e-5 there; -30 has 2.5e-7 and is not used)
STREAM4_THR = [-35.0, -32.5, -29.5, -27.5, -25.0, -20.0, -15.0, -10.0, -5.0, 0.0]
F32_THR = [-40.0, -36.75, -11.4, -6.85, 0.3, 2.9]


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0))) if a.size else 0.0


# ---------------------------------------------------------------------------------------------
# inputs (computed once, never modified)
# ---------------------------------------------------------------------------------------------
_cache = {}


def _once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _stream(T, seed=1, gps_every=20, keep=0.7, skips=0):
    """tests/test_gpu_timeparallel.py's stream: 200 Hz IMU, ~10 Hz GPS fixes (some missing);
    ``skips`` events are NONE (the driver's dt < 0 rule)."""
    rng = np.random.default_rng(seed)
    et = np.ones(T, np.uint8)
    gi = np.arange(0, T, gps_every)
    gi = gi[rng.random(len(gi)) < keep]
    et[gi] = ref15.GPS
    et[0] = ref15.GPS
    if skips:
        et[rng.choice(np.arange(1, T), skips, replace=False)] = ref15.NONE
    dt = np.full(T, 0.005)
    dt[0] = 0.0
    t = np.arange(T) * 0.005
    pos = np.stack([300 + 3.3 * t, -200 + 2.2 * t, 0.05 * np.cumsum(rng.normal(0, 0.1, T))], 1)
    pay = np.zeros((T, 9))
    g = et == 0
    pay[g, 0:3] = pos[g] + rng.normal(0, 1.5, (int(g.sum()), 3))
    i = ~g
    pay[i, 0] = rng.normal(0, 0.02, int(i.sum()))
    pay[i, 1] = rng.normal(-0.05, 0.01, int(i.sum()))
    pay[i, 2] = np.cumsum(rng.normal(0, 2e-4, T))[i]
    pay[i, 3:6] = rng.normal(0, 0.01, (int(i.sum()), 3))
    pay[i, 6:9] = rng.normal(0, 0.3, (int(i.sum()), 3))
    x0 = np.zeros(15)
    x0[0:3] = pay[0, 0:3]
    return et, dt, pay, x0


def _stream4():
    return _once('stream4', lambda: _stream(5000, seed=11, skips=300))


def _golden(golden_dir):
    def load():
        g = np.load(os.path.join(golden_dir, 'ref15_full.npz'))
        return g, unpack_events(g)
    return _once('golden', load)


def _list_arrays(events, start_idx=0, end_idx=None):
    """The adaptive driver's stream over an event list (kf_workers.py:990-1015): from the first
    fix of the window, a dt < 0 event skipped (NONE) without advancing the previous time.
    Returns et [T], dt [T], pay [T, 9], x0 [15]."""
    end_idx = len(events) if end_idx is None else end_idx
    s = next(i for i in range(start_idx, end_idx) if events[i][1] == 'GPS')
    x0 = np.zeros(15)
    x0[0:3] = [events[s][3][k] for k in ('easting', 'northing', 'altitude')]
    T = end_idx - s
    et, dt, pay = np.full(T, ref15.NONE, np.uint8), np.zeros(T), np.zeros((T, 9))
    prev = events[s][2]
    for j, (_, stype, t, sdata) in enumerate(events[s:end_idx]):
        if t - prev < 0:
            continue
        et[j] = ref15.GPS if stype == 'GPS' else ref15.IMU
        dt[j] = t - prev
        pay[j] = ref15.event_payload(stype, sdata)
        prev = t
    return et, dt, pay, x0


def _golden_arrays(golden_dir):
    return _once('golden_arrays', lambda: _list_arrays(_golden(golden_dir)[1]))


def _symmetric_consts(model, seed):
    """tests/test_gpu_timeparallel.py's _symmetric_params as a ModelConsts: caller constants that
    are the same on every axis."""
    rng = np.random.default_rng(seed)
    if model == 'ref15':
        g = lambda lo, hi: np.repeat(rng.uniform(lo, hi, 5), 3)  # noqa: E731 (pos, att, vel, rate, acc)
        q, ri, p0 = g(0.01, 8.0), g(0.02, 120.0), g(20.0, 2e4)
        rg = np.full(3, rng.uniform(0.5, 9.0))
    else:
        def g(lo, hi):  # [x, y, theta, vx, vy, theta_dot, ax, ay]
            a, t, v, w, c = rng.uniform(lo, hi, 5)
            return np.array([a, a, t, v, v, w, c, c])
        q, ri, p0 = g(0.01, 8.0), g(0.02, 120.0), g(20.0, 2e4)
        rg = np.full(2, rng.uniform(0.5, 9.0))
    return ref15.ModelConsts(model, q=q, r_imu=ri, r_gps=rg, p0=p0)


# ---------------------------------------------------------------------------------------------
# the margin rule (CPU)
# ---------------------------------------------------------------------------------------------
def gate_margins(et, dt, thresholds, model='ref15', K=None):
    """Covariance-only recursion of the gated filter with the NumPy oracle's matrices
    (oracle/ref_kf.py), every threshold at once: (margin [B], the smallest |logdet(P_pred) -
    threshold| over the run; n_updates [B]; min and max logdet(P_pred) of threshold 0's run)."""
    thr = np.asarray(thresholds, np.float64)
    B = len(thr)
    if model == 'ref15':
        n, Ff, Qf, Hg, Hi, Rg, Ri, P0 = (15, ref_kf.F_ref15, ref_kf.Q_ref15, ref_kf.H_gps15(), ref_kf.H_imu15(),
                                         ref_kf.R_gps15(), ref_kf.R_imu15(), ref_kf.P0_REF15)
    else:
        n, Ff, Qf, Hg, Hi, Rg, Ri, P0 = (8, ref_kf.F_ref8, ref_kf.Q_ref8, ref_kf.H_gps8(), ref_kf.H_imu8(),
                                         ref_kf.R_gps8(), ref_kf.R_imu8(), ref_kf.P0_REF8)
    if K is not None:
        Qf, Rg, Ri, P0 = ref_kf.consts_matrices(K, n)
    P = np.repeat(np.asarray(P0, np.float64)[None], B, 0)
    margin = np.full(B, np.inf)
    count = np.zeros(B, np.int64)
    lo, hi = np.inf, -np.inf
    fq = {}
    eye = np.eye(n)
    for ty, d in zip(et.tolist(), dt.tolist()):
        if ty == ref15.NONE:
            continue
        if d not in fq:
            fq[d] = (np.asarray(Ff(d), np.float64), np.asarray(Qf(d), np.float64))
        F, Q = fq[d]
        P = F @ P @ F.T + Q
        sgn, ld = np.linalg.slogdet(P)
        ld = sgn * ld
        lo, hi = min(lo, float(ld[0])), max(hi, float(ld[0]))
        with np.errstate(invalid='ignore'):
            margin = np.minimum(margin, np.where(np.isfinite(thr), np.abs(ld - thr), np.inf))
        opened = ld > thr
        H, R = (Hg, Rg) if ty == ref15.GPS else (Hi, Ri)
        S = H @ P @ H.T + R
        Kg = P @ H.T @ np.linalg.inv(S)
        Pn = (eye - Kg @ H) @ P
        P = np.where(opened[:, None, None], Pn, P)
        count += opened
    return margin, count, lo, hi


def _margins(key, et, dt, thresholds, **kw):
    return _once(('margins', key), lambda: gate_margins(et, dt, thresholds, **kw))


def pick_thresholds(et, dt, model, K, floor, n_cand=12):
    """At least 4 thresholds by the margin rule from ``n_cand`` candidates spread over the
    ungated run's log-det range; between them the update shares must run from under 10 % to over
    90 % (a condition on the inputs)."""
    _, _, lo, hi = gate_margins(et, dt, [-INF], model, K)
    cand = np.linspace(lo - 1.0, hi + 1.0, n_cand)
    margin, count, _, _ = gate_margins(et, dt, cand, model, K)
    n_ev = int(np.sum((et == ref15.GPS) | (et == ref15.IMU)))
    ok = margin >= floor
    share = count[ok] / n_ev
    assert ok.sum() >= 4 and share.min() < 0.10 and share.max() > 0.90, (margin, count, n_ev)
    return cand[ok], share


# ---------------------------------------------------------------------------------------------
# device helpers
# ---------------------------------------------------------------------------------------------
def _handle(model, B, dtype, params=None, x0=None, **kw):
    kf = kfmi.BatchedKF(model, B, dtype, params=params, **kw)
    P0 = kf.state()[1].cpu().numpy()
    xs = np.zeros((kf.n, B), P0.dtype)
    if x0 is not None:
        k = 3 if model == 'ref15' else 2
        xs[0:k] = np.asarray(x0)[0:k, None]
    kf.set_state(xs, P0)
    return kf


def _np(v):
    return None if v is None else v.cpu().numpy()


def _sweep(et, dt, pay, x0, thresholds, dtype='f64', model='ref15', params=None, state=None, **kw):
    """One sweep from the cold start (or ``state`` = (x [n, B], P [rows, B])).  Returns a dict of
    NumPy arrays in the handle's dtype: traj, logdet, updated, n_updated, ckpt_x, ckpt_P, x, P,
    status."""
    thr = np.asarray(thresholds, np.float64)
    kf = _handle(model, len(thr), dtype, params, x0)
    try:
        if state is not None:
            kf.set_state(np.ascontiguousarray(state[0]), np.ascontiguousarray(state[1]))
        npd = np.float64 if dtype == 'f64' else np.float32
        out = kf.run_sweep(et, dt, pay.astype(npd), thr, updated=True, **kw)
        x, P = kf.state()
        r = dict(zip(('traj', 'logdet', 'updated', 'n_updated', 'ckpt_x', 'ckpt_P'), map(_np, out)))
        r.update(x=_np(x), P=_np(P), status=_np(kf.status()))
        return r
    finally:
        kf.close()


def _seq(et, dt, pay, x0, thr, dtype='f64', model='ref15', params=None):
    """The existing engine: kf_run_events_seq on the chain kernel, one filter gated at ``thr``."""
    kf = _handle(model, 1, dtype, params, x0, options={'events_kernel': 'chain'})
    try:
        npd = np.float64 if dtype == 'f64' else np.float32
        tr, ld, up, _ = kf.run_events(et[:, None], dt[:, None], pay[:, :, None].astype(npd), updated=True,
                                      threshold=thr, sequential=True)
        x, P = kf.state()
        return dict(traj=_np(tr), logdet=_np(ld), updated=_np(up), x=_np(x), P=_np(P), status=_np(kf.status()))
    finally:
        kf.close()


RECORDS = ('traj', 'logdet', 'x', 'P')


def _column(r, f):
    """Filter f of a sweep's outputs, shaped as a one-filter run's."""
    return {k: (None if v is None else v[..., f:f + 1]) for k, v in r.items()}


def _assert_bitwise(a, b, keys):
    for k in keys:
        if a[k] is None and b[k] is None:
            continue
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _assert_close(a, b, tol, flags=True):
    if flags:
        np.testing.assert_array_equal(a['updated'], b['updated'])
    for k in RECORDS:
        assert a[k].shape == b[k].shape, k
        assert _rel(a[k], b[k]) <= tol, (k, _rel(a[k], b[k]))


# ---------------------------------------------------------------------------------------------
# 1, 2: against the oracle and the reference's own recording
# ---------------------------------------------------------------------------------------------
def _golden_sweep(golden_dir):
    g, events = _golden(golden_dir)
    return _once('golden_sweep', lambda: ref15.AdaptiveSweep(events, GRID + [-INF, INF], 0, len(events),
                                                             checkpoint_every=64))


def test_sweep_vs_oracle(golden_dir):
    """The golden stream under the 70-threshold grid plus -inf and +inf (B = 72: nine full
    waves): AdaptiveSweep.result(i) against oracle.ref_kf.run_adaptive_threshold per threshold.
    At most 2 of the 70 grid thresholds may be excluded by the margin rule (measured on the CPU:
    one, -28.3 with 8.8e-6)."""
    g, events = _golden(golden_dir)
    et, dt, _, _ = _golden_arrays(golden_dir)
    margin, count, _, _ = _margins('golden', et, dt, GRID)
    use = margin >= MARGIN['f64']
    assert (~use).sum() <= 2, margin[~use]
    sw = _golden_sweep(golden_dir)
    assert sw.thresholds.shape == sw.n_updates.shape == (72,)
    for i in [k for k in range(70) if use[k]] + [70, 71]:
        thr = float(sw.thresholds[i])
        st, ld, P, prev, times = ref_kf.run_adaptive_threshold(events, 0, len(events), R_threshold=thr)
        rs, rl, rP, rprev, rtimes = sw.result(i)
        np.testing.assert_array_equal(np.array(rtimes), np.array(times), err_msg=str(thr))
        assert np.array(rs).shape == np.array(st).shape
        assert _rel(rs, st) <= TOL and _rel(rl, ld) <= TOL and _rel(rP, P) <= TOL, thr
        assert rprev == prev
        assert sw.n_updates[i] == len(times) - 1
        if i < 70:
            assert sw.n_updates[i] == count[i]
    assert sw.n_updates[71] == 0 and len(sw.result(71)[4]) == 1   # +inf: the cold start's fix only
    assert sw.n_updates[70] == int(np.sum(et != ref15.NONE))       # -inf: every processed event


def test_minus_inf_is_the_ungated_filter(golden_dir):
    """thresholds = -inf always updates: the ungated filter.  Against the reference's ungated
    recording (run_kalman_filter_full's cold_logdets) within TOL over the records before the
    stream's one out-of-order event: from there the reference's two drivers differ by their own
    rules (the full driver moves its previous time back to a skipped event, kf_workers.py:683-685,
    the adaptive driver does not, :1013-1015), and the NumPy oracle's adaptive run at -inf is
    itself 1.5e-2 relative away from cold_logdets after it.  Over the whole stream: the engine's
    ungated chain kernel on the adaptive driver's stream, between kernels."""
    g, events = _golden(golden_dir)
    et, dt, pay, x0 = _golden_arrays(golden_dir)
    sw = _golden_sweep(golden_dir)
    ld = np.array(sw.result(70)[1])
    k = 1 + int(np.argmax(et == ref15.NONE))  # records before the first skipped event (the initial one included)
    assert 300 < k < len(ld) == len(g['cold_logdets'])
    assert _rel(ld[:k], g['cold_logdets'][:k]) <= TOL
    ungated = _seq(et, dt, pay, x0, None)
    keep = et != ref15.NONE
    assert _rel(ld[1:], ungated['logdet'][keep, 0]) <= KERNELS
    assert np.all(ungated['updated'][keep, 0] == 1)


def test_sweep_vs_reference_recording(golden_dir):
    """A sweep whose thresholds include the golden's own adapt_threshold, against the reference's
    recorded adaptive run (as test_adaptive_threshold)."""
    g, events = _golden(golden_dir)
    thr = [-11.4, float(g['adapt_threshold']), 0.3]
    sw = ref15.run_adaptive_threshold_sweep(events, thr, start_idx=0, end_idx=len(events), checkpoint_every=0)
    st, ld, P, prev, times = sw.result(1)
    np.testing.assert_array_equal(np.array(times), g['adapt_times'])
    assert _rel(st, g['adapt_states']) <= TOL
    assert _rel(ld, g['adapt_logdets']) <= TOL
    assert _rel(P, g['adapt_P']) <= TOL
    assert sw.n_updates[1] == len(g['adapt_times']) - 1


# ---------------------------------------------------------------------------------------------
# 3: lanes are independent
# ---------------------------------------------------------------------------------------------
def _single(golden_dir, thr):
    et, dt, pay, x0 = _golden_arrays(golden_dir)
    return _once(('single', thr), lambda: _sweep(et, dt, pay, x0, [thr]))


@pytest.mark.parametrize('B', [1, 8, 9, 72])
def test_lanes_are_independent(golden_dir, B):
    """Filter f of a sweep of B thresholds equals a one-filter sweep at thresholds[f] bit for bit:
    records, flags, counts, final state and status (B = 9: one full wave plus one group)."""
    et, dt, pay, x0 = _golden_arrays(golden_dir)
    thr = (GRID + [-INF, INF])[::-1][:B] if B < 72 else GRID + [-INF, INF]
    r = _sweep(et, dt, pay, x0, thr)
    assert r['traj'].shape == (len(et), 6, B) and r['updated'].shape == (len(et), B)
    for f in range(B):
        one = _single(golden_dir, thr[f])
        _assert_bitwise(_column(r, f), one, ('traj', 'logdet', 'updated', 'n_updated', 'x', 'P', 'status'))
    assert int(np.abs(r['status']).sum()) == 0


# ---------------------------------------------------------------------------------------------
# 4, 5: against the existing engine
# ---------------------------------------------------------------------------------------------
def test_sweep_vs_chain_kernel():
    """Stream 4 (5000 events, 300 NONE) under ten thresholds as filters of one sweep, each against
    kf_run_events_seq (chain kernel, B = 1) at that threshold: flags equal, records, final x and
    P within 1e-9 relative; NONE events leave the state and write records.  No threshold may be
    excluded by the margin rule (measured: margins >= 4e-5)."""
    et, dt, pay, x0 = _stream4()
    margin, count, _, _ = _margins('stream4', et, dt, STREAM4_THR)
    assert np.all(margin >= MARGIN['f64']), margin
    r = _sweep(et, dt, pay, x0, STREAM4_THR)
    assert int(np.abs(r['status']).sum()) == 0
    np.testing.assert_array_equal(r['n_updated'], count)
    np.testing.assert_array_equal(r['n_updated'], r['updated'].sum(0))
    for f, thr in enumerate(STREAM4_THR):
        _assert_close(_column(r, f), _seq(et, dt, pay, x0, thr), KERNELS)
    none = np.nonzero(et == ref15.NONE)[0]
    assert len(none) == 300 and none[0] > 0
    assert not r['updated'][none].any()
    np.testing.assert_array_equal(r['traj'][none], r['traj'][none - 1])
    np.testing.assert_array_equal(r['logdet'][none], r['logdet'][none - 1])


@pytest.mark.parametrize('T', [0, 1, 7, 8, 9])
def test_short_streams(T):
    """The first T events of stream 4 at thresholds -10 and -inf (the input ring's prologue and
    tail): each filter equals kf_run_events_seq; T = 0 leaves the handle's state bitwise unchanged
    and launches nothing."""
    et, dt, pay, x0 = (v[:T] if v.ndim and len(v) == 5000 else v for v in _stream4())
    thr = [-10.0, -INF]
    kf = _handle('ref15', 2, 'f64', x0=x0)
    try:
        x_in, P_in = (_np(v) for v in kf.state())
        tr, ld, up, nu, cx, cP = kf.run_sweep(et, dt, pay, np.array(thr), updated=True, checkpoint_every=4)
        x, P = (_np(v) for v in kf.state())
        assert tr.shape == (T, 6, 2) and cx.shape == (T // 4, 15, 2) and cP.shape == (T // 4, 27, 2)
        if T == 0:
            np.testing.assert_array_equal(x, x_in)
            np.testing.assert_array_equal(P, P_in)
            assert int(nu.sum()) == 0
            return
        r = dict(traj=_np(tr), logdet=_np(ld), updated=_np(up), x=x, P=P)
    finally:
        kf.close()
    for f in range(2):
        _assert_close(_column(r, f), _seq(et, dt, pay, x0, thr[f]), KERNELS)


# ---------------------------------------------------------------------------------------------
# 6: checkpoints
# ---------------------------------------------------------------------------------------------
def test_checkpoints_are_the_prefix_runs():
    """Stream 4 with ckpt_every = 512 (C = 9, T no multiple of it): row c of ckpt_x / ckpt_P is
    the final state of a sweep over the first (c + 1) 512 events, and a sweep started from row c
    over the remaining events reproduces the full run's tail records and final state, bit for
    bit."""
    et, dt, pay, x0 = _stream4()
    thr = STREAM4_THR[1::3]
    full = _sweep(et, dt, pay, x0, thr, checkpoint_every=512)
    assert full['ckpt_x'].shape == (9, 15, len(thr)) and full['ckpt_P'].shape == (9, 27, len(thr))
    for c in range(9):
        n = (c + 1) * 512
        head = _sweep(et[:n], dt[:n], pay[:n], x0, thr)
        np.testing.assert_array_equal(full['ckpt_x'][c], head['x'])
        np.testing.assert_array_equal(full['ckpt_P'][c], head['P'])
        if c in (0, 4, 8):
            tail = _sweep(et[n:], dt[n:], pay[n:], x0, thr, state=(full['ckpt_x'][c], full['ckpt_P'][c]))
            for k in ('traj', 'logdet', 'updated'):
                np.testing.assert_array_equal(tail[k], full[k][n:], err_msg=k)
            _assert_bitwise(tail, full, ('x', 'P', 'status'))
            np.testing.assert_array_equal(head['n_updated'] + tail['n_updated'], full['n_updated'])


def test_checkpoint_period_around_the_stream_length(golden_dir):
    """ckpt_every in {T - 1, T, T + 1} on the golden stream: one row (the filter after event
    T - 2, or the final state) or none; T + 1 writes no checkpoint and accepts null arrays."""
    et, dt, pay, x0 = _golden_arrays(golden_dir)
    T = len(et)
    thr = [-25.0, -11.4]
    base = _sweep(et, dt, pay, x0, thr)
    short = _sweep(et[:T - 1], dt[:T - 1], pay[:T - 1], x0, thr)
    for every, rows, want in ((T - 1, 1, short), (T, 1, base), (T + 1, 0, None)):
        r = _sweep(et, dt, pay, x0, thr, checkpoint_every=every)
        assert r['ckpt_x'].shape == (rows, 15, 2) and r['ckpt_P'].shape == (rows, 27, 2)
        _assert_bitwise(r, base, ('traj', 'logdet', 'updated', 'n_updated', 'x', 'P'))
        if rows:
            np.testing.assert_array_equal(r['ckpt_x'][0], want['x'])
            np.testing.assert_array_equal(r['ckpt_P'][0], want['P'])
    # the C ABI with ckpt_every = T + 1 and NULL checkpoint arrays
    kf = _handle('ref15', 2, 'f64', x0=x0)
    try:
        d = kf.device
        a = [torch.as_tensor(v, device=d) for v in (et, dt, pay, np.array(thr))]
        rc = _lib.lib().kf_run_sweep(kf.handle, T, *(v.data_ptr() for v in a), None, None, None, None, T + 1, None,
                                     None, kf._stream())
        assert rc == _lib.KF_OK, _lib.last_error()
        x, P = (_np(v) for v in kf.state())
        np.testing.assert_array_equal(x, base['x'])
        np.testing.assert_array_equal(P, base['P'])
    finally:
        kf.close()


# ---------------------------------------------------------------------------------------------
# 7: warm starts
# ---------------------------------------------------------------------------------------------
WARM_THR = [-25.0, -11.4, 0.3]


def _check_warm_starts(sw, events, plain, thresholds, ends):
    for end in ends:
        for i, thr in enumerate(thresholds):
            want = ref15.run_adaptive_threshold_kalman_filter(events, 0, end, R_threshold=thr)
            got = sw.warm_start(i, end)
            if want is None:
                assert got is None
                continue
            state, P, prev = got
            assert len(state) == 7
            assert _rel(state, want[0][-1]) <= KERNELS and _rel(P, want[2]) <= KERNELS, (end, thr)
            assert state[0] == want[0][-1][0] and prev == want[3]
            ost, _, oP, oprev, _ = ref_kf.run_adaptive_threshold(plain, 0, end, R_threshold=thr)
            assert _rel(state, ost[-1]) <= TOL and _rel(P, oP) <= TOL and prev == oprev, (end, thr)


def test_warm_start(golden_dir):
    """warm_start(i, end_idx) on the golden stream with checkpoint_every = 64: the checkpoint at
    or before end_idx plus a one-filter sweep over the tail (none at 68: the prefix ends on a
    checkpoint), against run_adaptive_threshold_kalman_filter(0, end_idx) and the oracle; an
    end_idx at or before the first fix (index 5) returns None.  The three thresholds must have a
    margin >= 1e-5 over the whole run, hence at every prefix (none may be excluded)."""
    g, events = _golden(golden_dir)
    et, dt, _, _ = _golden_arrays(golden_dir)
    margin, _, _, _ = _margins('golden_warm', et, dt, WARM_THR)
    assert np.all(margin >= MARGIN['f64']), margin
    sw = ref15.AdaptiveSweep(events, WARM_THR, 0, len(events), checkpoint_every=64, records=False)
    assert sw.warm_start(0, 3) is None and sw.warm_start(2, 5) is None
    with pytest.raises(ValueError):
        sw.result(0)
    _check_warm_starts(sw, events, events, WARM_THR, (1, 6, 64, 65, 68, 200, 427))
    sw.close()


@pytest.fixture(scope='module')
def csvs(golden_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp('sweep')
    out = []
    for name in ('gps_synth.csv.gz', 'imu_synth.csv.gz'):
        p = d / name[:-3]
        with gzip.open(os.path.join(golden_dir, name), 'rt') as fi:
            p.write_text(fi.read())
        out.append(str(p))
    return out


def test_warm_start_on_the_ingested_stream(csvs):
    """The device-resident path: the façade's sweep over its ingested EventStream (built as
    tests/test_gpu_compat.py builds one), warm starts and one whole result against the driver over
    the same list and the oracle over the plain tuples.  Thresholds by the margin rule from 12
    candidates over the window's log-det range (at least 3 must pass)."""
    sf = kfw.KF_SensorFusion(*csvs)
    sf.load_data()
    sf.gps_to_modified_utm()
    bw, ba, _ = sf.compute_imu_biases(sf.gps_data, sf.imu_data)
    sf.unbias_imu_data(bw, ba)
    sf.combine_sensor_data()
    ev = sf.indexed_sensor_data
    assert ref15._device_stream(ev) is not None
    end = 1300
    plain = list(ev)[:end]
    et, dt, _, _ = _list_arrays(plain)
    _, _, lo, hi = gate_margins(et, dt, [-INF])
    cand = np.linspace(lo + 1.0, hi - 1.0, 12)
    margin, count, _, _ = gate_margins(et, dt, cand)
    ok = margin >= MARGIN['f64']
    assert ok.sum() >= 3, margin
    thr = [float(v) for v in cand[ok][[0, ok.sum() // 2, -1]]]
    sw = sf.run_adaptive_threshold_sweep(thr, 0, end, checkpoint_every=256)
    first = next(i for i, e in enumerate(plain) if e[1] == 'GPS')
    assert sw.warm_start(0, first) is None
    _check_warm_starts(sw, ev, plain, thr, (first + 1, first + 256, 700, end))
    for i in (0, 2):
        a = sw.result(i)
        b = ref15.run_adaptive_threshold_kalman_filter(ev, 0, end, R_threshold=thr[i])
        assert a[4] == b[4] and a[3] == b[3] and len(a[0]) == len(b[0])
        assert _rel(a[0], b[0]) <= KERNELS and _rel(a[1], b[1]) <= KERNELS and _rel(a[2], b[2]) <= KERNELS
    sw.close()


# ---------------------------------------------------------------------------------------------
# 8: models, constants, f32
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', ['ref8', 'ref15'])
def test_models_and_custom_constants(model):
    """ref8 and ref15 with custom axis-symmetric constants, f64: the sweep against
    kf_run_events_seq per threshold, flags equal and records within 1e-9; thresholds picked by the
    margin rule (pick_thresholds: at least 4 of 12 candidates, update shares from under 10 % to
    over 90 %)."""
    consts = _symmetric_consts(model, 5)
    et, dt, pay, x0 = _stream(1500, seed=23, skips=40)
    thr, share = pick_thresholds(et, dt, model, consts.oracle(), MARGIN['f64'])
    r = _sweep(et, dt, pay, x0, thr, model=model, params=consts.params())
    assert int(np.abs(r['status']).sum()) == 0
    n_ev = int(np.sum(et != ref15.NONE))
    np.testing.assert_array_equal(r['n_updated'], np.rint(share * n_ev).astype(np.int64))
    for f in range(len(thr)):
        _assert_close(_column(r, f), _seq(et, dt, pay, x0, float(thr[f]), model=model, params=consts.params()),
                      KERNELS)


def test_ref8_reference_constants():
    """ref8 with the reference's own constants (the kernel's compile-time literals)."""
    et, dt, pay, x0 = _stream(1500, seed=23, skips=40)
    thr, _ = pick_thresholds(et, dt, 'ref8', None, MARGIN['f64'])
    r = _sweep(et, dt, pay, x0, thr, model='ref8')
    for f in range(len(thr)):
        _assert_close(_column(r, f), _seq(et, dt, pay, x0, float(thr[f]), model='ref8'), KERNELS)


def test_f32(golden_dir):
    """f32 on the golden stream under the six thresholds whose margin is >= 1e-2 (none may be
    excluded): flags equal the f32 kf_run_events_seq, records within 1e-4 relative."""
    et, dt, pay, x0 = _golden_arrays(golden_dir)
    margin, _, _, _ = _margins('golden_f32', et, dt, F32_THR)
    assert np.all(margin >= MARGIN['f32']), margin
    r = _sweep(et, dt, pay, x0, F32_THR, dtype='f32')
    assert r['traj'].dtype == np.float32 and int(np.abs(r['status']).sum()) == 0
    for f, thr in enumerate(F32_THR):
        _assert_close(_column(r, f), _seq(et, dt, pay, x0, thr, dtype='f32'), 1e-4)


# ---------------------------------------------------------------------------------------------
# 9, 10: failures
# ---------------------------------------------------------------------------------------------
def test_failure_is_per_filter(golden_dir):
    """One filter of eight starts from a covariance that is not positive definite: it ends NaN
    with KF_ENOTSPD; the other seven equal their one-filter runs bit for bit."""
    et, dt, pay, x0 = _golden_arrays(golden_dir)
    thr = [-INF] * 4 + [-25.0, -11.4, 0.3, INF]
    kf = _handle('ref15', 8, 'f64', x0=x0)
    x, P = (_np(v) for v in kf.state())
    kf.close()
    bad = 2
    P[0, bad] = -1e6  # var(pos_x) < -R_gps: the first fix's innovation variance is negative
    r = _sweep(et, dt, pay, x0, thr, state=(x, P))
    assert r['status'][bad] == _lib.KF_ENOTSPD
    assert np.isnan(r['x'][:, bad]).all() and np.isnan(r['P'][:, bad]).all() and np.isnan(r['traj'][-1, :, bad]).all()
    for f in range(8):
        if f == bad:
            continue
        assert r['status'][f] == 0
        _assert_bitwise(_column(r, f), _single(golden_dir, thr[f]),
                        ('traj', 'logdet', 'updated', 'n_updated', 'x', 'P', 'status'))


def test_argument_errors(golden_dir):
    """KF_EINVAL with its text for a cv3 handle, T = -1, null thresholds, ckpt_every = -1 and
    ckpt_every = 64 with null checkpoint arrays; nothing is launched (the handle's state stays)."""
    et, dt, pay, x0 = _golden_arrays(golden_dir)
    T = len(et)
    L = _lib.lib()
    kf = _handle('ref15', 2, 'f64', x0=x0)
    cv = kfmi.BatchedKF('cv3', 2, 'f64')
    try:
        d = kf.device
        e, t, p, th = (torch.as_tensor(v, device=d) for v in (et, dt, pay, np.array([-10.0, 0.0])))
        cx, cP = kf.empty(T // 64, 15, 2), kf.empty(T // 64, 27, 2)
        x_in, P_in = (_np(v) for v in kf.state())

        def call(h, n, thr, every, ckx, ckp):
            return L.kf_run_sweep(h.handle, n, e.data_ptr(), t.data_ptr(), p.data_ptr(), thr, None, None, None, None,
                                  every, ckx, ckp, kf._stream())
        for args, text in (((cv, T, th.data_ptr(), 0, None, None), 'KF_MODEL_REF15'),
                           ((kf, -1, th.data_ptr(), 0, None, None), 'T = -1'),
                           ((kf, T, None, 0, None, None), 'null thresholds'),
                           ((kf, T, th.data_ptr(), -1, None, None), 'ckpt_every = -1'),
                           ((kf, T, th.data_ptr(), 64, None, None), 'null ckpt_x/ckpt_P'),
                           ((kf, T, th.data_ptr(), 64, cx.data_ptr(), None), 'null ckpt_x/ckpt_P')):
            assert call(*args) == _lib.KF_EINVAL, text
            assert text in _lib.last_error(), (text, _lib.last_error())
            with pytest.raises(kfmi.KFError) as err:
                _lib.check(call(*args))
            assert err.value.code == _lib.KF_EINVAL
        with pytest.raises(ValueError):
            cv.run_sweep(et, dt, pay, np.array([-10.0, 0.0]))
        with pytest.raises(ValueError):
            kf.run_sweep(et, dt, pay, np.array([-10.0, 0.0]), checkpoint_every=-1)
        torch.cuda.synchronize()
        x, P = (_np(v) for v in kf.state())
        np.testing.assert_array_equal(x, x_in)
        np.testing.assert_array_equal(P, P_in)
        # the same call with its arrays is accepted
        assert call(kf, T, th.data_ptr(), 64, cx.data_ptr(), cP.data_ptr()) == _lib.KF_OK, _lib.last_error()
        torch.cuda.synchronize()
        assert not np.array_equal(_np(kf.state()[0]), x_in)
    finally:
        kf.close()
        cv.close()
