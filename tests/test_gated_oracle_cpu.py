"""tests/gated_oracle.py (the dense array-form gated oracle of test_gpu_gated_oracle.py) pinned on
the CPU: against the list-form oracle.ref_kf.run_adaptive_threshold, against a ref_kf.step8 loop,
and its margin against test_gpu_sweep.gate_margins.  No GPU."""
import os

import numpy as np
import pytest

import gated_oracle
from golden_events import unpack_events
from oracle import ref_kf
from test_gpu_sweep import STREAM4_THR, WARM_THR, _list_arrays, _stream, gate_margins

RTOL = 1e-12
INF = float('inf')


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)))


@pytest.fixture(scope='module')
def golden15(golden_dir):
    events = unpack_events(np.load(os.path.join(golden_dir, 'ref15_full.npz')))
    et, dt, pay, x0 = _list_arrays(events)
    return events, et, dt, pay, x0


def _thresholds(golden15):
    """test_gpu_sweep's WARM_THR (-25, -11.4, 0.3: spread over the gated runs' log-det range on
    this stream, from most events updating to few) and -inf.  They must lie inside the range
    between the lowest record of the always-updating run and the highest of the never-updating."""
    _, et, dt, pay, x0 = golden15
    lo = float(gated_oracle.run_gated('ref15', et, dt, pay, x0, ref_kf.P0_REF15, -INF).logdet.min())
    hi = float(gated_oracle.run_gated('ref15', et, dt, pay, x0, ref_kf.P0_REF15, INF).logdet.max())
    assert all(lo < t < hi for t in WARM_THR), (lo, hi)
    return WARM_THR + [-INF]


@pytest.mark.parametrize('which', [0, 1, 2, 3])
def test_ref15_equals_the_list_form_oracle(golden15, which):
    """The golden event list as arrays (a dt < 0 event is NONE) under three thresholds spread over
    the log-det range and -inf: the update times equal run_adaptive_threshold's, the states,
    log-dets and final P agree to 1e-12 relative.  The arithmetic is the same calls on the same
    numbers, and the results are in fact bitwise equal here (asserted: a later difference is a
    change of the helper, not rounding)."""
    events, et, dt, pay, x0 = golden15
    thr = _thresholds(golden15)[which]
    st, ld, P, prev, times = ref_kf.run_adaptive_threshold(events, 0, len(events), thr)
    r = gated_oracle.run_gated('ref15', et, dt, pay, x0, ref_kf.P0_REF15, thr)
    s = next(i for i, e in enumerate(events) if e[1] == 'GPS')
    t = np.array([e[2] for e in events[s:]])
    keep = et != gated_oracle.NONE
    assert 0 < (~keep).sum() < 10 and keep.sum() == len(st) - 1
    np.testing.assert_array_equal(t[r.updated == 1], np.array(times[1:]))
    assert not r.updated[~keep].any()
    if np.isfinite(thr):
        assert 2 < r.updated.sum() < keep.sum() - 2, r.updated.sum()  # the gate both opens and stays shut
        assert np.isfinite(r.margin) and r.margin == np.nanmin(np.abs(r.gate - thr))
    else:
        assert r.updated[keep].all() and r.margin == INF and np.isnan(r.gate).all()
    want = np.array(st)[:, 1:]
    assert _rel(r.traj[keep], want[1:]) <= RTOL
    assert _rel(r.logdet[keep], ld[1:]) <= RTOL
    assert _rel(r.P, P) <= RTOL and _rel(r.x[:6], want[-1]) <= RTOL
    np.testing.assert_array_equal(r.traj[keep], want[1:])
    np.testing.assert_array_equal(r.logdet[keep], np.array(ld[1:]))
    np.testing.assert_array_equal(r.P, P)
    # a NONE event repeats the record before it
    none = np.nonzero(~keep)[0]
    np.testing.assert_array_equal(r.traj[none], r.traj[none - 1])
    np.testing.assert_array_equal(r.logdet[none], r.logdet[none - 1])


@pytest.mark.parametrize('prefix', ['', 'ooo_'])
def test_ref8_minus_inf_is_the_step8_loop(golden_dir, prefix):
    """ref8 at -inf reproduces a ref_kf.step8 loop over the ref8_full.npz events (from the first
    fix, at dt = 0; hw5_2.py has no dt < 0 guard) to 1e-12: states, log-dets, every covariance."""
    events = unpack_events(np.load(os.path.join(golden_dir, 'ref8_full.npz')), prefix)
    first = next(i for i, e in enumerate(events) if e[1] == 'GPS')
    ev = events[first:]
    T = len(ev)
    et, dt, pay = np.zeros(T, np.uint8), np.zeros(T), np.zeros((T, 9))
    prev = ev[0][2]
    for j, (_, stype, t, sd) in enumerate(ev):
        et[j] = gated_oracle.GPS if stype == 'GPS' else gated_oracle.IMU
        dt[j] = t - prev
        pay[j] = [sd['easting'], sd['northing'], 0, 0, 0, 0, 0, 0, 0] if stype == 'GPS' else [float(v) for v in sd[1:10]]
        prev = t
    assert (dt < 0).any() == (prefix == 'ooo_')
    r = gated_oracle.run_gated('ref8', et, dt, pay, np.zeros(8), ref_kf.P0_REF8, -INF, cov=True)
    assert r.traj.shape == (T, 3) and r.cov.shape == (T, 8, 8) and r.updated.all()
    x, P = np.zeros(8), ref_kf.P0_REF8.copy()
    for j, (_, stype, t, sd) in enumerate(ev):
        x, P = ref_kf.step8(x, P, stype, sd, dt[j])
        assert _rel(r.traj[j], x[:3]) <= RTOL and _rel(r.cov[j], P) <= RTOL, j
        assert _rel(r.logdet[j], np.linalg.slogdet(P)[1]) <= RTOL, j
    assert _rel(r.x, x) <= RTOL and _rel(r.P, P) <= RTOL


def test_margin_equals_gate_margins():
    """Stream 4 (5,000 events, 300 NONE) under STREAM4_THR: the margin and the update count of
    each run equal test_gpu_sweep.gate_margins' covariance-only recursion (1e-9; the batched
    recursion multiplies in another order)."""
    et, dt, pay, x0 = _stream(5000, seed=11, skips=300)
    margin, count, _, _ = gate_margins(et, dt, STREAM4_THR)
    for k, thr in enumerate(STREAM4_THR):
        r = gated_oracle.run_gated('ref15', et, dt, pay, x0, ref_kf.P0_REF15, thr)
        assert abs(r.margin - margin[k]) <= 1e-9, (thr, r.margin, margin[k])
        assert int(r.updated.sum()) == count[k]


def test_event_types_and_thresholds():
    """KF_EVENT_PREDICT only predicts (no gate, no update), KF_EVENT_NONE leaves the filter and
    writes its record, +inf and NaN never update, and custom constants reach Q, R_gps and R_imu."""
    et, dt, pay, x0 = _stream(400, seed=3, skips=20)
    et = et.copy()
    et[5::7] = gated_oracle.PREDICT
    P0 = ref_kf.P0_REF15
    for thr in (INF, float('nan')):
        r = gated_oracle.run_gated('ref15', et, dt, pay, x0, P0, thr)
        assert not r.updated.any() and r.margin == INF
    full = gated_oracle.run_gated('ref15', et, dt, pay, x0, P0, -INF, cov=True)
    x, P = x0.copy(), P0.copy()
    for t in range(len(et)):
        if et[t] == gated_oracle.PREDICT:
            F = ref_kf.F_ref15(dt[t])
            x, P = F @ x, ref_kf.predict_covariance(P, F, ref_kf.Q_ref15(dt[t]))
        elif et[t] != gated_oracle.NONE:
            sd = ({'easting': pay[t, 0], 'northing': pay[t, 1], 'altitude': pay[t, 2]} if et[t] == gated_oracle.GPS
                  else ['t', *pay[t]])
            x, P = ref_kf.step15(x, P, 'GPS' if et[t] == gated_oracle.GPS else 'IMU', sd, dt[t])
        assert full.updated[t] == (et[t] in (gated_oracle.GPS, gated_oracle.IMU))
        assert _rel(full.traj[t], x[:6]) <= RTOL and _rel(full.cov[t], P) <= RTOL, t
    K = dict(q=np.linspace(0.1, 3.0, 15), r_imu=np.linspace(1.0, 40.0, 15), r_gps=np.array([2.0, 2.5, 4.0]),
             p0=np.linspace(50.0, 900.0, 15))
    keep = et != gated_oracle.PREDICT
    r = gated_oracle.run_gated('ref15', et[keep], dt[keep], pay[keep], x0, np.diag(K['p0']), -INF, K=K)
    x, P = x0.copy(), np.diag(K['p0'])
    for ty, d, p in zip(et[keep], dt[keep], pay[keep]):
        if ty != gated_oracle.NONE:
            sd = {'easting': p[0], 'northing': p[1], 'altitude': p[2]} if ty == gated_oracle.GPS else ['t', *p]
            x, P = ref_kf.step15(x, P, 'GPS' if ty == gated_oracle.GPS else 'IMU', sd, d, K)
    assert _rel(r.x, x) <= RTOL and _rel(r.P, P) <= RTOL
