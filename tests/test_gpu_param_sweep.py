"""Parameter sweep: ONE event stream under B constant sets (and gates) in one launch
(kf_run_sweep_params through BatchedKF.run_sweep(consts=...), kfmi.ref15.ParameterSweep and the
façade) — needs an MI355X.

The existing route for a constant set is one handle allocated with kf_params = that set (the
CUSTOM kernels, or the reference's literals for the reference's own set) and a one-filter
kf_run_sweep.  The parameter sweep runs the same event step with the same values in the lane's
registers, so column f is compared with that run by ==.  Inputs are tests/test_gpu_sweep.py's
stream and constant sets, imported.
"""
import numpy as np
import pytest
import torch

import kfmi
from kfmi import _lib, engine, ref15
from kfmi import kf_workers as kfw
from oracle import ref_kf
from test_gpu_sweep import INF, KERNELS, MARGIN, TOL, _column, _np, _once, _rel, _stream, _symmetric_consts, gate_margins

pytestmark = pytest.mark.gpu
NAN = float('nan')
NPD = {'f64': np.float64, 'f32': np.float32}
ALL = ('traj', 'logdet', 'updated', 'n_updated', 'x', 'P', 'status', 'ckpt_x', 'ckpt_P')
BMAX = 17
# filter f's gate: -inf (no gate), finite values that open for a part of the run, +inf and NaN (never)
THRESHOLDS = [-INF, 40.0, INF, 0.0, NAN, -20.0, 80.0, 20.0, -INF, 60.0, -40.0, NAN, 10.0, INF, 30.0, -10.0, 50.0]


def _sets(model):
    """Filter f's constants: the reference's own in column 0, then axis-symmetric custom sets."""
    return _once(('psets', model),
                 lambda: [ref15.ModelConsts(model)] + [_symmetric_consts(model, 100 + f) for f in range(1, BMAX)])


def _events(T):
    return _once(('pstream', T), lambda: _stream(T, seed=31, gps_every=7, skips=(6 if T >= 100 else 0)))


def _start(model, sets, x0, dtype):
    """The cold start of every column: the stream's first fix, and the set's own P0."""
    n, k = (15, 3) if model == 'ref15' else (8, 2)
    x = np.zeros((n, len(sets)), NPD[dtype])
    x[0:k] = np.asarray(x0)[0:k, None]
    P = np.stack([ref15.to_blocks(c.P0) for c in sets], 1).astype(NPD[dtype])
    return x, P


def _run(model, dtype, et, dt, pay, x, P, thresholds, consts=None, params=None, every=0):
    """One sweep from (x, P) on a handle of len(thresholds) filters allocated with ``params``."""
    kf = kfmi.BatchedKF(model, x.shape[1], dtype, params=params)
    try:
        kf.set_state(np.ascontiguousarray(x), np.ascontiguousarray(P))
        thr = None if thresholds is None else np.asarray(thresholds, np.float64)
        out = kf.run_sweep(et, dt, pay.astype(NPD[dtype]), thr, updated=True, checkpoint_every=every, consts=consts)
        xs, Ps = kf.state()
        r = dict(zip(('traj', 'logdet', 'updated', 'n_updated', 'ckpt_x', 'ckpt_P'), map(_np, out)))
        r.update(x=_np(xs), P=_np(Ps), status=_np(kf.status()))
        return r
    finally:
        kf.close()


def _one_filter(model, dtype, T, f, every):
    """The existing route: a handle with kf_params = set f, one filter, kf_run_sweep."""
    def run():
        et, dt, pay, x0 = _events(T)
        c = _sets(model)[f]
        x, P = _start(model, [c], x0, dtype)
        return _run(model, dtype, et, dt, pay, x, P, [THRESHOLDS[f]], params=c.params(), every=every)
    return _once(('one', model, dtype, T, f, every), run)


def _assert_equal(a, b, keys=ALL, msg=''):
    """==, NaNs in the same places."""
    for k in keys:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f'{k} {msg}')


# ---------------------------------------------------------------------------------------------
# bit for bit against one handle and one launch per set
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 3, 19, 300])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_column_equals_one_filter_run(model, dtype, T):
    """Column f of a B-filter parameter sweep == a one-filter kf_run_sweep at thresholds[f] on a
    handle allocated with kf_params = set f (the CUSTOM instantiation; column 0 holds the
    reference's constants and its handle runs the literals): records, counts, final state, status
    and every checkpoint row.  B = 1, 8, 9, 17 (a partial group of 8, a second and third wave);
    T = 1, 3, 19, 300 with the ring depth 4 (prologue only, remainder only, steady state)."""
    et, dt, pay, x0 = _events(T)
    every = 64 if T >= 64 else 2
    sets = _sets(model)
    assert sets[0].params() is None and all(c.params() is not None for c in sets[1:])
    for B in (1, 8, 9, 17):
        x, P = _start(model, sets[:B], x0, dtype)
        r = _run(model, dtype, et, dt, pay, x, P, THRESHOLDS[:B], consts=sets[:B], every=every)
        assert r['traj'].shape == (T, 6 if model == 'ref15' else 3, B) and r['ckpt_x'].shape[0] == T // every
        for f in range(B):
            _assert_equal(_column(r, f), _one_filter(model, dtype, T, f, every), msg=f'B={B} f={f}')
    if T == 300:  # the gates did something: some finite threshold opened for a part of the run
        share = r['n_updated'] / int(np.sum(et != ref15.NONE))
        assert share[0] == 1.0 and share[2] == 0.0 and share[4] == 0.0
        assert np.any((share > 0.02) & (share < 0.98)), share


def test_null_consts_is_run_sweep():
    """consts = NULL through the new entry point is kf_run_sweep: bit for bit, on a CUSTOM handle."""
    et, dt, pay, x0 = _events(300)
    c = _sets('ref15')[3]
    thr = THRESHOLDS[:9]
    x, P = _start('ref15', [c] * 9, x0, 'f64')
    want = _run('ref15', 'f64', et, dt, pay, x, P, thr, params=c.params(), every=64)
    kf = kfmi.BatchedKF('ref15', 9, 'f64', params=c.params())
    try:
        kf.set_state(x, P)
        d = kf.device
        a = [torch.as_tensor(v, device=d) for v in (et, dt, pay, np.array(thr))]
        tr, ld = kf.empty(300, 6, 9), kf.empty(300, 9)
        up = torch.empty(300, 9, dtype=torch.uint8, device=d)
        nu = torch.zeros(9, dtype=torch.int32, device=d)
        cx, cP = kf.empty(4, 15, 9), kf.empty(4, 27, 9)
        rc = _lib.lib().kf_run_sweep_params(kf.handle, 300, *(v.data_ptr() for v in a), None, tr.data_ptr(),
                                            ld.data_ptr(), up.data_ptr(), nu.data_ptr(), 64, cx.data_ptr(),
                                            cP.data_ptr(), kf._stream())
        assert rc == _lib.KF_OK, _lib.last_error()
        xs, Ps = kf.state()
        got = dict(traj=_np(tr), logdet=_np(ld), updated=_np(up), n_updated=_np(nu), ckpt_x=_np(cx), ckpt_P=_np(cP),
                   x=_np(xs), P=_np(Ps), status=_np(kf.status()))
        _assert_equal(got, want)
        # without a table the thresholds stay mandatory, as in kf_run_sweep
        rc = _lib.lib().kf_run_sweep_params(kf.handle, 300, *(v.data_ptr() for v in a[:3]), None, None, None, None, None,
                                            None, 0, None, None, kf._stream())
        assert rc == _lib.KF_EINVAL and 'null thresholds' in _lib.last_error()
    finally:
        kf.close()


def test_null_thresholds_is_ungated():
    """thresholds = NULL with a table: every filter -inf."""
    et, dt, pay, x0 = _events(300)
    sets = _sets('ref8')[:9]
    x, P = _start('ref8', sets, x0, 'f64')
    a = _run('ref8', 'f64', et, dt, pay, x, P, None, consts=sets)
    b = _run('ref8', 'f64', et, dt, pay, x, P, [-INF] * 9, consts=sets)
    _assert_equal(a, b)
    assert np.all(a['n_updated'] == int(np.sum(et != ref15.NONE)))


# ---------------------------------------------------------------------------------------------
# against the NumPy oracle
# ---------------------------------------------------------------------------------------------
ORACLE_THR = {'ref15': [-INF, 40.0, INF, 0.0, 70.0, -20.0, 80.0, 20.0, 60.0],
              'ref8': [-INF, 20.0, INF, -0.5, 35.0, -10.0, 40.0, 10.0, 30.0]}


def _oracle_run(model, K, et, dt, pay, x0, thr):
    """The gated filter on oracle/ref_kf.py's primitives with the constants K (ModelConsts.oracle()):
    step15 / step8 where the gate logdet(P_pred) > thr opens, their predict alone where it does
    not; records after every event (a NONE event repeats the last)."""
    n, k, step, Ff, w = (15, 3, ref_kf.step15, ref_kf.F_ref15, 6) if model == 'ref15' else \
        (8, 2, ref_kf.step8, ref_kf.F_ref8, 3)
    Qf, _, _, P0 = ref_kf.consts_matrices(K, n)
    x = np.zeros(n)
    x[0:k] = x0[0:k]
    P = P0.copy()
    traj, ld, up = np.zeros((len(et), w)), np.zeros(len(et)), np.zeros(len(et), np.uint8)
    for t in range(len(et)):
        if et[t] != ref15.NONE:
            F = Ff(dt[t])
            Pp = ref_kf.predict_covariance(P, F, Qf(dt[t]))
            sgn, l = np.linalg.slogdet(Pp)
            if sgn * l > thr:
                if et[t] == ref15.GPS:
                    sd = {'easting': pay[t, 0], 'northing': pay[t, 1], 'altitude': pay[t, 2]}
                    x, P = step(x, P, 'GPS', sd, dt[t], K)
                else:
                    x, P = step(x, P, 'IMU', ['t', *pay[t]], dt[t], K)
                up[t] = 1
            else:
                x, P = np.dot(F, x), Pp
        traj[t], ld[t] = x[:w], np.linalg.slogdet(P)[1]
    return dict(traj=traj, logdet=ld, updated=up, x=x, P=P)


@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_columns_vs_oracle(model):
    """B = 9, T = 300, f64: every column against the oracle run with its own constants and
    threshold, flags equal and records within the sweep tests' TOL.  First the margin rule: every
    finite threshold must be at least MARGIN away from the oracle's logdet(P_pred) over the whole
    run under that column's constants (none may be excluded), and the finite thresholds' update
    shares must reach from under 25 % to over 75 % (conditions on the inputs)."""
    et, dt, pay, x0 = _events(300)
    sets, thr = _sets(model)[:9], ORACLE_THR[model]
    shares = []
    n_ev = int(np.sum(et != ref15.NONE))
    for f in range(9):
        if np.isfinite(thr[f]):
            margin, count, _, _ = gate_margins(et, dt, [thr[f]], model, sets[f].oracle())
            assert margin[0] >= MARGIN['f64'], (f, thr[f], margin)
            shares.append(count[0] / n_ev)
    assert min(shares) < 0.25 and max(shares) > 0.75, shares
    x, P = _start(model, sets, x0, 'f64')
    r = _run(model, 'f64', et, dt, pay, x, P, thr, consts=sets)
    assert int(np.abs(r['status']).sum()) == 0
    for f in range(9):
        o = _oracle_run(model, sets[f].oracle(), et, dt, pay, x0, thr[f])
        np.testing.assert_array_equal(r['updated'][:, f], o['updated'], err_msg=str(f))
        assert r['n_updated'][f] == o['updated'].sum()
        assert _rel(r['traj'][:, :, f], o['traj']) <= TOL and _rel(r['logdet'][:, f], o['logdet']) <= TOL, f
        assert _rel(r['x'][:, f], o['x']) <= TOL and _rel(ref15.from_blocks(r['P'][:, f]), o['P']) <= TOL, f


def test_columns_differ_by_their_constants():
    """Two columns that differ only in R_gps: the same log-det before the first fix that is
    applied as an update, different from it on."""
    T = 60
    et, dt, pay, x0 = (v.copy() if v.ndim else v for v in _events(300))
    et, dt, pay = et[:T], dt[:T], pay[:T]
    et[0] = ref15.IMU  # the stream's first event is a fix: move the first fix to event `first`
    first = int(np.argmax(et == ref15.GPS))
    assert 3 <= first < T - 3
    base = _sets('ref15')[1]
    other = ref15.ModelConsts('ref15', q=base.q, r_imu=base.r_imu, r_gps=base.r_gps * 3.0, p0=base.p0)
    x, P = _start('ref15', [base, other], x0, 'f64')
    r = _run('ref15', 'f64', et, dt, pay, x, P, None, consts=[base, other])
    ld = r['logdet']
    np.testing.assert_array_equal(ld[:first, 0], ld[:first, 1])
    np.testing.assert_array_equal(r['traj'][:first, :, 0], r['traj'][:first, :, 1])
    assert ld[first, 0] < ld[first, 1]  # the larger R_gps leaves the larger covariance
    # and from there on (the IMU updates between the fixes shrink the gap, every fix renews it)
    fixes = np.nonzero(et == ref15.GPS)[0]
    assert len(fixes) >= 5 and np.all(ld[fixes, 0] < ld[fixes, 1])
    assert np.all(ld[first:, 0] <= ld[first:, 1])


# ---------------------------------------------------------------------------------------------
# failure containment
# ---------------------------------------------------------------------------------------------
def test_bad_constants_poison_one_filter():
    """One column of nine carries an IMU R entry so negative that the innovation covariance of its
    first IMU event has a non-positive pivot (checked on the oracle's S first): KF_ENOTSPD and NaN
    records from that event on for that column, every other column equal to the run without it."""
    et, dt, pay, x0 = _events(300)
    sets = list(_sets('ref15')[:9])
    bad = 3
    good = sets[bad]
    r_imu = good.r_imu.copy()
    r_imu[0] = -1e9
    sets[bad] = ref15.ModelConsts('ref15', q=good.q, r_imu=r_imu, r_gps=good.r_gps, p0=good.p0)
    thr = list(THRESHOLDS[:9])
    thr[bad] = -INF
    # the oracle's S at the first IMU event, after the events before it
    t_imu = int(np.argmax(et == ref15.IMU))
    assert t_imu >= 1 and np.all(et[:t_imu] == ref15.GPS)
    K = sets[bad].oracle()
    Qf, _, Ri, P0 = ref_kf.consts_matrices(K, 15)
    xo, Po = np.zeros(15), P0.copy()
    xo[0:3] = x0[0:3]
    for t in range(t_imu):
        xo, Po = ref_kf.step15(xo, Po, 'GPS', {'easting': pay[t, 0], 'northing': pay[t, 1], 'altitude': pay[t, 2]},
                               dt[t], K)
    F = ref_kf.F_ref15(dt[t_imu])
    S = ref_kf.H_imu15() @ ref_kf.predict_covariance(Po, F, Qf(dt[t_imu])) @ ref_kf.H_imu15().T + Ri
    assert S[0, 0] <= 0.0, S[0, 0]

    x, P = _start('ref15', sets, x0, 'f64')
    r = _run('ref15', 'f64', et, dt, pay, x, P, thr, consts=sets, every=64)
    assert r['status'][bad] == _lib.KF_ENOTSPD
    assert np.isfinite(r['traj'][:t_imu, :, bad]).all() and np.isfinite(r['logdet'][:t_imu, bad]).all()
    assert np.isnan(r['traj'][t_imu:, :, bad]).all() and np.isnan(r['logdet'][t_imu:, bad]).all()
    assert np.isnan(r['x'][:, bad]).all() and np.isnan(r['P'][:, bad]).all() and np.isnan(r['ckpt_x'][:, :, bad]).all()
    keep = [f for f in range(9) if f != bad]
    rest = _run('ref15', 'f64', et, dt, pay, x[:, keep], P[:, keep], [thr[f] for f in keep],
                consts=[sets[f] for f in keep], every=64)
    assert int(np.abs(rest['status']).sum()) == 0
    for j, f in enumerate(keep):
        _assert_equal(_column(r, f), _column(rest, j), msg=str(f))


# ---------------------------------------------------------------------------------------------
# checkpoints and warm starts (kfmi.ref15.ParameterSweep, the façade)
# ---------------------------------------------------------------------------------------------
def _event_list(T):
    """_events(T) as the reference's event list (its first event is a fix at time 0)."""
    et, dt, pay, _ = _events(T)
    t = np.cumsum(dt)
    ev = []
    for i in range(T):
        if et[i] == ref15.NONE:  # an out-of-order event: the drivers skip it (dt < 0)
            ev.append((i, 'IMU', -1.0, ['t', *pay[i]]))
        elif et[i] == ref15.GPS:
            ev.append((i, 'GPS', float(t[i]), {'easting': pay[i, 0], 'northing': pay[i, 1], 'altitude': pay[i, 2]}))
        else:
            ev.append((i, 'IMU', float(t[i]), ['t', *pay[i]]))
    return ev


def test_warm_start_is_the_sweeps_own_state():
    """ParameterSweep with checkpoint_every = 64 over T = 300 events, nine constant sets with their
    own P0 and gates: warm_start(i, e) == the state a parameter sweep over the first e events
    leaves (the sweep's own state after event e - 1), for e on and off a checkpoint and every i;
    result(i) is run_adaptive_threshold_kalman_filter's with consts = set i (another kernel of the
    engine: within the sweep tests' KERNELS)."""
    ev = _event_list(300)
    sets, thr = _sets('ref15')[:9], THRESHOLDS[:9]
    sw = ref15.ParameterSweep(ev, sets, thr, checkpoint_every=64)
    try:
        assert sw._cx.shape == (301 // 64, 15, 9)
        # array entry 0 is the leading NONE record: a prefix of e events is e + 1 entries, so
        # e = 63, 127 end on a checkpoint (no tail) and the others off one
        for e in (1, 2, 63, 64, 100, 127, 128, 255, 299, 300):
            head = ref15.ParameterSweep(ev, sets, thr, end_idx=e, checkpoint_every=0)
            for i in range(9):
                state, P, prev = sw.warm_start(i, e)
                np.testing.assert_array_equal(np.array(state[1:]), _np(head._x[:6, i]), err_msg=f'{e} {i}')
                np.testing.assert_array_equal(P, ref15.from_blocks(_np(head._Pb[:, i])), err_msg=f'{e} {i}')
                assert prev == state[0] == head.result(i)[3]
            head.close()
        ws = sw.warm_starts([2, 5], [100, 128])
        for (i, e), got in zip(((2, 100), (5, 128)), ws):
            want = sw.warm_start(i, e)
            assert got[0] == want[0] and got[2] == want[2]
            np.testing.assert_array_equal(got[1], want[1])
        for i in (0, 5, 8):  # gates that are open throughout (-inf, and -20 below every log-det: no margin to check)
            a = sw.result(i)
            b = ref15.run_adaptive_threshold_kalman_filter(ev, R_threshold=thr[i], consts=sets[i])
            assert a[3] == b[3] and a[4] == b[4] and len(a[0]) == len(b[0])
            assert _rel(a[0], b[0]) <= KERNELS and _rel(a[1], b[1]) <= KERNELS and _rel(a[2], b[2]) <= KERNELS
    finally:
        sw.close()


def test_facade_parameter_sweep():
    """KF_SensorFusion.run_parameter_sweep over its event list is ref15.ParameterSweep; thresholds
    = None runs every set ungated."""
    ev = _event_list(300)
    sf = kfw.KF_SensorFusion.__new__(kfw.KF_SensorFusion)
    sf.indexed_sensor_data, sf.dtype, sf.device = ev, 'f64', 0
    sets = _sets('ref15')[:3]
    a = sf.run_parameter_sweep(sets, end_idx=120, checkpoint_every=0)
    b = ref15.ParameterSweep(ev, sets, [-INF] * 3, end_idx=120, checkpoint_every=0)
    try:
        assert isinstance(a, ref15.ParameterSweep)
        np.testing.assert_array_equal(a.n_updates, b.n_updates)
        assert a.n_updates[0] == int(np.sum(_events(300)[0][:120] != ref15.NONE))
        for i in range(3):
            ra, rb = a.result(i), b.result(i)
            assert ra[0] == rb[0] and ra[1] == rb[1] and ra[4] == rb[4]
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------
def test_argument_errors():
    """KF_EINVAL with its text: a float32 table (the table is float64 for every handle dtype), a
    table of the wrong shape, a list of the wrong length, sets of the other model; and the
    table-size limit R B 8 < 2 GiB at the C ABI, before anything is queued."""
    et, dt, pay, x0 = _events(19)
    sets = _sets('ref15')
    kf = kfmi.BatchedKF('ref15', 4, 'f32')
    try:
        x_in = _np(kf.state()[0])
        thr = np.zeros(4)
        tab = engine.consts_table('ref15', sets[:4])
        for consts, text in ((tab.astype(np.float32), 'dtype torch.float32 != torch.float64'),
                             (torch.from_numpy(tab).float(), 'dtype torch.float32 != torch.float64'),
                             (tab[:, :3], 'shape (33, 3) != expected (33, 4)'),
                             (tab[:18], 'shape (18, 4) != expected (33, 4)'),
                             (sets[:5], '5 constant sets for B = 4 filters'),
                             (_sets('ref8')[:4], "model 'ref8' for a ref15 handle")):
            with pytest.raises(kfmi.KFError) as err:
                kf.run_sweep(et, dt, pay.astype(np.float32), thr, consts=consts)
            assert err.value.code == _lib.KF_EINVAL and text in str(err.value), (text, str(err.value))
        with pytest.raises(ValueError):
            kf.run_sweep(et, dt, pay.astype(np.float32), None)
        with pytest.raises(kfmi.KFError) as err:
            ref15.ParameterSweep(_event_list(19), sets[:4], [0.0] * 3)
        assert err.value.code == _lib.KF_EINVAL and '3 thresholds for 4 constant sets' in str(err.value)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_np(kf.state()[0]), x_in)
    finally:
        kf.close()
    # the smallest f32 ref15 batch whose table reaches 2 GiB (its state span, 27 B 4, is below its limit)
    B = -(-(1 << 31) // (33 * 8))
    big = kfmi.BatchedKF('ref15', B, 'f32')
    try:
        d = big.device
        e, t, p = (torch.as_tensor(v, device=d) for v in (et, dt, pay.astype(np.float32)))
        fake = torch.zeros(8, dtype=torch.float64, device=d)  # never read: the call fails before it queues
        rc = _lib.lib().kf_run_sweep_params(big.handle, 19, e.data_ptr(), t.data_ptr(), p.data_ptr(), None,
                                            fake.data_ptr(), None, None, None, None, 0, None, None, big._stream())
        assert rc == _lib.KF_EINVAL
        assert f'kf_run_sweep_params: B = {B} filters exceed the 2 GiB constants table (33 B 8)' in _lib.last_error()
    finally:
        big.close()
