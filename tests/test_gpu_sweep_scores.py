"""Scored parameter sweep: kf_run_sweep_scores through BatchedKF.run_sweep_scores,
kfmi.ref15.ParameterSweep(scores=True) and the façade — needs an MI355X.

The inputs are tests/test_gpu_param_sweep.py's, imported: its stream, constant sets, start states
and thresholds; the track is the stream's noiseless position with every third row NaN
(tests/score_cases.py).  The filter must be what kf_run_sweep_params runs (==), the scores must
not depend on the neighbours or the records (==), the counts are exact, and the float rows are
judged against tests/score_oracle.py's longdouble truth with the project's budget rule: E_gpu <=
max(8 E_ref, floor), E_ref the plain reference of the handle's precision on the same rounded
inputs, the floor propagated from the per-component floors the state budgets already accept.
"""

import numpy as np
import pytest
import torch

import kfmi
import score_cases as sc
import score_oracle as so
from kfmi import _lib, engine, ref15
from kfmi import kf_workers as kfw
from test_gpu_param_sweep import (ALL, NPD, ORACLE_THR, THRESHOLDS, _assert_equal, _event_list, _events, _run, _sets,
                                  _start)
from test_gpu_sweep import INF, MARGIN, _column, _np, _once, gate_margins

pytestmark = pytest.mark.gpu
LD = so.LD
ROW = engine.SCORE_ROWS
FLOAT_ROWS = so.FLOAT_ROWS
COUNT_ROWS = (0, 3, 6)


def _scored(model, dtype, et, dt, pay, x, P, thresholds, consts, track='own', every=0, records=True):
    """One scored sweep from (x, P): _run's dict plus scores [8, B]."""
    kf = kfmi.BatchedKF(model, x.shape[1], dtype)
    try:
        kf.set_state(np.ascontiguousarray(x), np.ascontiguousarray(P))
        thr = None if thresholds is None else np.asarray(thresholds, np.float64)
        trk = sc.track(len(et)) if isinstance(track, str) else track
        out = kf.run_sweep_scores(et, dt, pay.astype(NPD[dtype]), consts, thr, track=trk, traj=records, logdet=records,
                                  updated=records, checkpoint_every=every)
        xs, Ps = kf.state()
        r = {k: _np(getattr(out, k)) for k in out._fields}
        r.update(x=_np(xs), P=_np(Ps), status=_np(kf.status()))
        return r
    finally:
        kf.close()


def _launch(model, dtype, T=300, B=9, thr='own', records=True):
    """The B-filter scored launch over _events(T) under _sets(model)[:B], cached (never modified)."""
    def run():
        et, dt, pay, x0 = _events(T)
        sets = _sets(model)[:B]
        x, P = _start(model, sets, x0, dtype)
        t = {'own': THRESHOLDS[:B], 'open': None, 'oracle': ORACLE_THR[model][:B]}[thr]
        return _scored(model, dtype, et, dt, pay, x, P, t, sets, records=records)
    return _once(('scored', model, dtype, T, B, thr, records), run)


# ---------------------------------------------------------------------------------------------
# 1. the filter is untouched
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 3, 19, 300])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_filter_is_kf_run_sweep_params(model, dtype, T):
    """Every record, count, checkpoint row, end state and status == run_sweep(consts=...)'s on the
    same inputs, NaNs in the same places (the NaN and +inf thresholds of THRESHOLDS included), for
    B = 1, 8, 9, 17; the same with track = None, and with every record pointer NULL."""
    et, dt, pay, x0 = _events(T)
    every = 64 if T >= 64 else 2
    sets = _sets(model)
    for B in (1, 8, 9, 17):
        x, P = _start(model, sets[:B], x0, dtype)
        want = _run(model, dtype, et, dt, pay, x, P, THRESHOLDS[:B], consts=sets[:B], every=every)
        got = _scored(model, dtype, et, dt, pay, x, P, THRESHOLDS[:B], sets[:B], every=every)
        _assert_equal(got, want, msg=f'B={B}')
        assert got['scores'].shape == (8, B) and got['scores'].dtype == np.float64
        blind = _scored(model, dtype, et, dt, pay, x, P, THRESHOLDS[:B], sets[:B], track=None, every=every)
        _assert_equal(blind, want, msg=f'B={B} no track')
        np.testing.assert_array_equal(blind['scores'][6:], np.zeros((2, B)))
        np.testing.assert_array_equal(blind['scores'][:6], got['scores'][:6])
        bare = _scored(model, dtype, et, dt, pay, x, P, THRESHOLDS[:B], sets[:B], every=every, records=False)
        assert bare['traj'] is None and bare['logdet'] is None and bare['updated'] is None
        _assert_equal(bare, want, keys=('n_updated', 'x', 'P', 'status', 'ckpt_x', 'ckpt_P'), msg=f'B={B} no records')
        np.testing.assert_array_equal(bare['scores'], got['scores'])


# ---------------------------------------------------------------------------------------------
# 2. scores do not depend on the neighbours
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_scores_do_not_depend_on_the_neighbours(model, dtype):
    """Column f of the B = 17 launch == the eight rows of a one-filter launch of set f (another B,
    another place in the wave), with records on and off."""
    et, dt, pay, x0 = _events(300)
    sets = _sets(model)
    full = _launch(model, dtype, B=17)
    np.testing.assert_array_equal(_launch(model, dtype, B=17, records=False)['scores'], full['scores'])
    for f in range(17):
        x, P = _start(model, [sets[f]], x0, dtype)
        one = _scored(model, dtype, et, dt, pay, x, P, [THRESHOLDS[f]], [sets[f]], records=bool(f % 2))
        np.testing.assert_array_equal(one['scores'][:, 0], full['scores'][:, f], err_msg=str(f))


# ---------------------------------------------------------------------------------------------
# 3. counts are exact
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_counts_are_exact(model, dtype):
    et = _events(300)[0]
    r = _launch(model, dtype, B=17)
    s, up = r['scores'], r['updated'].astype(bool)
    np.testing.assert_array_equal(s[ROW['gps_n']], (up & (et == ref15.GPS)[:, None]).sum(0))
    np.testing.assert_array_equal(s[ROW['imu_n']], (up & (et == ref15.IMU)[:, None]).sum(0))
    np.testing.assert_array_equal(s[ROW['gps_n']] + s[ROW['imu_n']], r['n_updated'])
    assert int((et == ref15.NONE).sum()) == 6 and s[ROW['gps_n'], 0] == 35 and s[ROW['imu_n'], 0] == 259
    trk = sc.track(300)
    n_ref = int((~np.isnan(trk[:, :(3 if model == 'ref15' else 2)]).any(1)).sum())
    assert n_ref == 200 and (~np.isnan(trk[et == ref15.NONE]).any(1)).any()  # NONE events are scored too
    np.testing.assert_array_equal(s[ROW['pos_n']], np.full(17, n_ref))
    shut = [f for f, t in enumerate(THRESHOLDS) if t == INF or t != t]
    assert len(shut) == 4
    np.testing.assert_array_equal(s[:6, shut], np.zeros((6, 4)))   # exactly 0: nothing was added
    assert np.all(s[ROW['pos_sse'], shut] > 0) and int(np.abs(r['status']).sum()) == 0


# ---------------------------------------------------------------------------------------------
# 4. pos_sse against its own records
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_pos_sse_is_its_own_trajectorys(model, dtype):
    """pos_sse recomputed from the same launch's traj record in longdouble: |delta| <= (3 pos_n +
    8) 2^-53 sse.  The terms are non-negative, about four roundings each, the sum is double, and the
    f32 positions convert to double exactly, so the bound is the same for both dtypes."""
    r = _launch(model, dtype, B=17)
    k = 3 if model == 'ref15' else 2
    trk = sc.track(300)[:, :k]
    have = ~np.isnan(trk).any(1)
    for f in range(17):
        e = r['traj'][have, :k, f].astype(LD) - trk[have].astype(LD)
        sse = (e * e).sum()
        got = LD(r['scores'][ROW['pos_sse'], f])
        assert abs(got - sse) <= (3 * have.sum() + 8) * LD(2.0) ** -53 * sse, (f, float(got), float(sse))


# ---------------------------------------------------------------------------------------------
# 5, 6. against the truth
# ---------------------------------------------------------------------------------------------
def _judge(model, dtype, r, thr, tag):
    """Rows 1, 2, 4, 5, 7 of every column of launch ``r`` against the truth under ``thr[f]``:
    E_gpu <= max(8 E_ref, floor).  One line per (model, dtype, set, row); returns the worst
    E_gpu / budget."""
    worst = 0.0
    fails = []
    for f in range(r['scores'].shape[1]):
        truth, ref = sc.case(model, dtype, f, thr[f])
        for i in COUNT_ROWS:
            assert r['scores'][i, f] == truth['scores'][i] == ref['scores'][i], (f, so.ROWS[i])
        for i in FLOAT_ROWS:
            e_gpu = float(abs(LD(r['scores'][i, f]) - truth['scores'][i]))
            e_ref = float(abs(LD(ref['scores'][i]) - truth['scores'][i]))
            budget = max(8.0 * e_ref, float(truth['floor'][i]))
            if truth['scores'][i] == 0 and e_gpu == 0:
                continue  # a shut gate's empty sums
            ratio = e_gpu / budget
            print(f'score_budget {tag} {model} {dtype} set {f} {so.ROWS[i]:13s} truth {float(truth["scores"][i]): .9e} '
                  f'E_gpu {e_gpu:.3e} E_ref {e_ref:.3e} E_gpu/E_ref {e_gpu / e_ref if e_ref else float("inf"):9.3g} '
                  f'floor {float(truth["floor"][i]):.3e} budget {budget:.3e} E_gpu/budget {ratio:.3g}')
            worst = max(worst, ratio)
            if not e_gpu <= budget:
                fails.append((f, so.ROWS[i], e_gpu, budget))
    print(f'score_budget {tag} {model} {dtype} worst E_gpu/budget {worst:.3g}')
    assert not fails, fails
    return worst


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_scores_vs_truth_ungated(model, dtype):
    """B = 9, T = 300, thresholds NULL (-inf), every set of _sets(model)[:9]."""
    r = _launch(model, dtype, thr='open')
    assert int(np.abs(r['status']).sum()) == 0
    _judge(model, dtype, r, [-INF] * 9, 'ungated')


@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_scores_vs_truth_gated(model):
    """f64, B = 9, T = 300, ORACLE_THR[model].  First the margin rule, as test_columns_vs_oracle
    asserts it and on the truth's own gate quantity: every finite threshold at least MARGIN from
    logdet(P_pred) over the whole run under that column's constants, none excluded, the shares
    from under 25 % to over 75 %.  Then the flags == the truth's, and the scores as ungated,
    against the truth run under its own flags."""
    et, dt, pay, x0 = _events(300)
    sets, thr = _sets(model)[:9], ORACLE_THR[model]
    n_ev = int(np.sum(et != ref15.NONE))
    shares = []
    for f in range(9):
        if np.isfinite(thr[f]):
            margin, count, _, _ = gate_margins(et, dt, [thr[f]], model, sets[f].oracle())
            assert margin[0] >= MARGIN['f64'], (f, thr[f], margin)
            truth = sc.case(model, 'f64', f, thr[f])[0]
            g = truth['gate'][np.isin(et, (ref15.GPS, ref15.IMU))]
            assert float(np.abs(g - thr[f]).min()) >= MARGIN['f64'], f
            assert count[0] == truth['applied'].sum()
            shares.append(count[0] / n_ev)
    assert min(shares) < 0.25 and max(shares) > 0.75, shares
    r = _launch(model, 'f64', thr='oracle')
    assert int(np.abs(r['status']).sum()) == 0
    for f in range(9):
        np.testing.assert_array_equal(r['updated'][:, f].astype(bool), sc.case(model, 'f64', f, thr[f])[0]['applied'],
                                      err_msg=str(f))
    _judge(model, 'f64', r, thr, 'gated')


# ---------------------------------------------------------------------------------------------
# 7. the aw trap
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_inert_third_state_is_no_part_of_log_det_s(dtype):
    """A ref15 stream of IMU events only, ungated.  An (att, rate) lane's inert third state has
    pivot 1 + 1: counted, it would add 3 log 2 = 2.08 per IMU update to imu_logdet_s.  The row must
    be the truth's to far less: |delta| < 1e-6 n.  For an f32 handle the pivots are float32: 15
    pivots per update at the project's f32 floor of 2^-17 each, |delta| < 15 2^-17 n = 1.1e-4 n."""
    et, dt, pay, x0 = _events(300)
    keep = et == ref15.IMU
    et, dt, pay = et[keep], dt[keep], pay[keep]
    n = int(keep.sum())
    assert n == 259
    c = _sets('ref15')[0]
    x, P = _start('ref15', [c], x0, dtype)
    r = _scored('ref15', dtype, et, dt, pay, x, P, None, [c], track=None)
    xs, Ps = sc.start('ref15', c, x0)
    truth = so.run('ref15', xs, Ps, et, dt, pay, K=c.oracle(), dtype=dtype)
    s = r['scores'][:, 0]
    assert s[ROW['imu_n']] == n == truth['scores'][3] and s[ROW['gps_n']] == 0 and r['status'][0] == 0
    delta = float(abs(LD(s[ROW['imu_logdet_s']]) - truth['scores'][5]))
    print(f'aw trap {dtype}: imu_logdet_s {s[ROW["imu_logdet_s"]]:.9f} truth {float(truth["scores"][5]):.9f} '
          f'delta {delta:.3e} (3 n log 2 = {3 * n * np.log(2):.1f})')
    assert delta < (1e-6 if dtype == 'f64' else 15 * 2.0 ** -17) * n


# ---------------------------------------------------------------------------------------------
# 8. a failed filter
# ---------------------------------------------------------------------------------------------
def test_failed_filter_scores_nan_and_no_neighbour():
    """test_bad_constants_poison_one_filter's case: column 3's IMU R makes its first IMU event's
    pivot non-positive.  Its status is KF_ENOTSPD, its float rows NaN, its counts finite; its
    neighbours' eight rows == those of a launch without that column."""
    et, dt, pay, x0 = _events(300)
    sets = list(_sets('ref15')[:9])
    bad = 3
    good = sets[bad]
    r_imu = good.r_imu.copy()
    r_imu[0] = -1e9
    sets[bad] = ref15.ModelConsts('ref15', q=good.q, r_imu=r_imu, r_gps=good.r_gps, p0=good.p0)
    thr = list(THRESHOLDS[:9])
    thr[bad] = -INF
    x, P = _start('ref15', sets, x0, 'f64')
    r = _scored('ref15', 'f64', et, dt, pay, x, P, thr, sets, every=64)
    assert r['status'][bad] == _lib.KF_ENOTSPD
    s = r['scores'][:, bad]
    assert np.isnan(s[list(FLOAT_ROWS)]).all()
    assert s[ROW['gps_n']] == 35 and s[ROW['imu_n']] == 259 and s[ROW['pos_n']] == 200
    keep = [f for f in range(9) if f != bad]
    rest = _scored('ref15', 'f64', et, dt, pay, x[:, keep], P[:, keep], [thr[f] for f in keep],
                   [sets[f] for f in keep], every=64)
    assert int(np.abs(rest['status']).sum()) == 0 and np.isfinite(rest['scores']).all()
    np.testing.assert_array_equal(r['scores'][:, keep], rest['scores'])
    for j, f in enumerate(keep):
        _assert_equal(_column(r, f), _column(rest, j), keys=ALL, msg=str(f))


# ---------------------------------------------------------------------------------------------
# 9. the Python layer
# ---------------------------------------------------------------------------------------------
def _facade(ev):
    sf = kfw.KF_SensorFusion.__new__(kfw.KF_SensorFusion)
    sf.indexed_sensor_data, sf.dtype, sf.device = ev, 'f64', 0
    return sf


def test_parameter_sweep_ranks_without_records():
    """ParameterSweep(scores=True, records=False) over the T = 300 event list, the track the list's
    own fixes: scores['pos_rmse'][i] against the façade's calculate_accuracy_metrics of
    result(i)'s states from a records=True twin, relative 1e-9.  The gap is the summation order plus
    the two interpolations' fp64 rounding (interp1d's formula in track_positions against SciPy's
    own): measured 3.6e-16 at the worst of the nine sets.  best() is the argmin over the finite values; the
    façade passes scores and track through; AdaptiveSweep scores its one set in every column."""
    ev = _event_list(300)
    sets, thr = _sets('ref15')[:9], THRESHOLDS[:9]
    sw = ref15.ParameterSweep(ev, sets, thr, checkpoint_every=64, scores=True, records=False)
    twin = ref15.ParameterSweep(ev, sets, thr, checkpoint_every=64)
    sf = _facade(ev)
    sf._ground_truth = [(t, sd['easting'], sd['northing'], sd['altitude']) for _, ty, t, sd in ev if ty == 'GPS']
    try:
        assert twin.scores is None and set(sw.scores) == {
            'gps_n', 'gps_nis', 'gps_logdet_s', 'gps_nll', 'imu_n', 'imu_nis', 'imu_logdet_s', 'imu_nll', 'pos_n',
            'pos_rmse'}
        assert all(v.shape == (9,) and v.dtype == np.float64 for v in sw.scores.values())
        np.testing.assert_array_equal(sw.n_updates, twin.n_updates)
        np.testing.assert_array_equal(sw.scores['gps_n'] + sw.scores['imu_n'], twin.n_updates)
        np.testing.assert_array_equal(_np(sw._x), _np(twin._x))
        with pytest.raises(ValueError):
            sw.result(0)
        gap = 0.0
        for i in range(9):
            states = twin.result(i)[0]
            assert sw.scores['pos_n'][i] == len(states) == 1 + 300 - 6   # the leading NONE entry; not the skipped
            want = sf.calculate_accuracy_metrics(states)['total_position_rmse']
            gap = max(gap, abs(sw.scores['pos_rmse'][i] - want) / want)
        print(f'pos_rmse against calculate_accuracy_metrics: worst relative gap {gap:.3e}')
        assert gap <= 1e-9
        for by in ('gps_nll', 'pos_rmse', 'imu_nll'):
            v = sw.scores[by]
            assert np.isfinite(v).any() and sw.best(by) == int(np.nanargmin(np.where(np.isfinite(v), v, np.nan)))
        np.testing.assert_array_equal(sw.scores['gps_nll'],
                                      0.5 * (sw.scores['gps_nis'] + sw.scores['gps_logdet_s'] +
                                             sw.scores['gps_n'] * 3 * np.log(2 * np.pi)))
        assert sw.best() == sw.best('gps_nll')
        a = sf.run_parameter_sweep(sets, thr, checkpoint_every=64, scores=True, records=False)
        for k in sw.scores:
            np.testing.assert_array_equal(a.scores[k], sw.scores[k], err_msg=k)
        a.close()
        # another track: a (times, positions) pair shifted by 1 m in x moves the error
        tt = np.array([t for _, ty, t, _ in ev if ty == 'GPS'])
        tp = np.array([[sd['easting'], sd['northing'], sd['altitude']] for _, ty, _, sd in ev if ty == 'GPS'])
        b = ref15.ParameterSweep(ev, sets[:2], None, scores=True, records=False, track=(tt, tp + [1.0, 0, 0]))
        assert np.all(b.scores['pos_rmse'] != sw.scores['pos_rmse'][:2]) and np.all(b.scores['imu_n'] == 259)
        b.close()
        one = ref15.AdaptiveSweep(ev, [thr[1], thr[1]], consts=sets[1], scores=True, records=False)
        for k in sw.scores:
            np.testing.assert_array_equal(one.scores[k], np.repeat(sw.scores[k][1], 2), err_msg=k)
        one.close()
    finally:
        sw.close()
        twin.close()


def test_argument_errors():
    """NULL consts and NULL scores at the C ABI, a wrong table shape and a wrong track shape or
    dtype in Python: KF_EINVAL with its text, nothing run."""
    et, dt, pay, x0 = _events(19)
    sets = _sets('ref15')[:4]
    kf = kfmi.BatchedKF('ref15', 4, 'f64')
    try:
        x_in = _np(kf.state()[0])
        d = kf.device
        a = [torch.as_tensor(v, device=d) for v in (et, dt, pay)]
        tab = torch.from_numpy(engine.consts_table('ref15', sets)).to(d)
        out = torch.full((8, 4), 7.0, dtype=torch.float64, device=d)
        L = _lib.lib()
        rc = L.kf_run_sweep_scores(kf.handle, 19, *(v.data_ptr() for v in a), None, None, None, out.data_ptr(), None,
                                   None, None, None, 0, None, None, kf._stream())
        assert rc == _lib.KF_EINVAL and 'kf_run_sweep_scores: null consts' in _lib.last_error()
        rc = L.kf_run_sweep_scores(kf.handle, 19, *(v.data_ptr() for v in a), None, tab.data_ptr(), None, None, None,
                                   None, None, None, 0, None, None, kf._stream())
        assert rc == _lib.KF_EINVAL and 'kf_run_sweep_scores: null scores' in _lib.last_error()
        with pytest.raises(kfmi.KFError) as err:
            kf.run_sweep_scores(et, dt, pay, None)
        assert err.value.code == _lib.KF_EINVAL and 'consts is mandatory' in str(err.value)
        for consts, track, text in ((_np(tab)[:, :3], None, 'shape (33, 3) != expected (33, 4)'),
                                    (_np(tab)[:18], None, 'shape (18, 4) != expected (33, 4)'),
                                    (sets, np.zeros((19, 2)), 'track: expected a float64 [T, 3] = (19, 3)'),
                                    (sets, np.zeros((18, 3)), 'track: expected a float64 [T, 3] = (19, 3)'),
                                    (sets, np.zeros((19, 3), np.float32), 'track: expected a float64 [T, 3] = (19, 3)')):
            with pytest.raises(kfmi.KFError) as err:
                kf.run_sweep_scores(et, dt, pay, consts, track=track)
            assert err.value.code == _lib.KF_EINVAL and text in str(err.value), (text, str(err.value))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_np(kf.state()[0]), x_in)
        np.testing.assert_array_equal(_np(out), np.full((8, 4), 7.0))
        # T = 0: nothing runs, the rows are zeroed
        rc = L.kf_run_sweep_scores(kf.handle, 0, None, None, None, None, tab.data_ptr(), None, out.data_ptr(), None, None,
                                   None, None, 0, None, None, kf._stream())
        assert rc == _lib.KF_OK, _lib.last_error()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_np(out), np.zeros((8, 4)))
    finally:
        kf.close()
