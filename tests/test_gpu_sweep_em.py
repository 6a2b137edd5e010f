"""kf_smooth_sweep_em (BatchedKF.smooth_sweep_em, kfmi.ref_em_update, AdaptiveSweep / ParameterSweep(
em=True), ref15.fit_noise): the EM statistics for the diagonals of Q, R_imu and R_gps gathered by the
reference models' smoother — needs an MI355X.

Accuracy is judged by the project's rule: per row group (Q, R_imu, R_gps), the worst relative error
against the longdouble truth of tests/sweep_em_oracle.py within extended_oracle.budget(E_ref, 'f64')
(8 x E_ref, floor 2^-40), E_ref the plain float64 textbook (lag-one) leg's own error on the same
inputs.  The streams, constant sets and thresholds are tests/test_gpu_smoother.py's (through
tests/sweep_em_cases.py).  Everything that should be the same bits is compared with ==.

Measured on an MI355X (each test prints its figures with -s; profiles/sweep_em/em_budget.log), the
worst E_gpu / budget over the cases of each test (the Q rows' E_ref, the lag-one form, is 1e-13 ..
4e-12 where the kernel's gain form is at 1e-15 .. 1e-14):
  E-step, end to end           Q 0.0045, R_imu 0.154,  R_gps 0.187
  E-step, backward pass alone  Q 0.0045, R_imu 0.176,  R_gps 0.253
  E-step, typed stream         Q 0.0053, R_imu 0.165,  R_gps 0.275
  EM loop, tables              Q 0.0001, R_imu 0.0022, R_gps 0.148;  NLL 0.0025
"""
import itertools

import numpy as np
import pytest
import torch

import kfmi
import sweep_em_cases as cases
import sweep_em_oracle as seo
from kfmi import _lib, engine, ref15
from sweep_em_cases import COLUMNS, GATE_MARGIN, MODELS, THR, T
from test_gpu_param_sweep import _events, _sets, _start
from test_gpu_smoother import _assert_same, _forward, _smooth
from test_gpu_sweep import INF, _golden, _np

pytestmark = pytest.mark.gpu
SENTINEL = -777.25
BS = (1, 7, 8, 9, 17)
TS = (1, 2, 4, 5, 6, 17)        # around both ring depths (2 and 4)
OUT = ('x', 'P', 'traj', 'logdet')


def _ptr(t):
    return None if t is None else t.data_ptr()


def _em(model, et, dt, pay, up, fx, fP, consts=None, params=None, kf=None, **kw):
    """smooth_sweep_em on a fresh (or the given) handle; every output by default.  NumPy dict."""
    kw = {**dict(x=True, P=True, traj=True, logdet=True), **kw}
    own = kf is None
    if own:
        kf = kfmi.BatchedKF(model, fx.shape[2], 'f64', params=params)
    try:
        sm = kf.smooth_sweep_em(et, dt, pay, up, fx, fP, consts=consts, **kw)
        return {k: _np(v) for k, v in sm._asdict().items()}
    finally:
        if own:
            kf.close()


def _counts(et, dt, up):
    """[3, B]: N_TRANS, N_IMU, N_GPS from the stream and the flags, in NumPy."""
    later = (np.arange(len(et)) >= 1)[:, None]
    up = up.astype(bool)
    n_tr = np.sum(later & ((et != ref15.NONE) & (dt != 0))[:, None], axis=0) * np.ones(up.shape[1], int)
    n_imu = np.sum(later & up & (et == ref15.IMU)[:, None], axis=0)
    n_gps = np.sum(later & up & (et == ref15.GPS)[:, None], axis=0)
    return np.stack([n_tr, n_imu, n_gps]).astype(np.float64)


def _count_rows(model):
    r = engine.ref_em_rows(model)
    return [r['n_trans'], r['n_imu'], r['n_gps']]


def _float_rows(model):
    return sorted(sum(seo.float_rows(model).values(), []))


def _edge_events(Tn):
    """_events(19) with NONE events at 3 and 6, a PREDICT event at 8 and dt = 0 at 2 and 10."""
    et, dt, pay, x0 = _events(19)
    et, dt = et.copy(), dt.copy()
    et[[3, 6]] = ref15.NONE
    et[8] = ref15.PREDICT
    dt[[2, 10]] = 0.0
    return et[:Tn], dt[:Tn], pay[:Tn], x0


# ---------------------------------------------------------------------------------------------
# 1. bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', MODELS)
def test_edges_bit_for_bit(model):
    """T = 1, 2, 4, 5, 6, 17 (around both ring depths) on a stream with NONE, PREDICT and dt = 0
    events, thresholds -inf / -10 / 5 cycled over 17 columns of custom constants.  At every T and B =
    1, 7, 8, 9, 17: the sm_* outputs are kf_smooth_sweep's, column f == filter f run alone, the counts
    are NumPy's on etype / dt / updated (event 0's applied fix is not in them).  At every T, B = 9: em
    is the same with every subset of the outputs NULL and in place; payload / updated NULL leaves the
    Q rows and N_TRANS what they were and the R blocks 0; a table column holding set c == a handle
    allocated with params = c and consts = NULL."""
    sets = _sets(model)[:17]
    thr = [THR[f % 3] for f in range(17)]
    rows = engine.ref_em_rows(model)
    cr, fr = _count_rows(model), _float_rows(model)
    handles = {B: kfmi.BatchedKF(model, B, 'f64') for B in BS}
    try:
        for Tn in TS:
            et, dt, pay, x0 = _edge_events(Tn)
            x, P = _start(model, sets, x0, 'f64')
            fx, fP, up = _forward(model, et, dt, pay, x, P, thr, consts=sets)
            assert et[0] == ref15.GPS and up[0].any()                 # event 0 is a fix, applied, and not counted below
            solo = [_em(model, et, dt, pay, up[:, f:f + 1], fx[:, :, f:f + 1].contiguous(), fP[:, :, f:f + 1].contiguous(),
                        consts=sets[f:f + 1], kf=handles[1]) for f in range(17)]
            for B in BS:
                rx, rP, ru = fx[:, :, :B].contiguous(), fP[:, :, :B].contiguous(), np.ascontiguousarray(up[:, :B])
                got = _em(model, et, dt, pay, ru, rx, rP, consts=sets[:B], kf=handles[B])
                assert got['em'].shape == (rows['rows'], B) and np.all(got['status'] == 0)
                _assert_same(got, _smooth(model, et, dt, rx, rP, consts=sets[:B], kf=handles[B]), msg=f'T={Tn} B={B}')
                for f in range(B):
                    _assert_same({k: v[..., f:f + 1] for k, v in got.items()}, solo[f],
                                 keys=OUT + ('status', 'em'), msg=f'T={Tn} B={B} f={f}')
                np.testing.assert_array_equal(got['em'][cr], _counts(et, dt, ru), err_msg=f'counts T={Tn} B={B}')
                if Tn == 1:
                    assert not got['em'].any()
                else:
                    assert np.all(got['em'][fr][:, :] >= 0) and np.all(np.isfinite(got['em']))
                if Tn == 17:
                    assert np.all(got['em'][rows['q']:rows['q'] + 3] > 0)
                if B != 9:
                    continue
                for keep in itertools.product((False, True), repeat=4):
                    for status in ((True, False) if not any(keep) else (True,)):
                        one = _em(model, et, dt, pay, ru, rx, rP, consts=sets[:B], kf=handles[B], status=status,
                                  **dict(zip(OUT, keep)))
                        assert all((one[k] is not None) == on for k, on in zip(OUT, keep))
                        assert (one['status'] is not None) == status
                        np.testing.assert_array_equal(one['em'], got['em'], err_msg=f'outputs {keep} T={Tn}')
                        _assert_same(one, got, keys=[k for k, on in zip(OUT, keep) if on], msg=f'outputs {keep} T={Tn}')
                ix, iP = rx.clone(), rP.clone()
                inp = _em(model, et, dt, pay, ru, ix, iP, consts=sets[:B], kf=handles[B], inplace=True)
                _assert_same(inp, got, keys=OUT + ('status', 'em'), msg=f'in place T={Tn}')
                np.testing.assert_array_equal(_np(ix), got['x'])
                np.testing.assert_array_equal(_np(iP), got['P'])
                bare = _em(model, et, dt, None, None, rx, rP, consts=sets[:B], kf=handles[B])
                _assert_same(bare, got, keys=OUT + ('status',), msg=f'no measurements T={Tn}')
                q_rows = [rows['n_trans']] + seo.float_rows(model)['q']
                np.testing.assert_array_equal(bare['em'][q_rows], got['em'][q_rows])
                assert not bare['em'][rows['n_imu']:].any()
                for f in (0, 1, 2):   # set 0 is the reference's: the literals
                    assert (sets[f].params() is None) == (f == 0)
                    own = _em(model, et, dt, pay, up[:, f:f + 1], fx[:, :, f:f + 1].contiguous(),
                              fP[:, :, f:f + 1].contiguous(), params=sets[f].params())
                    _assert_same(own, solo[f], keys=OUT + ('status', 'em'), msg=f'handle constants T={Tn} f={f}')
    finally:
        for kf in handles.values():
            kf.close()


@pytest.mark.parametrize('model', MODELS)
def test_event_types_counts(model):
    """test_gpu_smoother.py's "typed" stream (PREDICT events, dt = 0 events after event 0, the
    stream's own NONE events), T = 300: the counts are NumPy's, and they are what the truth counted."""
    et, dt, pay, x0 = cases.STREAMS['typed']()
    sets = _sets(model)
    cols = [(0, -INF), (0, 5.0), (1, -INF), (1, 5.0)]
    tab = [sets[ci] for ci, _ in cols]
    x, P = _start(model, tab, x0, 'f64')
    fx, fP, up = _forward(model, et, dt, pay, x, P, [thr for _, thr in cols], consts=tab)
    got = _em(model, et, dt, pay, up, fx, fP, consts=tab, x=False, P=False, traj=False, logdet=False)
    assert np.all(got['status'] == 0)
    np.testing.assert_array_equal(got['em'][_count_rows(model)], _counts(et, dt, up))
    for f, (ci, thr) in enumerate(cols):
        c = cases.estep_truth(model, ci, thr, 'typed')
        np.testing.assert_array_equal(up[:, f].astype(bool), c['truth']['applied'])
        np.testing.assert_array_equal(got['em'][_count_rows(model), f], c['em'][_count_rows(model)].astype(np.float64))
        _judge(model, got['em'][:, f], c, f'{model} typed stream, set {ci} thr {thr}')
    assert got['em'][0, 0] < np.sum(et[1:] != ref15.NONE)


# ---------------------------------------------------------------------------------------------
# 2. against the truth
# ---------------------------------------------------------------------------------------------
def _judge(model, em, c, label):
    """One column of em against the truth of its case, per row group, within the budget."""
    e_ref = seo.em_errors(c['em_ref'], c['em'], model)
    bud = cases.budget(e_ref)
    e = seo.em_errors(em, c['em'], model)
    print(label, ' '.join(f'{k} {e[k]:.1e}/{bud[k]:.1e} = {e[k] / bud[k]:.3f} (E_ref {e_ref[k]:.1e})' for k in bud))
    for k in bud:
        assert e[k] <= bud[k], (label, k, e[k], bud[k], e_ref[k])
    cr = _count_rows(model)
    np.testing.assert_array_equal(np.asarray(em)[cr], c['em'][cr].astype(np.float64), err_msg=label)


def _check_gates(truth, thr, updated=None):
    if np.isfinite(thr):
        g = truth['gate'][~np.isnan(truth['gate'].astype(np.float64))]
        assert float(np.min(np.abs(g - thr))) >= GATE_MARGIN
    if updated is not None:
        np.testing.assert_array_equal(updated.astype(bool), truth['applied'])


@pytest.mark.parametrize('model', MODELS)
def test_end_to_end(model):
    """run_sweep(checkpoint_every=1) -> smooth_sweep_em, T = 300: column 0's constants on a plain
    handle with consts = NULL, and two custom sets through the table, each under the three
    thresholds; the device applied exactly the truth's updates, and every row group of every filter is
    within the budget."""
    et, dt, pay, x0 = _events(T)
    sets = _sets(model)
    x, P = _start(model, [sets[0]] * 3, x0, 'f64')
    fx, fP, up = _forward(model, et, dt, pay, x, P, THR)
    got = _em(model, et, dt, pay, up, fx, fP, x=False, P=False, traj=False, logdet=False)
    assert np.all(got['status'] == 0)
    for f, thr in enumerate(THR):
        c = cases.estep_truth(model, 0, thr)
        _check_gates(c['truth'], thr, up[:, f])
        _judge(model, got['em'][:, f], c, f'{model} set 0 thr {thr}')
    cols = [(ci, thr) for ci in COLUMNS[1:] for thr in THR]
    tab = [sets[ci] for ci, _ in cols]
    x, P = _start(model, tab, x0, 'f64')
    fx, fP, up = _forward(model, et, dt, pay, x, P, [thr for _, thr in cols], consts=tab)
    got = _em(model, et, dt, pay, up, fx, fP, consts=tab, x=False, P=False, traj=False, logdet=False)
    assert np.all(got['status'] == 0)
    for f, (ci, thr) in enumerate(cols):
        c = cases.estep_truth(model, ci, thr)
        _check_gates(c['truth'], thr, up[:, f])
        _judge(model, got['em'][:, f], c, f'{model} set {ci} thr {thr}')


@pytest.mark.parametrize('model', MODELS)
def test_backward_pass_alone(model):
    """No forward launch: the record is the truth's filtered record rounded to f64 and the flags the
    truth's applied updates; the handle gives the model only and the table the constants."""
    et, dt, pay, x0 = _events(T)
    sets = _sets(model)
    cols = [(ci, thr) for ci in COLUMNS for thr in THR]
    tr = [cases.estep_truth(model, ci, thr) for ci, thr in cols]
    fx = np.stack([c['truth']['xf'].astype(np.float64) for c in tr], 2)
    fP = np.stack([ref15.to_blocks(c['truth']['Pf'].astype(np.float64)) for c in tr], 2)
    up = np.stack([c['truth']['applied'] for c in tr], 1).astype(np.uint8)
    got = _em(model, et, dt, pay, np.ascontiguousarray(up), np.ascontiguousarray(fx), np.ascontiguousarray(fP),
              consts=[sets[ci] for ci, _ in cols], x=False, P=False, traj=False, logdet=False)
    assert np.all(got['status'] == 0)
    for f, (ci, thr) in enumerate(cols):
        _check_gates(tr[f]['truth'], thr)
        _judge(model, got['em'][:, f], tr[f], f'{model} backward only, set {ci} thr {thr}')


# ---------------------------------------------------------------------------------------------
# 3. the EM loop
# ---------------------------------------------------------------------------------------------
def _device_loop(model, et, dt, pay, x, P, thr, tab, iters, imu_rows):
    """fit_noise's loop on engine calls: (tables [iters + 1, R, B], nll [iters + 1, B], updated per
    iteration)."""
    B = x.shape[1]
    tabs, nlls, ups = [tab], [], []
    with kfmi.BatchedKF(model, B, 'f64') as kf:
        def forward(tab, record):
            kf.set_state(np.ascontiguousarray(x), np.ascontiguousarray(P))
            r = kf.run_sweep_scores(et, dt, pay, tab, np.asarray(thr, np.float64), updated=True,
                                    checkpoint_every=1 if record else 0)
            nlls.append(_np(kfmi.innovation_nll(r.scores, model, 'gps') + kfmi.innovation_nll(r.scores, model, 'imu')))
            ups.append(_np(r.updated))
            assert np.all(_np(kf.status()) == 0)
            return r
        for _ in range(iters):
            r = forward(tab, True)
            sm = kf.smooth_sweep_em(et, dt, pay, r.updated, r.ckpt_x, r.ckpt_P, consts=tab, x=True, P=True, inplace=True)
            assert np.all(_np(sm.status) == 0)
            tab = _np(kfmi.ref_em_update(sm.em, torch.as_tensor(tab).to(sm.em.device), model, imu_rows))
            tabs.append(tab)
        forward(tab, False)
    return np.stack(tabs), np.stack(nlls), ups


@pytest.mark.parametrize('imu_rows', cases.LOOP_IMU_ROWS)
@pytest.mark.parametrize('model', MODELS)
def test_em_loop(model, imu_rows):
    """LOOP_ITERS iterations of forward sweep, smooth_sweep_em in place and ref_em_update against
    sweep_em_oracle.em_loop in longdouble, ungated and under the case's finite threshold: at every
    iteration the device applied the truth's updates; the tables per row group and the NLL within the
    budget that the plain float64 loop's own error sets.  No monotonicity is asserted."""
    et, dt, pay, x0 = cases.loop_events()
    thr = cases.LOOP_THR[model]
    c = _sets(model)[cases.LOOP_SET]
    x, P = _start(model, [c] * len(thr), x0, 'f64')
    tab0 = engine.consts_table(model, [c] * len(thr))
    tabs, nll, ups = _device_loop(model, et, dt, pay, x, P, thr, tab0, cases.LOOP_ITERS, imu_rows)
    for f, th in enumerate(thr):
        truth, plain = cases.loop_truth(model, th, imu_rows)
        assert np.all(truth['margin'] >= GATE_MARGIN)
        for it in range(cases.LOOP_ITERS + 1):
            np.testing.assert_array_equal(ups[it][:, f].astype(bool), truth['applied'][it], err_msg=f'iteration {it}')
        e_ref = seo.table_errors(plain['tables'][1:], truth['tables'][1:], model)
        e = seo.table_errors(tabs[1:, :, f], truth['tables'][1:], model)
        tn = truth['nll'].astype(seo.LD)
        e_ref['nll'] = float(np.max(np.abs(plain['nll'].astype(seo.LD) - tn) / np.abs(tn)))
        e['nll'] = float(np.max(np.abs(nll[:, f].astype(seo.LD) - tn) / np.abs(tn)))
        bud = cases.budget(e_ref)
        print(f'{model} loop thr {th} {imu_rows}:',
              ' '.join(f'{k} {e[k]:.1e}/{bud[k]:.1e} = {e[k] / bud[k]:.3f} (E_ref {e_ref[k]:.1e})' for k in bud),
              '| nll', ' '.join(f'{v:.6g}' for v in nll[:, f]))
        np.testing.assert_array_equal(tabs[0, :, f], truth['tables'][0].astype(np.float64))
        for k in bud:
            assert e[k] <= bud[k], (model, th, imu_rows, k, e[k], bud[k], e_ref[k])
        n = seo.dims(model)[0]
        rest = [n + i for i in range(n) if i not in seo.IMU_MEASURED[model]]
        if imu_rows == 'measured':                                   # position and velocity rows of R_imu are kept
            assert np.all(tabs[:, rest, f] == tabs[0, rest, f])
        else:
            assert np.all(tabs[-1, rest, f] != tabs[0, rest, f])


# ---------------------------------------------------------------------------------------------
# 4. failure isolation (by data, not by a fault)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', MODELS)
def test_failure_is_isolated(model):
    """A NaN in one entry of filt_P at row r of one column: that column's float rows are NaN, its
    counts what they were, its status KF_ENOTSPD; every other column and status bit for bit."""
    et, dt, pay, x0 = cases.loop_events()
    sets = _sets(model)[:9]
    x, P = _start(model, sets, x0, 'f64')
    fx, fP, up = _forward(model, et, dt, pay, x, P, [THR[f % 3] for f in range(9)], consts=sets)
    clean = _em(model, et, dt, pay, up, fx, fP, consts=sets)
    assert np.all(clean['status'] == 0) and np.all(np.isfinite(clean['em']))
    r, col = 60, 4
    bad_P = fP.clone()
    bad_P[r, 7, col] = float('nan')
    bad = _em(model, et, dt, pay, up, fx, bad_P, consts=sets)
    others = [f for f in range(9) if f != col]
    cr, fr = _count_rows(model), _float_rows(model)
    assert np.isnan(bad['em'][fr, col]).all()
    np.testing.assert_array_equal(bad['em'][cr, col], clean['em'][cr, col])
    np.testing.assert_array_equal(bad['em'][:, others], clean['em'][:, others])
    for k in OUT:
        assert np.isnan(bad[k][:r + 1, ..., col]).all(), k
        np.testing.assert_array_equal(bad[k][r + 1:, ..., col], clean[k][r + 1:, ..., col], err_msg=k)
        np.testing.assert_array_equal(bad[k][..., others], clean[k][..., others], err_msg=k)
    assert bad['status'][col] == _lib.KF_ENOTSPD and np.all(bad['status'][others] == 0)


# ---------------------------------------------------------------------------------------------
# 5. refusals, T = 0, graph capture
# ---------------------------------------------------------------------------------------------
def _raw(kf, Tn, n, rows_P, em_rows, payload=True, updated=True, filt_x=True, filt_P=True):
    """kf_smooth_sweep_em with sentinel-filled outputs: (rc, outputs)."""
    B, d, k = kf.batch, 'cuda', max(Tn, 1)
    td = kf.torch_dtype
    et = torch.full((k,), ref15.IMU, dtype=torch.uint8, device=d)
    dts = torch.full((k,), 0.01, dtype=torch.float64, device=d)
    pay = torch.zeros(k, 9, dtype=td, device=d) if payload else None
    up = torch.ones(k, B, dtype=torch.uint8, device=d) if updated else None
    fx = torch.zeros(k, n, B, dtype=td, device=d) if filt_x else None
    fP = torch.ones(k, rows_P, B, dtype=td, device=d) if filt_P else None
    outs = [torch.full((k, n, B), SENTINEL, dtype=td, device=d), torch.full((k, rows_P, B), SENTINEL, dtype=td, device=d),
            torch.full((k, 6, B), SENTINEL, dtype=td, device=d), torch.full((k, B), SENTINEL, dtype=td, device=d),
            torch.full((B,), 55, dtype=torch.int32, device=d),
            torch.full((em_rows, B), SENTINEL, dtype=torch.float64, device=d)]
    rc = _lib.lib().kf_smooth_sweep_em(kf.handle, Tn, _ptr(et), _ptr(dts), _ptr(pay), _ptr(up), None, _ptr(fx), _ptr(fP),
                                       *[_ptr(o) for o in outs], kf._stream())
    torch.cuda.synchronize()
    return rc, outs


def _untouched(outs):
    return all(bool((o == (55 if o.dtype == torch.int32 else SENTINEL)).all()) for o in outs)


@pytest.mark.parametrize('why', ['f32', 'cv_handle', 'payload_alone', 'updated_alone', 'null_filt_x', 'null_filt_P',
                                 'negative_T'])
def test_refusals(why):
    model, dtype = ('cv3', 'f64') if why == 'cv_handle' else ('ref15', 'f32' if why == 'f32' else 'f64')
    kw = dict(payload_alone=dict(updated=False), updated_alone=dict(payload=False), null_filt_x=dict(filt_x=False),
              null_filt_P=dict(filt_P=False)).get(why, {})
    with kfmi.BatchedKF(model, 9, dtype) as kf:
        rc, outs = _raw(kf, -1 if why == 'negative_T' else 5, 15, 27, 36, **kw)
        assert rc == _lib.KF_EINVAL and 'kf_smooth_sweep_em' in _lib.last_error(), _lib.last_error()
        assert _untouched(outs)
        if why == 'f32':
            with pytest.raises(kfmi.KFError) as e:
                kf.smooth_sweep_em(np.zeros(5, np.uint8), np.zeros(5), None, None, np.zeros((5, 15, 9), np.float32),
                                   np.zeros((5, 27, 9), np.float32))
            assert e.value.code == _lib.KF_EINVAL
    if why == 'payload_alone':
        with kfmi.BatchedKF('ref15', 9, 'f64') as kf, pytest.raises(kfmi.KFError) as e:
            kf.smooth_sweep_em(np.zeros(5, np.uint8), np.zeros(5), np.zeros((5, 9)), None, np.zeros((5, 15, 9)),
                               np.zeros((5, 27, 9)))
        assert e.value.code == _lib.KF_EINVAL


@pytest.mark.parametrize('model', MODELS)
def test_T0_zeroes_the_table_and_the_handle_is_not_touched(model):
    n, rows_P = (15, 27) if model == 'ref15' else (8, 15)
    with kfmi.BatchedKF(model, 65, 'f64') as kf:
        before = [_np(t) for t in kf.state()] + [_np(kf.status())]
        rc, outs = _raw(kf, 0, n, rows_P, engine.em_rows(model))
        assert rc == _lib.KF_OK, _lib.last_error()
        assert not _np(outs[5]).any() and _untouched(outs[:5])
        rc, outs = _raw(kf, 1, n, rows_P, engine.em_rows(model))          # T = 1: no step, all zero
        assert rc == _lib.KF_OK and not _np(outs[5]).any() and not _untouched(outs[:1])
        rc, outs = _raw(kf, 5, n, rows_P, engine.em_rows(model))
        assert rc == _lib.KF_OK and not any(bool((o == SENTINEL).any()) for o in (outs[0], outs[1], outs[5]))
        assert np.all(_np(outs[5])[_count_rows(model)] == np.array([[4.0], [4.0], [0.0]]))
        after = [_np(t) for t in kf.state()] + [_np(kf.status())]
        assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_graph_capture_replays_the_eager_bits():
    """kf_set_state + kf_run_sweep_scores + kf_smooth_sweep_em captured into one graph (nothing
    allocates or synchronises) and replayed twice == the eager calls."""
    model, Tn, B = 'ref15', 17, 17
    et, dt, pay, x0 = _edge_events(Tn)
    sets = _sets(model)[:B]
    thr = np.array([THR[f % 3] for f in range(B)])
    x, P = _start(model, sets, x0, 'f64')
    fx, fP, up = _forward(model, et, dt, pay, x, P, thr, consts=sets)
    eager = _em(model, et, dt, pay, up, fx, fP, consts=sets)
    d = 'cuda'
    kf = kfmi.BatchedKF(model, B, 'f64')
    dev = [torch.as_tensor(np.ascontiguousarray(a), device=d) for a in (et, dt, pay, thr, engine.consts_table(model, sets),
                                                                        x, P)]
    d_et, d_dt, d_pay, d_thr, d_tab, d_x, d_P = dev
    cx, cP = kf.empty(Tn, 15, B), kf.empty(Tn, 27, B)
    d_up = torch.empty(Tn, B, dtype=torch.uint8, device=d)
    sc = torch.empty(8, B, dtype=torch.float64, device=d)
    sx, sP, st_, sl = kf.empty(Tn, 15, B), kf.empty(Tn, 27, B), kf.empty(Tn, 6, B), kf.empty(Tn, B)
    em = torch.empty(36, B, dtype=torch.float64, device=d)
    st = torch.full((B,), 55, dtype=torch.int32, device=d)
    L = _lib.lib()

    def calls():
        s = kf._stream()
        _lib.check(L.kf_set_state(kf.handle, _ptr(d_x), _ptr(d_P), 1, s))
        _lib.check(L.kf_run_sweep_scores(kf.handle, Tn, _ptr(d_et), _ptr(d_dt), _ptr(d_pay), _ptr(d_thr), _ptr(d_tab), None,
                                         _ptr(sc), None, None, _ptr(d_up), None, 1, _ptr(cx), _ptr(cP), s))
        _lib.check(L.kf_smooth_sweep_em(kf.handle, Tn, _ptr(d_et), _ptr(d_dt), _ptr(d_pay), _ptr(d_up), _ptr(d_tab), _ptr(cx),
                                        _ptr(cP), _ptr(sx), _ptr(sP), _ptr(st_), _ptr(sl), _ptr(st), _ptr(em), s))

    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        calls()
    for _ in range(2):
        for t in (cx, cP, sx, sP, st_, sl, em):
            t.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        for name, got in (('x', sx), ('P', sP), ('traj', st_), ('logdet', sl), ('status', st), ('em', em)):
            assert np.array_equal(_np(got), eager[name]), name
        np.testing.assert_array_equal(_np(d_up), up)
    kf.close()


# ---------------------------------------------------------------------------------------------
# 6. the Python drivers
# ---------------------------------------------------------------------------------------------
def test_facade(golden_dir):
    """AdaptiveSweep(em=True).em == the direct call over the driver's own arrays (records=False
    too), its smoothed() the em=False object's; ParameterSweep.em_update() round-trips through
    consts_table and keeps each set's P0; fit_noise's first iteration is that update."""
    _, events = _golden(golden_dir)
    thr = [-INF, -10.0]
    sw = ref15.AdaptiveSweep(events, thr, 0, len(events), smooth=True, em=True, records=False)
    plain_sw = ref15.AdaptiveSweep(events, thr, 0, len(events), smooth=True)
    sets = [ref15.ModelConsts('ref15'), _sets('ref15')[1]]
    ps = ref15.ParameterSweep(events, sets, thr, 0, len(events), smooth=True, em=True)
    try:
        assert isinstance(sw.em, np.ndarray) and sw.em.shape == (36, 2) and plain_sw.em is None
        assert sw.smoothed(0) == plain_sw.smoothed(0) and sw.smoothed(1) == plain_sw.smoothed(1)
        with kfmi.BatchedKF('ref15', 2, 'f64') as kf:
            direct = kf.smooth_sweep_em(sw._et, sw._dt, sw._pay, sw._up, sw._cx, sw._cP, x=False)
            np.testing.assert_array_equal(_np(direct.em), sw.em)
        assert sw._et[0] == ref15.NONE                                  # the leading entry: nothing is lost
        np.testing.assert_array_equal(sw.em[[0, 16, 32]], _counts(_np(sw._et), _np(sw._dt), _np(sw._up)))
        np.testing.assert_array_equal(ps.em[:, 0], sw.em[:, 0])         # the reference's set, ungated, in a table
        new = ps.em_update()
        assert len(new) == 2 and all(isinstance(c, ref15.ModelConsts) for c in new)
        want = kfmi.ref_em_update(ps.em, engine.consts_table('ref15', sets), 'ref15')
        np.testing.assert_array_equal(engine.consts_table('ref15', new), want)
        for c, old in zip(new, sets):
            np.testing.assert_array_equal(c.p0, old.p0)
        every = ps.em_update(imu_rows='all')
        assert not np.array_equal(every[0].r_imu[:3], sets[0].r_imu[:3])
        np.testing.assert_array_equal(new[0].r_imu[:3], sets[0].r_imu[:3])
        one = sw.em_update()
        np.testing.assert_array_equal(one[0].q, new[0].q)
        fit = ref15.fit_noise(events, sets, thr, iters=2, start_idx=0, end_idx=len(events))
        assert fit.history.shape == (3, 33, 2) and fit.nll.shape == (3, 2) and np.all(fit.status == 0)
        np.testing.assert_array_equal(fit.history[0], engine.consts_table('ref15', sets))
        np.testing.assert_array_equal(fit.history[1], want)
        np.testing.assert_array_equal(engine.consts_table('ref15', fit.consts), fit.history[2])
        nll0 = np.asarray(ps_scores_nll(events, sets, thr))
        np.testing.assert_array_equal(fit.nll[0], nll0)
        assert np.all(np.isfinite(fit.nll))
        with pytest.raises(ValueError):
            ref15.AdaptiveSweep(events, thr, 0, len(events), em=True)
    finally:
        sw.close()
        plain_sw.close()
        ps.close()


def ps_scores_nll(events, sets, thr):
    """The GPS + IMU innovation NLL of a scored ParameterSweep (fit_noise's nll[0])."""
    ps = ref15.ParameterSweep(events, sets, thr, 0, len(events), scores=True, records=False)
    try:
        with kfmi.BatchedKF('ref15', len(sets), 'f64') as kf:
            kf.set_state(ps._x0.expand(15, len(sets)).contiguous(), ps._P0.expand(27, len(sets)).contiguous())
            r = kf.run_sweep_scores(ps._et, ps._dt, ps._pay, ps._table, torch.from_numpy(ps.thresholds))
            return _np(kfmi.innovation_nll(r.scores, 'ref15', 'gps') + kfmi.innovation_nll(r.scores, 'ref15', 'imu'))
    finally:
        ps.close()
