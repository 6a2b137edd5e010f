"""kf_smooth_sweep, the RTS backward pass over a sweep's filtered record (BatchedKF.smooth_sweep,
kfmi.ref15.AdaptiveSweep(smooth=True)) — needs an MI355X.

Accuracy is judged as the filter kernels' is (tests/test_gpu_error_budget.py): the kernel's
error against the longdouble truth of tests/smoother_oracle.py, per component group, within
extended_oracle.budget(E_ref, 'f64') (8 x E_ref, floor 2^-40), E_ref the plain NumPy float64
smoother's own error on the same inputs.  The stream and the constant sets are
tests/test_gpu_param_sweep.py's, imported; thresholds -inf, -10 and 5 apply 294 / 18 / 5 (ref8:
294 / 137 / 8) of the stream's 294 updates under the reference's constants.  Everything that
should be the same bits is compared with ==.

Measured on an MI355X over the 46 filter runs of the three oracle tests (each prints its figures
with -s; profiles/rts_smoother/smoother_budget.log): the worst E_gpu / budget is 0.016 (pos),
0.001 (att), 0.124 (vel), 0.0004 (rate), 0.110 (acc), 0.250 (P: 1.2e-11 against E_ref 6.0e-12) and
0.425 (log det: 3.1e-12 against E_ref 6.4e-13).
"""
import numpy as np
import pytest
import torch

import extended_oracle as xo
import kfmi
import smoother_oracle as so
from kfmi import _lib, ref15
from test_gpu_param_sweep import _events, _sets, _start
from test_gpu_sweep import INF, _golden, _list_arrays, _np, _once

pytestmark = pytest.mark.gpu
MODELS = ['ref15', 'ref8']
THR = [-INF, -10.0, 5.0]
COLUMNS = (0, 1, 3)      # the reference's constants, then two custom sets
GATE_MARGIN = 1e-6       # every threshold at least this far from the truth's gate values (measured: >= 5e-4)
DEPTH = 4                # the kernel's input ring (KF_SMOOTH_DEPTH)
T = 300


def _dims(model):
    return (15, 3) if model == 'ref15' else (8, 2)


def _x0(model, x0):
    n, k = _dims(model)
    x = np.zeros(n)
    x[:k] = np.asarray(x0)[:k]
    return x


def _typed_events():
    """_events(300) with PREDICT events and dt = 0 events after event 0."""
    def make():
        et, dt, pay, x0 = _events(T)
        et, dt = et.copy(), dt.copy()
        imu = np.nonzero(et == ref15.IMU)[0]
        et[imu[5::11]] = ref15.PREDICT
        dt[[1, 50, 51, 120, 299]] = 0.0
        return et, dt, pay, x0
    return _once('sm_typed', make)


STREAMS = {'events': lambda: _events(T), 'typed': _typed_events}


def _truth(model, ci, thr, stream='events'):
    """(truth, plain f64) of the smoother oracle for constant set ci under thr, computed once."""
    def make():
        et, dt, pay, x0 = STREAMS[stream]()
        c = _sets(model)[ci]
        a = (model, _x0(model, x0), c.P0, et, dt, pay)
        return so.run(*a, thr=thr, K=c.oracle()), so.run(*a, thr=thr, K=c.oracle(), arith='f64')
    return _once(('sm_truth', model, ci, thr, stream), make)


def _check_gates(truth, thr, updated=None):
    """The precondition of every comparison: the threshold is clear of the truth's gate values, and
    (after a forward launch) the device applied exactly the truth's updates."""
    if np.isfinite(thr):
        g = truth['gate'][~np.isnan(truth['gate'])]
        assert float(np.min(np.abs(g - thr))) >= GATE_MARGIN
    if updated is not None:
        np.testing.assert_array_equal(updated.astype(bool), truth['applied'])


def _column(sm, f):
    """Filter f of a smooth_sweep result as extended_oracle.errors' dict."""
    return dict(x=sm['x'][:, None, :, f], P=ref15.from_blocks(sm['P'][:, :, f])[:, None], logdet=sm['logdet'][:, f:f + 1])


def _judge(model, got, truth, plain, label):
    M = xo.Model(model)
    t = so.as_records(truth, 's')
    e_ref = xo.errors(so.as_records(plain, 's'), t, M.groups)
    bud = xo.budget(e_ref, 'f64')
    e = xo.errors(got, t, M.groups)
    print(label, ' '.join(f'{k} {e[k]:.1e}/{bud[k]:.1e} (E_ref {e_ref[k]:.1e})' for k in bud))
    for k in bud:
        assert e[k] <= bud[k], (label, k, e[k], bud[k], e_ref[k])


def _forward(model, et, dt, pay, x, P, thr, consts=None, params=None):
    """run_sweep(checkpoint_every=1): (filt_x, filt_P, updated) as device tensors / an array."""
    with kfmi.BatchedKF(model, x.shape[1], 'f64', params=params) as kf:
        kf.set_state(np.ascontiguousarray(x), np.ascontiguousarray(P))
        out = kf.run_sweep(et, dt, pay, np.asarray(thr, np.float64), traj=False, logdet=False, updated=True,
                           checkpoint_every=1, consts=consts)
        assert np.all(_np(kf.status()) == 0)
        return out[4], out[5], _np(out[2])


def _smooth(model, et, dt, fx, fP, consts=None, params=None, kf=None, **kw):
    """smooth_sweep on a fresh (or the given) handle; every output by default.  NumPy dict."""
    kw = {**dict(x=True, P=True, traj=True, logdet=True), **kw}
    own = kf is None
    if own:
        kf = kfmi.BatchedKF(model, fx.shape[2], 'f64', params=params)
    try:
        sm = kf.smooth_sweep(et, dt, fx, fP, consts=consts, **kw)
        return {k: _np(v) for k, v in sm._asdict().items()}
    finally:
        if own:
            kf.close()


def _assert_same(a, b, keys=('x', 'P', 'traj', 'logdet', 'status'), msg=''):
    for k in keys:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f'{k} {msg}')


# ---------------------------------------------------------------------------------------------
# against the truth
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', MODELS)
def test_end_to_end(model):
    """run_sweep(checkpoint_every=1) -> smooth_sweep, T = 300: column 0's constants on a plain
    handle with consts = NULL (the literal kernels), and two custom sets through the table, each
    under the three thresholds; x, P and logdet of every filter within the budget."""
    et, dt, pay, x0 = _events(T)
    sets = _sets(model)
    # the reference's constants: the handle's own, no table
    x, P = _start(model, [sets[0]] * 3, x0, 'f64')
    fx, fP, up = _forward(model, et, dt, pay, x, P, THR)
    sm = _smooth(model, et, dt, fx, fP)
    assert np.all(sm['status'] == 0)
    for f, thr in enumerate(THR):
        truth, plain = _truth(model, 0, thr)
        _check_gates(truth, thr, up[:, f])
        _judge(model, _column(sm, f), truth, plain, f'{model} set 0 thr {thr}')
    # two custom sets, columns of the table
    cols = [(ci, thr) for ci in COLUMNS[1:] for thr in THR]
    tab = [sets[ci] for ci, _ in cols]
    x, P = _start(model, tab, x0, 'f64')
    fx, fP, up = _forward(model, et, dt, pay, x, P, [thr for _, thr in cols], consts=tab)
    sm = _smooth(model, et, dt, fx, fP, consts=tab)
    assert np.all(sm['status'] == 0)
    for f, (ci, thr) in enumerate(cols):
        truth, plain = _truth(model, ci, thr)
        _check_gates(truth, thr, up[:, f])
        _judge(model, _column(sm, f), truth, plain, f'{model} set {ci} thr {thr}')
    n_up = [int(_truth(model, 0, thr)[0]['applied'].sum()) for thr in THR]
    assert n_up == ([294, 18, 5] if model == 'ref15' else [294, 137, 8])


@pytest.mark.parametrize('model', MODELS)
def test_backward_pass_alone(model):
    """No forward launch: the record is the truth's filtered record rounded to f64, the handle
    gives the model only and the table the constants.  Same budget."""
    et, dt, pay, x0 = _events(T)
    sets = _sets(model)
    cols = [(ci, thr) for ci in COLUMNS for thr in THR]
    fx = np.stack([_truth(model, ci, thr)[0]['xf'].astype(np.float64) for ci, thr in cols], 2)
    fP = np.stack([ref15.to_blocks(_truth(model, ci, thr)[0]['Pf'].astype(np.float64)) for ci, thr in cols], 2)
    sm = _smooth(model, et, dt, np.ascontiguousarray(fx), np.ascontiguousarray(fP), consts=[sets[ci] for ci, _ in cols])
    assert np.all(sm['status'] == 0)
    for f, (ci, thr) in enumerate(cols):
        truth, plain = _truth(model, ci, thr)
        _check_gates(truth, thr)
        _judge(model, _column(sm, f), truth, plain, f'{model} backward only, set {ci} thr {thr}')


@pytest.mark.parametrize('model', MODELS)
def test_event_types(model):
    """PREDICT events and dt = 0 events after event 0 are the same one step."""
    et, dt, pay, x0 = _typed_events()
    assert np.sum(et == ref15.PREDICT) >= 10 and np.sum(dt[1:] == 0) >= 4
    sets = _sets(model)
    cols = [(0, -INF), (0, 5.0), (1, -INF), (1, 5.0)]
    tab = [sets[ci] for ci, _ in cols]
    x, P = _start(model, tab, x0, 'f64')
    fx, fP, up = _forward(model, et, dt, pay, x, P, [thr for _, thr in cols], consts=tab)
    sm = _smooth(model, et, dt, fx, fP, consts=tab)
    assert np.all(sm['status'] == 0)
    for f, (ci, thr) in enumerate(cols):
        truth, plain = _truth(model, ci, thr, 'typed')
        _check_gates(truth, thr, up[:, f])
        _judge(model, _column(sm, f), truth, plain, f'{model} typed stream, set {ci} thr {thr}')


# ---------------------------------------------------------------------------------------------
# bit for bit
# ---------------------------------------------------------------------------------------------
BS = (1, 7, 8, 9, 17)
EDGE_THR = [-INF, -10.0, 5.0, INF]


def _edge_events(Tn):
    et, dt, pay, x0 = _events(19)
    et = et.copy()
    et[[3, 6]] = ref15.NONE
    return et[:Tn], dt[:Tn], pay[:Tn], x0


@pytest.mark.parametrize('model', MODELS)
def test_edges_bit_for_bit(model):
    """Every T from 1 to 2 depth + 1 (T = 1: no step; the ring's prologue only, its remainder only,
    its steady state) with NONE events at 3 and 6, B = 1, 7, 8, 9, 17 (a partial group of 8, a
    second and a third wave).  At every T and B: column f == filter f run alone at B = 1; row T - 1
    == the filtered row; row t == row t + 1 where etype[t + 1] is NONE.  At every T, B = 9: in
    place == out of place; each output alone == the run with every output; and a table column
    holding set c == a handle allocated with params = c and consts = NULL."""
    sets = _sets(model)[:17]
    thr = [EDGE_THR[f % 4] for f in range(17)]
    handles = {B: kfmi.BatchedKF(model, B, 'f64') for B in BS}
    try:
        for Tn in range(1, 2 * DEPTH + 2):
            et, dt, pay, x0 = _edge_events(Tn)
            x, P = _start(model, sets, x0, 'f64')
            fx, fP, _ = _forward(model, et, dt, pay, x, P, thr, consts=sets)
            assert tuple(fx.shape) == (Tn, x.shape[0], 17)
            solo = [_smooth(model, et, dt, fx[:, :, f:f + 1].contiguous(), fP[:, :, f:f + 1].contiguous(),
                            consts=sets[f:f + 1], kf=handles[1]) for f in range(17)]
            for B in BS:
                rx, rP = fx[:, :, :B].contiguous(), fP[:, :, :B].contiguous()
                sm = _smooth(model, et, dt, rx, rP, consts=sets[:B], kf=handles[B])
                assert np.all(sm['status'] == 0) and not np.isnan(sm['x']).any() and not np.isnan(sm['logdet']).any()
                for f in range(B):
                    _assert_same({k: v[..., f:f + 1] for k, v in sm.items()}, solo[f], msg=f'T={Tn} B={B} f={f}')
                np.testing.assert_array_equal(sm['x'][-1], _np(rx)[-1])
                np.testing.assert_array_equal(sm['P'][-1], _np(rP)[-1])
                for t in range(Tn - 1):
                    if et[t + 1] == ref15.NONE:
                        for k in ('x', 'P', 'traj', 'logdet'):
                            np.testing.assert_array_equal(sm[k][t], sm[k][t + 1], err_msg=f'{k} T={Tn} B={B} t={t}')
                    elif Tn > 1:
                        assert not np.array_equal(sm['P'][t], sm['P'][t + 1])
                if B != 9:
                    continue
                ix, iP = rx.clone(), rP.clone()
                inp = _smooth(model, et, dt, ix, iP, consts=sets[:B], kf=handles[B], inplace=True)
                _assert_same(inp, sm, msg=f'in place T={Tn}')
                np.testing.assert_array_equal(_np(ix), sm['x'])
                np.testing.assert_array_equal(_np(iP), sm['P'])
                ix = rx.clone()
                inp = _smooth(model, et, dt, ix, rP, consts=sets[:B], kf=handles[B], inplace=True, P=False)
                np.testing.assert_array_equal(_np(ix), sm['x'])
                for only in ('x', 'P', 'traj', 'logdet'):
                    one = _smooth(model, et, dt, rx, rP, consts=sets[:B], kf=handles[B],
                                  **{k: k == only for k in ('x', 'P', 'traj', 'logdet')})
                    assert all(one[k] is None for k in ('x', 'P', 'traj', 'logdet') if k != only)
                    _assert_same(one, sm, keys=(only, 'status'), msg=f'only {only} T={Tn}')
                for f in (0, 1, 2):   # set 0 is the reference's: the literal kernel
                    assert (sets[f].params() is None) == (f == 0)
                    own = _smooth(model, et, dt, fx[:, :, f:f + 1].contiguous(), fP[:, :, f:f + 1].contiguous(),
                                  params=sets[f].params())
                    _assert_same(own, solo[f], msg=f'handle constants T={Tn} f={f}')
    finally:
        for kf in handles.values():
            kf.close()


@pytest.mark.parametrize('model', MODELS)
def test_failure_is_isolated(model):
    """A NaN in one entry of filt_P at row r of one column (data, not a fault): that column's
    rows <= r are NaN, its rows > r the clean run's bits, its status KF_ENOTSPD; every other column
    and status unchanged bit for bit."""
    et, dt, pay, x0 = _events(T)
    sets = _sets(model)[:9]
    x, P = _start(model, sets, x0, 'f64')
    fx, fP, _ = _forward(model, et, dt, pay, x, P, [THR[f % 3] for f in range(9)], consts=sets)
    clean = _smooth(model, et, dt, fx, fP, consts=sets)
    assert np.all(clean['status'] == 0)
    r, col = 150, 4
    bad_P = fP.clone()
    bad_P[r, 7, col] = float('nan')
    bad = _smooth(model, et, dt, fx, bad_P, consts=sets)
    others = [f for f in range(9) if f != col]
    for k in ('x', 'P', 'traj', 'logdet'):
        assert np.isnan(bad[k][:r + 1, ..., col]).all(), k
        np.testing.assert_array_equal(bad[k][r + 1:, ..., col], clean[k][r + 1:, ..., col], err_msg=k)
        np.testing.assert_array_equal(bad[k][..., others], clean[k][..., others], err_msg=k)
    assert bad['status'][col] == _lib.KF_ENOTSPD and np.all(bad['status'][others] == 0)


def test_rejected_before_launch():
    """An f32 handle, another model and a NULL record are KF_EINVAL; T = 0 is KF_OK."""
    et, dt, pay, x0 = _events(19)
    d = torch.device('cuda', 0)
    a = [torch.as_tensor(v, device=d) for v in (et, dt)]
    fx, fP = torch.zeros(19, 15, 1, dtype=torch.float64, device=d), torch.zeros(19, 27, 1, dtype=torch.float64, device=d)
    L = _lib.lib()
    with kfmi.BatchedKF('ref15', 1, 'f32') as kf:
        args = (a[0].data_ptr(), a[1].data_ptr(), None, fx.data_ptr(), fP.data_ptr(), fx.data_ptr(), None, None, None, None)
        assert L.kf_smooth_sweep(kf.handle, 19, *args, kf._stream()) == _lib.KF_EINVAL and 'f64' in _lib.last_error()
        with pytest.raises(kfmi.KFError):
            kf.smooth_sweep(et, dt, fx.float(), fP.float())
    with kfmi.BatchedKF('cv3', 1, 'f64') as kf:
        assert L.kf_smooth_sweep(kf.handle, 19, *args, kf._stream()) == _lib.KF_EINVAL
    with kfmi.BatchedKF('ref15', 1, 'f64') as kf:
        assert L.kf_smooth_sweep(kf.handle, 19, a[0].data_ptr(), a[1].data_ptr(), None, None, fP.data_ptr(), None, None,
                                 None, None, None, kf._stream()) == _lib.KF_EINVAL
        assert 'null' in _lib.last_error()
        assert L.kf_smooth_sweep(kf.handle, -1, *args, kf._stream()) == _lib.KF_EINVAL
        assert L.kf_smooth_sweep(kf.handle, 0, None, None, None, None, None, None, None, None, None, None,
                                 kf._stream()) == _lib.KF_OK
        torch.cuda.synchronize()
        assert float(fx.abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------
# the Python drivers
# ---------------------------------------------------------------------------------------------
def test_adaptive_sweep_smoothed(golden_dir):
    """AdaptiveSweep(golden events, [-inf, -10], smooth=True): smoothed(i) against the oracle over
    the driver's own arrays (a leading NONE entry, then the window from its first fix) within the
    budget; result(i) and warm_start equal the smooth=False object's; dtype='f32' raises."""
    _, events = _golden(golden_dir)
    thr = [-INF, -10.0]
    sw = ref15.AdaptiveSweep(events, thr, 0, len(events), smooth=True)
    plain_sw = ref15.AdaptiveSweep(events, thr, 0, len(events), checkpoint_every=64)
    try:
        assert sw.every == 1
        et, dt, pay, x0 = _list_arrays(events)
        et = np.concatenate([[ref15.NONE], et]).astype(np.uint8)
        dt, pay = np.concatenate([[0.0], dt]), np.concatenate([np.zeros((1, 9)), pay])
        keep = et != ref15.NONE
        keep[0] = True
        M = xo.Model('ref15')
        for i, th in enumerate(thr):
            a = ('ref15', x0, ref15.P0, et, dt, pay)
            truth, plain = so.run(*a, thr=th), so.run(*a, thr=th, arith='f64')
            _check_gates(truth, th)
            res, ref = sw.result(i), plain_sw.result(i)
            assert res[0] == ref[0] and res[1] == ref[1] and res[3] == ref[3] and res[4] == ref[4]
            np.testing.assert_array_equal(res[2], ref[2])
            assert len(res[4]) - 1 == int(truth['applied'].sum())
            for end in (6, 64, 65, 200, len(events)):
                w, v = sw.warm_start(i, end), plain_sw.warm_start(i, end)
                assert w[0] == v[0] and w[2] == v[2]
                np.testing.assert_array_equal(w[1], v[1])
            states, logdets = sw.smoothed(i)
            assert len(states) == len(res[0]) and len(logdets) == len(res[1])
            assert [s[0] for s in states] == [s[0] for s in res[0]]
            assert states[-1] == res[0][-1] and logdets[-1] == res[1][-1]
            # states hold x[0:6]; P is not returned: compared through masks
            Tn = len(et)
            x = np.zeros((Tn, 1, 15))
            x[keep, 0, :6] = np.array(states)[:, 1:]
            ld = np.zeros((Tn, 1))
            ld[keep, 0] = logdets
            have = np.zeros((Tn, 1, 15), bool)
            have[keep, 0, :6] = True
            t = so.as_records(truth, 's')
            got = dict(x=x, x_have=have, P=np.zeros((Tn, 1, 15, 15)), P_have=np.zeros(Tn, bool), logdet=ld,
                       logdet_have=keep)
            groups = {g: M.groups[g] for g in ('pos', 'att')}
            e_ref = xo.errors(so.as_records(plain, 's'), t, groups)
            bud, e = xo.budget(e_ref, 'f64'), xo.errors(got, t, groups)
            print(f'golden thr {th}', ' '.join(f'{k} {e[k]:.1e}/{bud[k]:.1e}' for k in ('pos', 'att', 'logdet')))
            for k in ('pos', 'att', 'logdet'):
                assert e[k] <= bud[k], (th, k, e[k], bud[k])
        with pytest.raises(kfmi.KFError) as err:
            ref15.AdaptiveSweep(events, thr, 0, len(events), smooth=True, dtype='f32')
        assert err.value.code == _lib.KF_EINVAL
        out = ref15.run_smoothed_kalman_filter(events, 0, len(events), R_threshold=-10.0)
        assert len(out) == 7 and out[5] == sw.smoothed(1)[0] and out[6] == sw.smoothed(1)[1]
    finally:
        sw.close()
        plain_sw.close()
