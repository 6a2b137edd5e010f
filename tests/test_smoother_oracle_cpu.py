"""tests/smoother_oracle.py referees the smoother kernel, so it is checked here first, without a
GPU: its longdouble RTS recursion against an independent derivation (one information-form solve
over all T states), the NONE pass-through, and the smoother's basic properties."""
import numpy as np
import pytest

import smoother_oracle as so
from extended_oracle import GPS, IMU, LD, NONE, PREDICT, Model

T = 12


def _stream(T, seed=5):
    """GPS at 0, 4, 8, 11, one PREDICT event, IMU elsewhere; dt = 0 at event 0 only."""
    rng = np.random.default_rng(seed)
    et = np.full(T, IMU, np.uint8)
    et[[0, 4, 8, 11]] = GPS
    et[6] = PREDICT
    dt = rng.uniform(0.004, 0.05, T)
    dt[0] = 0.0
    t = np.cumsum(dt)
    pay = np.zeros((T, 9))
    g = et == GPS
    pay[g, 0:3] = np.stack([300 + 3.3 * t, -200 + 2.2 * t, 0.1 * t], 1)[g] + rng.normal(0, 1.5, (int(g.sum()), 3))
    i = et == IMU
    pay[i, 0:3] = rng.normal(0, 0.02, (int(i.sum()), 3))
    pay[i, 3:6] = rng.normal(0, 0.01, (int(i.sum()), 3))
    pay[i, 6:9] = rng.normal(0, 0.05, (int(i.sum()), 3))
    return et, dt, pay


def _start(model, pay):
    M = Model(model)
    x0 = np.zeros(M.n)
    x0[:M.m] = pay[0, :M.m]
    return x0, M.P0()


@pytest.mark.parametrize('thr', [-np.inf, 25.0])
@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_rts_equals_information_form_batch_solve(model, thr):
    """The truth's smoothed means and covariances against the batch solve's: within 1e-12 of
    max(|x|, sd), and of sd_i sd_j for P (measured in longdouble: <= 1.1e-14)."""
    et, dt, pay = _stream(T)
    x0, P0 = _start(model, pay)
    r = so.run(model, x0, P0, et, dt, pay, thr=thr)
    assert r['xs'].dtype == LD
    n_upd = int(np.sum((et == GPS) | (et == IMU)))
    if thr == -np.inf:
        assert int(r['applied'].sum()) == n_upd
    xb, Pb = so.batch_solve(model, et, dt, r)
    idx = np.arange(r['xs'].shape[1])
    sd = np.sqrt(r['Ps'][:, idx, idx])
    ex = float(np.max(np.abs(r['xs'] - xb) / np.maximum(np.abs(xb), sd)))
    eP = float(np.max(np.abs(r['Ps'] - Pb) / (sd[:, :, None] * sd[:, None, :])))
    print(f'{model} thr={thr}: applied {int(r["applied"].sum())}/{n_upd}, x {ex:.2e}, P {eP:.2e}')
    assert ex <= 1e-12 and eP <= 1e-12, (ex, eP)


@pytest.mark.parametrize('arith', ['longdouble', 'f64'])
@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_none_event_passes_through(model, arith):
    """A NONE event inserted at k leaves every other row bit-identical; its own filtered row is
    row k - 1, and its smoothed row and the one before it are the original's smoothed row k - 1."""
    et, dt, pay = _stream(T)
    x0, P0 = _start(model, pay)
    a = so.run(model, x0, P0, et, dt, pay, arith=arith)
    for k in (3, T - 1, T):
        et2, dt2, pay2 = np.insert(et, k, NONE), np.insert(dt, k, 0.123), np.insert(pay, k, 7.0, axis=0)
        b = so.run(model, x0, P0, et2, dt2, pay2, arith=arith)
        keep = np.arange(T + 1) != k
        for key in ('xf', 'Pf', 'ldf', 'xs', 'Ps', 'lds'):
            np.testing.assert_array_equal(b[key][keep], a[key], err_msg=f'{key} k={k}')
            np.testing.assert_array_equal(b[key][k], a[key][k - 1], err_msg=f'{key} k={k}')
        assert not b['applied'][k]


@pytest.mark.parametrize('thr', [-np.inf, 25.0])
@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_last_row_is_filtered_and_variances_shrink(model, thr):
    et, dt, pay = _stream(T)
    x0, P0 = _start(model, pay)
    for arith, slack in (('longdouble', 1e-17), ('f64', 1e-12)):
        r = so.run(model, x0, P0, et, dt, pay, thr=thr, arith=arith)
        np.testing.assert_array_equal(r['xs'][-1], r['xf'][-1])
        np.testing.assert_array_equal(r['Ps'][-1], r['Pf'][-1])
        idx = np.arange(r['xs'].shape[1])
        vs, vf = r['Ps'][:, idx, idx], r['Pf'][:, idx, idx]
        assert np.all(vs > 0) and np.all(vs <= vf * (1 + slack))
        assert np.any(vs < 0.9 * vf)     # the backward pass did something


def test_plain_f64_is_close_to_the_truth():
    """The plain float64 leg is the same recursion: its error against the truth is rounding."""
    et, dt, pay = _stream(T)
    x0, P0 = _start('ref15', pay)
    a, b = so.run('ref15', x0, P0, et, dt, pay), so.run('ref15', x0, P0, et, dt, pay, arith='f64')
    assert b['xs'].dtype == np.float64
    np.testing.assert_array_equal(a['applied'], b['applied'])
    idx = np.arange(15)
    sd = np.sqrt(a['Ps'][:, idx, idx])
    assert float(np.max(np.abs(b['xs'] - a['xs']) / np.maximum(np.abs(a['xs']), sd))) < 1e-9
    assert float(np.max(np.abs(b['Ps'] - a['Ps']) / (sd[:, :, None] * sd[:, None, :]))) < 1e-9
