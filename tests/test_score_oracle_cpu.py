"""tests/score_oracle.py can referee kf_run_sweep_scores (no GPU): its float64 reference is
within 1e-12 relative of its longdouble truth on every float row, the rows are additive over a
cut run, a shut gate scores nothing, and innovation_nll is the Gaussian log-likelihood."""
import numpy as np
import pytest

import score_cases as sc
import score_oracle as so
from kfmi import engine
from test_gpu_param_sweep import ORACLE_THR, _events, _sets

INF = float('inf')
CAP = 1e-12


@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_f64_reference_is_within_1e12_of_the_truth(model):
    """E_ref / |truth| <= 1e-12 for rows 1, 2, 4, 5, 7 over the T = 300 stream, ungated, under each
    of the nine constant sets the GPU tests use (the reference's own and eight _symmetric_consts
    sets; the worst seen is 2.2e-13 for ref15 and 2.4e-13 for ref8).  Counts are equal."""
    worst = 0.0
    for f in range(9):
        tr, ref = sc.case(model, 'f64', f)
        s, r = tr['scores'], ref['scores']
        np.testing.assert_array_equal(np.asarray(s[[0, 3, 6]], np.float64), r[[0, 3, 6]])
        assert s[0] == 35 and s[3] == 259 and s[6] == 200
        for i in so.FLOAT_ROWS:
            rel = float(abs(so.LD(r[i]) - s[i]) / abs(s[i]))
            print(f'{model} set {f} {so.ROWS[i]:13s} truth {float(s[i]):.12g} E_ref {float(abs(so.LD(r[i]) - s[i])):.3e} '
                  f'rel {rel:.3e} floor {float(tr["floor"][i]):.3e}')
            assert rel <= CAP, (model, f, so.ROWS[i], rel)
            assert tr['floor'][i] > 0
            worst = max(worst, rel)
    print(f'{model}: worst E_ref / |truth| = {worst:.3e}')


@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_gated_reference_follows_the_truths_flags(model):
    """Under a finite gate the plain reference runs on the truth's flags (a caller-given mask), so
    its counts are the truth's, fewer than the ungated run's, and the cap holds there too."""
    f = 4
    thr = ORACLE_THR[model][f]
    tr, ref = sc.case(model, 'f64', f, thr)
    open_ = sc.case(model, 'f64', f)[0]['scores']
    s, r = tr['scores'], ref['scores']
    assert 0 < s[0] + s[3] < open_[0] + open_[3]
    np.testing.assert_array_equal(np.asarray(s[[0, 3, 6]], np.float64), r[[0, 3, 6]])
    assert s[0] + s[3] == tr['applied'].sum() and s[6] == open_[6]
    for i in so.FLOAT_ROWS:
        if s[i] != 0:
            assert float(abs(so.LD(r[i]) - s[i]) / abs(s[i])) <= CAP, so.ROWS[i]


def test_scores_are_additive_over_a_cut():
    """A run cut at event 128 and continued from its end state: the two parts' rows add up to the
    whole run's, counts exactly and sums to rounding (another summation order)."""
    et, dt, pay, x0 = _events(300)
    c = _sets('ref15')[2]
    x, P = sc.start('ref15', c, x0)
    kw = dict(K=c.oracle(), arith='f64')
    trk = sc.track(300)
    whole = so.run('ref15', x, P, et, dt, pay, track=trk, **kw)
    a = so.run('ref15', x, P, et[:128], dt[:128], pay[:128], track=trk[:128], **kw)
    b = so.run('ref15', a['x_end'], a['P_end'], et[128:], dt[128:], pay[128:], track=trk[128:], **kw)
    both = a['scores'] + b['scores']
    np.testing.assert_array_equal(both[[0, 3, 6]], whole['scores'][[0, 3, 6]])
    np.testing.assert_allclose(both, whole['scores'], rtol=1e-13, atol=0)
    np.testing.assert_array_equal(b['x_end'], whole['x_end'])


@pytest.mark.parametrize('thr', [INF, float('nan')])
def test_shut_gate_scores_no_innovation(thr):
    et, dt, pay, x0 = _events(300)
    c = _sets('ref8')[1]
    x, P = sc.start('ref8', c, x0)
    r = so.run('ref8', x, P, et, dt, pay, K=c.oracle(), arith='f64', thr=thr, track=sc.track(300))
    assert not r['applied'].any()
    np.testing.assert_array_equal(r['scores'][:6], np.zeros(6))
    assert r['scores'][6] == 200 and r['scores'][7] > 0


@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_innovation_nll_is_the_gaussian_log_likelihood(model):
    """engine.innovation_nll on the oracle's rows == -sum log N(y; 0, S) from SciPy over the
    applied updates of a 12-event case, per sensor."""
    from scipy.stats import multivariate_normal
    et, dt, pay, x0 = (v[:12] if v.ndim and len(v) == 300 else v for v in _events(300))
    assert (et == so.GPS).sum() >= 2 and (et == so.IMU).sum() >= 8
    c = _sets(model)[3]
    x, P = sc.start(model, c, x0)
    r = so.run(model, x, P, et, dt, pay, K=c.oracle(), arith='f64', keep_innov=True)
    table = r['scores'][:, None]
    for sensor in ('gps', 'imu'):
        want = -sum(multivariate_normal.logpdf(y, mean=np.zeros(len(y)), cov=(S + S.T) / 2)
                    for s, y, S in r['innov'] if s == sensor)
        got = engine.innovation_nll(table, model, sensor)
        assert got.shape == (1,)
        np.testing.assert_allclose(got[0], want, rtol=1e-11)
        np.testing.assert_allclose(so.innovation_nll(r['scores'], model, sensor), want, rtol=1e-11)
    assert engine.SCORE_ROWS == {k: i for i, k in enumerate(so.ROWS)}
    with pytest.raises(ValueError):
        engine.innovation_nll(table, model, 'lidar')
