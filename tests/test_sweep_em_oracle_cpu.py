"""tests/sweep_em_oracle.py referees kf_smooth_sweep_em, so it is checked here first, without a GPU:
the gain form of the E-step against the textbook lag-one form in longdouble, the lag-one covariance
against the off-diagonal blocks of one joint solve over all T states, the counts, the M-step's
keep-old rules, and the precondition of the GPU tests' gated cases (every finite threshold clear of
the truth's gate values, at every iteration of the EM-loop cases too)."""
import numpy as np
import pytest

import smoother_oracle as so
import sweep_em_cases as cases
import sweep_em_oracle as seo
from extended_oracle import GPS, IMU, LD, NONE, PREDICT
from test_smoother_oracle_cpu import _start, _stream

MODELS = cases.MODELS


@pytest.mark.parametrize('thr', cases.THR)
@pytest.mark.parametrize('model', MODELS)
def test_gain_form_is_the_lag_one_form(model, thr):
    """In longdouble, on the GPU tests' T = 300 stream, for every column they use: the same per-state
    sums (measured: <= 1.4e-15 relative), and the R rows and counts do not depend on the form."""
    et, dt, pay, x0 = cases.STREAMS['events']()
    worst = {g: 0.0 for g in seo.GROUPS}
    for ci in cases.COLUMNS:
        c = cases.estep_truth(model, ci, thr)
        K = cases._sets(model)[ci].oracle()
        lag = seo.estep(model, et, dt, c['truth'], K=K, form='lag_one')
        assert c['em'].dtype == LD and lag.dtype == LD
        e = seo.em_errors(lag, c['em'], model)
        worst = {g: max(worst[g], e[g]) for g in worst}
        R = seo.rows(model)
        for k in ('n_trans', 'n_imu', 'n_gps'):
            assert lag[R[k]] == c['em'][R[k]]
        # the plain leg is the same quantity, to rounding
        assert max(seo.em_errors(c['em_ref'], c['em'], model).values()) < 1e-9
    print(f'{model} thr={thr}: gain vs lag-one', ' '.join(f'{g} {v:.1e}' for g, v in worst.items()))
    assert max(worst.values()) <= 1e-12, worst


@pytest.mark.parametrize('thr', [-np.inf, 25.0])
@pytest.mark.parametrize('model', MODELS)
def test_lag_one_covariance_is_the_joint_solves_off_diagonal_block(model, thr):
    """On a stream without NONE events: Cov(x[t - 1], x[t] | all) = C_{t-1} P_s[t] against the joint
    Gaussian's off-diagonal block, and the Q sums built from the joint's blocks alone against estep's."""
    et, dt, pay = _stream(12)
    x0, P0 = _start(model, pay)
    r = so.run(model, x0, P0, et, dt, pay, thr=thr)
    mean, cov = seo.joint_cov(model, et, dt, r)
    n = r['xs'].shape[1]
    A = so._arith('longdouble')
    idx = np.arange(n)
    em = np.zeros(n, LD)
    worst = 0.0
    for t in range(1, len(et)):
        a, b = slice((t - 1) * n, t * n), slice(t * n, (t + 1) * n)
        F = r['F'][t]
        C = so._inv_apply(A, r['Pp'][t][None], (r['Pf'][t - 1] @ F.T)[None])[0]
        L = C @ r['Ps'][t]
        sd = np.sqrt(np.outer(r['Ps'][t - 1][idx, idx], r['Ps'][t][idx, idx]))
        worst = max(worst, float(np.max(np.abs(L - cov[a, b]) / sd)))
        e = mean[t] - F @ mean[t - 1]
        FS = F @ cov[a, b]
        W = np.outer(e, e) + cov[b, b] + F @ cov[a, a] @ F.T - FS - FS.T
        em += W[idx, idx] / LD(dt[t])
    print(f'{model} thr={thr}: lag-one covariance {worst:.1e}')
    assert worst <= 1e-12
    got = seo.estep(model, et, dt, r)
    R = seo.rows(model)
    err = np.abs(got[R['q']:R['q'] + n] - em) / np.abs(em)
    assert float(err.max()) <= 1e-10, err
    assert got[R['n_trans']] == len(et) - 1


@pytest.mark.parametrize('model', MODELS)
def test_counts(model):
    """NONE, PREDICT and dt = 0 events; event 0 is never counted, whatever it is."""
    et, dt, pay = _stream(12)
    et, dt = et.copy(), dt.copy()
    et[3] = NONE
    et[9] = PREDICT
    dt[5] = 0.0
    x0, P0 = _start(model, pay)
    for thr in (-np.inf, 25.0):
        r = so.run(model, x0, P0, et, dt, pay, thr=thr)
        em = seo.estep(model, et, dt, r)
        R = seo.rows(model)
        later = np.arange(12) >= 1
        assert em[R['n_trans']] == 12 - 1 - 1 - 1                       # not the NONE event, not the dt = 0 one
        assert em[R['n_imu']] == int(np.sum(later & r['applied'] & (et == IMU)))
        assert em[R['n_gps']] == int(np.sum(later & r['applied'] & (et == GPS)))
        assert (em[R['n_trans']], em[R['n_imu']], em[R['n_gps']]) == seo.counts(model, et, dt, r['applied'])
        assert et[0] == GPS and r['applied'][0]                          # event 0's fix was applied and is not in N_GPS
        if thr == -np.inf:
            assert em[R['n_gps']] == int(np.sum(et == GPS)) - 1
            assert em[R['n_imu']] == int(np.sum(et == IMU))
        assert np.all(em[seo.float_rows(model)['q']] > 0)
    typed = cases.STREAMS['typed']()
    c = cases.estep_truth(model, 0, -np.inf, 'typed')
    assert (c['em'][R['n_trans']], c['em'][R['n_imu']], c['em'][R['n_gps']]) == \
        seo.counts(model, typed[0], typed[1], c['truth']['applied'])
    assert c['em'][R['n_trans']] < np.sum(typed[0][1:] != NONE)         # its dt = 0 events are not counted


@pytest.mark.parametrize('model', MODELS)
def test_mstep_keeps_old_values(model):
    n, m = seo.dims(model)
    R = seo.rows(model)
    rng = np.random.default_rng(3)
    em = rng.uniform(1, 2, R['rows']).astype(LD)
    em[R['n_trans']], em[R['n_imu']], em[R['n_gps']] = 7, 5, 3
    tab = rng.uniform(1, 2, 2 * n + m)
    tab[2] = 0.0
    new = seo.mstep(em, tab, model)
    assert new.dtype == LD and new[2] == 0
    meas = list(seo.IMU_MEASURED[model])
    rest = [i for i in range(n) if i not in meas]
    keep = [i for i in range(n) if i != 2]
    np.testing.assert_array_equal(new[keep], em[R['q'] + np.array(keep)] / 7)
    np.testing.assert_array_equal(new[n + np.array(meas)], em[R['r_imu'] + np.array(meas)] / 5)
    np.testing.assert_array_equal(new[n + np.array(rest)], tab[n + np.array(rest)].astype(LD))
    np.testing.assert_array_equal(new[2 * n:], em[R['r_gps']:] / 3)
    np.testing.assert_array_equal(seo.mstep(em, tab, model, 'all')[n:2 * n], em[R['r_imu']:R['r_imu'] + n] / 5)
    np.testing.assert_array_equal(seo.mstep(em, tab, model, 'none')[n:2 * n], tab[n:2 * n].astype(LD))
    zero = em.copy()
    zero[R['n_trans']] = zero[R['n_imu']] = zero[R['n_gps']] = 0
    np.testing.assert_array_equal(seo.mstep(zero, tab, model, 'all'), tab.astype(LD))
    # the engine's M-step is the same rule in float64
    from kfmi import ref_em_update
    for rows in ('measured', 'all', 'none'):
        got = ref_em_update(em.astype(np.float64)[:, None], tab[:, None], model, rows)[:, 0]
        np.testing.assert_allclose(got, seo.mstep(em, tab, model, rows).astype(np.float64), rtol=4e-16, atol=0)


@pytest.mark.parametrize('model', MODELS)
def test_thresholds_are_clear_of_the_gate_values(model):
    """The precondition of every gated GPU comparison, on the truth: the E-step cases' finite
    thresholds (measured: >= 5e-4 under the reference's constants), both streams, and every iteration
    of the EM-loop cases."""
    worst = np.inf
    for stream, cols in (('events', cases.COLUMNS), ('typed', (0, 1))):
        for ci in cols:
            for thr in cases.THR + [5.0]:
                if not np.isfinite(thr) or (stream == 'typed' and thr != 5.0):
                    continue
                g = cases.estep_truth(model, ci, thr, stream)['truth']['gate']
                g = g[~np.isnan(g.astype(np.float64))]
                worst = min(worst, float(np.min(np.abs(g - thr))))
    print(f'{model}: E-step cases, gate margin {worst:.1e}')
    assert worst >= cases.GATE_MARGIN
    for thr in cases.LOOP_THR[model]:
        for rows in cases.LOOP_IMU_ROWS:
            truth, plain = cases.loop_truth(model, thr, rows)
            print(f'{model} loop thr={thr} {rows}: gate margins', ' '.join(f'{v:.1e}' for v in truth['margin']),
                  'applied', truth['applied'].sum(axis=1).tolist(), 'nll', ' '.join(f'{float(v):.6g}' for v in truth['nll']))
            assert np.all(truth['margin'] >= cases.GATE_MARGIN), (thr, rows, truth['margin'])
            np.testing.assert_array_equal(truth['applied'], plain['applied'])
            assert np.all(np.isfinite(truth['tables'].astype(np.float64))) and np.all(truth['tables'][:, :] >= 0)
