"""The EM oracle (cv_em_oracle, longdouble) against itself (no GPU): the recursive E-step statistics
against the joint (x[t - 1], x[t]) blocks of one information-form solve; the two algebraic forms of
the noise statistic against each other; the innovation negative log-likelihood over EM iterations;
the counts without the initial row.

Pass conditions.  Two longdouble derivations of one number: within 1e-12 relative (the smoothed
means and covariances by test_cv_smoother_oracle_cpu.py's measure and bound; 6e-16 measured for the
statistics, 6e-15 for the moments, 2e-14 between the two forms).
The likelihood: EM with an exact E-step never raises the data's negative log-likelihood, which for
this model is the innovation form ``cv_em_oracle.nll`` sums; the exact E-step needs the transition
out of the initial state.  Allowed increase per iteration: 2^-50 |NLL| (longdouble rounding of a sum
of ~200 terms; the smallest late decrease measured is 2e-6 relative).
"""
import numpy as np
import pytest

import cv_em_oracle as eo
import cv_smoother_oracle as co
import error_budget_cases as ec
import extended_oracle as xo
from test_cv_smoother_oracle_cpu import _case

T, B = 12, 3
SETS = [(0.0625, 0.5, (2.0, 3.0, 4.0)), (0.5, 0.125, (1.0, 1.0, 1.0)), (1.0, 1.0, (4.0, 4.0, 0.25))]


def _table(model):
    d = co.axes(model)
    return eo.cso.table(model, [(qp, qv, r[:d]) for qp, qv, r in SETS], B)


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


@pytest.mark.parametrize('model', ['cv2', 'cv3'])
@pytest.mark.parametrize('k', [1, 4])
def test_recursion_equals_joint_solve(model, k):
    x0, dt_steps, u, z, mask = _case(model, k, 100 * k + co.axes(model))
    d = co.axes(model)
    tab = _table(model)
    fwd, e = eo.iterate(model, x0, dt_steps, u, z, k, mask, tab)
    assert np.array_equal(e['em'][0], np.full(B, T)) and np.array_equal(e['em'][3], fwd['applied'].sum(axis=0))
    assert e['em'][3, 1] == T // k - 1                                  # the mask dropped one fix
    rows = [1, 2] + list(range(4, 4 + d))
    worst = worst_x = worst_P = 0.0
    for f in range(B):
        j = eo.joint_solve(model, x0, dt_steps, u, z, k, f, mask, tab)
        assert np.array_equal(j['em'][[0, 3]], e['em'][[0, 3], f])
        worst = max(worst, _rel(e['em'][rows, f], j['em'][rows]))
        xs = np.concatenate([e['init_x'][f][None], e['x'][:, f]])
        Ps = np.concatenate([e['init_P'][f][None], e['P'][:, f]])
        sd = np.sqrt(np.einsum('tii->ti', j['P']))
        worst_x = max(worst_x, float((np.abs(xs - j['x']) / np.maximum(np.abs(j['x']), sd)).max()))
        worst_P = max(worst_P, float((np.abs(Ps - j['P']) / (sd[:, :, None] * sd[:, None, :])).max()))
    print(f'cv-em-oracle | {model} | k {k} | em {worst:.2e} | mean {worst_x:.2e} | cov {worst_P:.2e}')
    assert worst <= 1e-12 and worst_x <= 1e-12 and worst_P <= 1e-12, (worst, worst_x, worst_P)


@pytest.mark.parametrize('model', ['cv2', 'cv3'])
def test_the_two_forms_agree(model):
    k = 4
    x0, dt_steps, u, z, mask = _case(model, k, 7 + co.axes(model))
    tab = _table(model)
    _, a = eo.iterate(model, x0, dt_steps, u, z, k, mask, tab, form='gain')
    _, b = eo.iterate(model, x0, dt_steps, u, z, k, mask, tab, form='lag_one')
    assert np.array_equal(a['em'][[0, 3]], b['em'][[0, 3]])
    worst = _rel(a['em'][[1, 2]], b['em'][[1, 2]])
    print(f'cv-em-oracle | {model} | gain form against lag-one form {worst:.2e}')
    assert worst <= 1e-12
    assert np.array_equal(a['em'][4:], b['em'][4:])                     # the R rows do not depend on the form


@pytest.mark.parametrize('model', ['cv2', 'cv3'])
def test_without_the_initial_row_the_counts_are_T_minus_1(model):
    k = 4
    x0, dt_steps, u, z, mask = _case(model, k, 11)
    tab = _table(model)
    _, e = eo.iterate(model, x0, dt_steps, u, z, k, mask, tab, use_init=False)
    assert np.array_equal(e['em'][0], np.full(B, T - 1)) and 'init_x' not in e
    dz = dt_steps.copy()
    dz[5] = 0.0                                                          # a transition of no duration is not counted
    _, e0 = eo.iterate(model, x0, dz, u, z, k, mask, tab, use_init=False)
    assert np.array_equal(e0['em'][0], np.full(B, T - 2)) and np.isfinite(e0['em'].astype(np.float64)).all()
    j = eo.joint_solve(model, x0, dt_steps, u, z, k, 2, mask, tab, use_init=False)
    assert j['em'][0] == T - 1 and _rel(e['em'][[1, 2], 2], j['em'][[1, 2]]) <= 1e-12


def test_mstep_keeps_the_old_value_at_a_zero_count():
    em = np.array([[4.0, 0.0], [8.0, 0.0], [2.0, 0.0], [0.0, 5.0], [0.0, 10.0], [0.0, 20.0]])
    tab = np.array([[9.0, 9.5], [7.0, 7.5], [3.0, 3.5], [1.0, 1.5]])
    new = eo.mstep(em, tab, 2)
    assert np.array_equal(new, np.array([[1.0, 9.5], [0.25, 7.5], [3.0, 2.0], [1.0, 4.0]]))


@pytest.mark.parametrize('k', [1, 5])
@pytest.mark.parametrize('model', ['cv2', 'cv3'])
def test_nll_never_increases_with_the_initial_row(model, k):
    """error_budget_cases.cv_case's inputs (regime A: T = 64, B = 70), a 70 % mask, 10 iterations from
    (q_pos, q_vel, r) = (5, 1, 3)."""
    c = ec.cv_case(model, 'A', k, False)
    rng = np.random.default_rng(ec._seed('cv-em-cpu', model, k))
    mask = (rng.random((ec.CV_T // k, ec.B)) < 0.7).astype(np.uint8)
    tab = eo.cso.table(model, [(5.0, 1.0, 3.0)], ec.B)
    tabs, nll = eo.em_loop(model, c['x0'], c['dt_steps'], c['u'], c['z'], k, mask, tab, 10)
    assert tabs.shape == (11, 2 + co.axes(model), ec.B) and nll.shape == (11, ec.B) and nll.dtype == xo.LD
    step = nll[1:] - nll[:-1]
    slack = xo.LD(2.0) ** -50 * np.abs(nll[:-1])
    print(f'cv-em-oracle | {model} | k {k} | NLL {float(nll[0].sum()):.3f} -> {float(nll[-1].sum()):.3f}, largest step '
          f'{float(step.max()):.3e}, smallest relative decrease {float((-step / np.abs(nll[:-1])).min()):.3e}')
    assert (step <= slack).all(), float((step - slack).max())
    assert (tabs[-1] > 0).all() and not np.array_equal(tabs[-1], tabs[0])
