"""Pins cv_score_oracle without the GPU: its filter is cv_smoother_oracle.forward's, a batched run
with a table is the one-filter runs with K, and its innovation rows satisfy the prediction-error
decomposition against a joint Gaussian that no filter built.

The decomposition: the stacked fixes z of one filter are jointly Gaussian, N(mu, C), with mu and C
from F, Q, G u, P0 and R alone; factoring that density into the one-step predictive densities
gives sum NIS = (z - mu)^T C^-1 (z - mu) and sum log det S = log det C.  Both to 1e-12 relative in
longdouble (a float64 prototype of the identity agreed to 2e-13 at condition number 6.4e4).
"""
import numpy as np
import pytest

import cv_score_oracle as cso
import cv_smoother_oracle as cvo
import extended_oracle as xo

T, B = 12, 5
SETS = [(0.05, 0.4, 2.0), (0.5, 0.1, (1.0, 4.0, 9.0)), (0.01, 1.5, 0.5)]


def _case(model, k, seed, nB=B):
    d = cvo.axes(model)
    rng = np.random.default_rng(seed)
    dt_steps = rng.uniform(0.05, 0.3, T)
    p0, v = rng.uniform(-200, 200, (nB, d)), rng.normal(0, 3.0, (nB, d))
    x0 = np.zeros((nB, 2 * d))
    x0[:, :d] = p0 + rng.normal(0, np.sqrt(3), (nB, d))
    u = rng.normal(0, 0.3, (T, d, nB))
    t_fix = np.cumsum(dt_steps)[k - 1::k][:T // k]
    z = p0.T[None] + v.T[None] * t_fix[:, None, None] + rng.normal(0, np.sqrt(3), (T // k, d, nB))
    mask = np.ones((T // k, nB), np.uint8)
    if nB > 2:
        mask[(T // k) // 2, 1] = 0
    track = p0.T[None] + v.T[None] * np.cumsum(dt_steps)[:, None, None] + rng.normal(0, 0.5, (T, d, nB))
    track[::3] = np.nan
    if nB > 2:
        track[:, :, 2] = np.nan
    return x0, dt_steps, u, z, mask, track


def _sets(model):
    d = cvo.axes(model)
    return [(qp, qv, np.broadcast_to(r, (3,))[:d].copy()) for qp, qv, r in SETS]


@pytest.mark.parametrize('model', ['cv2', 'cv3'])
@pytest.mark.parametrize('arith', ['longdouble', 'f64'])
def test_filter_is_cv_smoother_oracles_forward(model, arith):
    x0, dt_steps, u, z, mask, track = _case(model, 2, 7)
    ref = cvo.forward(model, x0, dt_steps, u, z, 2, mask, arith=arith)
    got = cso.run(model, x0, dt_steps, u, z, 2, mask=mask, track=track, arith=arith)
    assert got['x'].dtype == ref['x'].dtype
    assert np.array_equal(got['x'], ref['x']) and np.array_equal(got['P'], ref['P'])
    # counts: the mask dropped one fix of filter 1; every third track row and filter 2's column are NaN
    n_fix = np.full(B, T // 2)
    n_fix[1] -= 1
    assert np.array_equal(got['scores'][0], n_fix)
    n_pos = np.full(B, T - len(range(0, T, 3)))
    n_pos[2] = 0
    assert np.array_equal(got['scores'][6], n_pos) and got['scores'][7, 2] == 0
    assert not got['scores'][3:6].any()


@pytest.mark.parametrize('model', ['cv2', 'cv3'])
@pytest.mark.parametrize('arith,dtype', [('longdouble', 'f64'), ('f64', 'f64'), ('f32', 'f32'), ('longdouble', 'f32')])
def test_table_run_equals_one_filter_runs_with_K(model, arith, dtype):
    x0, dt_steps, u, z, mask, track = _case(model, 3, 11)
    sets = _sets(model)
    tab = cso.table(model, sets, B)
    assert tab.shape == (2 + cvo.axes(model), B)
    fl = arith == 'longdouble'
    got = cso.run(model, x0, dt_steps, u, z, 3, mask=mask, consts=tab, track=track, dtype=dtype, arith=arith,
                  floors=fl)
    for f in range(B):
        one = cso.run(model, x0[f:f + 1], dt_steps, u[:, :, f:f + 1], z[:, :, f:f + 1], 3, mask=mask[:, f:f + 1],
                      K=sets[f % len(sets)], track=track[:, :, f:f + 1], dtype=dtype, arith=arith, floors=fl)
        assert np.array_equal(got['x'][:, f], one['x'][:, 0]) and np.array_equal(got['P'][:, f], one['P'][:, 0])
        assert np.array_equal(got['scores'][:, f], one['scores'][:, 0]), (f, got['scores'][:, f], one['scores'][:, 0])
        if fl:
            assert np.array_equal(got['floor'][:, f], one['floor'][:, 0])
            assert (got['floor'][[1, 2], f] > 0).all() and (got['floor'][[0, 3, 4, 5, 6], f] == 0).all()
    # distinct sets give distinct filters
    assert not np.array_equal(got['scores'][1, 0], got['scores'][1, 1])


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_prediction_error_decomposition(seed):
    model, k = 'cv2', 2
    x0, dt_steps, u, z, _, _ = _case(model, k, 40 + seed, nB=1)
    K = _sets(model)[seed % 3]
    got = cso.run(model, x0, dt_steps, u, z, k, K=K)
    mu, C = cso.joint_fixes(model, x0, dt_steps, u, k, K=K)
    A = xo._LongDouble
    zs = A.conv(z[:, :, 0]).reshape(-1)                                # fix-major, axes within
    L = xo._chol(A, C[None])
    w = xo._chol_solve(A, L, (zs - mu)[None, :, None])[0, :, 0]
    quad = (zs - mu).dot(w)
    logdet = 2 * np.log(np.stack([L[0, i, i] for i in range(len(mu))])).sum()
    nis, lds = got['scores'][1, 0], got['scores'][2, 0]
    assert got['scores'][0, 0] == T // k
    e_nis, e_ld = abs(nis - quad) / abs(quad), abs(lds - logdet) / abs(logdet)
    print(f'cv-score-oracle | seed {seed} | NIS {float(nis):.6f} rel {float(e_nis):.2e} | '
          f'logdet S {float(lds):.6f} rel {float(e_ld):.2e}')
    assert e_nis <= 1e-12 and e_ld <= 1e-12, (e_nis, e_ld)
