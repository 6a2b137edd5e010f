"""The CV smoother oracle (cv_smoother_oracle.forward + backward, longdouble) against an independent
derivation: the information-form solve over all T states at once (no GPU).

Pass condition, test_smoother_oracle_cpu.py's: smoothed means within 1e-12 of max(|x|, sd) and
covariances within 1e-12 of sd_i sd_j (two longdouble derivations; 5e-15 was measured there).
"""
import numpy as np
import pytest

import cv_smoother_oracle as co

T, B = 12, 3


def _case(model, k, seed):
    d = co.axes(model)
    rng = np.random.default_rng(seed)
    dt_steps = rng.uniform(0.05, 0.3, T)
    p0, v = rng.uniform(-200, 200, (B, d)), rng.normal(0, 3.0, (B, d))
    x0 = np.zeros((B, 2 * d))
    x0[:, :d] = p0 + rng.normal(0, np.sqrt(3), (B, d))
    u = rng.normal(0, 0.3, (T, d, B))
    t_fix = np.cumsum(dt_steps)[k - 1::k][:T // k]
    z = p0.T[None] + v.T[None] * t_fix[:, None, None] + rng.normal(0, np.sqrt(3), (T // k, d, B))
    mask = np.ones((T // k, B), np.uint8)
    mask[(T // k) // 2, 1] = 0                          # filter 1 loses one fix
    return x0, dt_steps, u, z, mask


@pytest.mark.parametrize('model', ['cv2', 'cv3'])
@pytest.mark.parametrize('k', [1, 4])
def test_oracle_equals_information_form_solve(model, k):
    x0, dt_steps, u, z, mask = _case(model, k, 100 * k + co.axes(model))
    filt, sm = co.smoothed(model, x0, dt_steps, u, z, k, mask)
    assert int((filt['etype'][:, 1] == co.GPS).sum()) == T // k - 1   # the mask dropped one fix
    worst_x = worst_P = 0.0
    for f in range(B):
        xb, Pb = co.batch_solve(model, x0, dt_steps, u, z, k, f, mask)
        sd = np.sqrt(np.einsum('tii->ti', Pb))
        ex = np.abs(sm['x'][:, f] - xb) / np.maximum(np.abs(xb), sd)
        eP = np.abs(sm['P'][:, f] - Pb) / (sd[:, :, None] * sd[:, None, :])
        worst_x, worst_P = max(worst_x, float(ex.max())), max(worst_P, float(eP.max()))
    print(f'cv-smoother-oracle | {model} | k {k} | mean {worst_x:.2e} | cov {worst_P:.2e}')
    assert worst_x <= 1e-12 and worst_P <= 1e-12, (worst_x, worst_P)


def test_pack_unpack_roundtrip():
    rng = np.random.default_rng(3)
    cov = rng.normal(size=(4, 9, 5))
    P = co.unpack_cov('cv3', cov)
    assert np.array_equal(co.pack_cov('cv3', P), cov)
    assert np.array_equal(P, np.swapaxes(P, -1, -2)) and P[0, 0, 0, 1] == 0 and P[0, 0, 0, 4] == 0
