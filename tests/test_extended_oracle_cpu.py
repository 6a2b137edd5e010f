"""The extended-precision oracle checked on the CPU: it is the same filter as oracle/ref_kf.py,
it is accurate enough to referee where float64 NumPy is not, and the budgets that
test_gpu_error_budget.py derives from the plain references stay under the caps of the regime
table for the committed seeds and shapes (so the GPU test cannot be loosened through its inputs).
"""
import numpy as np
import pytest

import error_budget_cases as ec
import extended_oracle as xo
from oracle import ref_kf


def _over_scale(e):
    """The worst entry of an ``errors`` result, log det over its scale like the other groups."""
    return max(v / (e['logdet_scale'] if k == 'logdet' else 1.0) for k, v in e.items() if k != 'logdet_scale')


def _benign(model, B=6, T=64, seed=3):
    rng = np.random.default_rng(seed)
    n = 15 if model == 'ref15' else 8
    etype = rng.choice([0, 1, 1, 1], size=(T, B)).astype(np.uint8)
    etype[rng.random((T, B)) < 0.05] = xo.PREDICT
    etype[0] = xo.GPS
    etype[T - 4:, 0] = xo.NONE
    dt = rng.uniform(0.0, 0.02, (T, B))
    dt[0] = 0.0
    pay = ec._payloads(rng, etype, dt, B)
    x0 = rng.normal(0, 0.1, (B, n))
    return x0, xo.Model(model).P0(), etype, dt, pay


@pytest.mark.parametrize('custom', [False, True])
@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_truth_is_the_reference_filter(model, custom):
    """Rounded to float64, the longdouble filter equals ref_kf.step15 / step8 on benign 64-event
    streams within 1e-11 on the ``errors`` scale (reference and caller constants).  Log det is
    taken over its scale here: slogdet's own absolute error on log det P0 = 117 is 1.2e-11."""
    K = ec.custom_constants(model, 77) if custom else None
    x0, P0, etype, dt, pay = _benign(model)
    if custom:
        P0 = xo.Model(model, K).P0()
    truth = xo.run_truth(model, x0, P0, etype, dt, pay, K=K)
    plain = xo.plain_f64(model, x0, P0, etype, dt, pay, K=K)
    rounded = {k: v.astype(np.float64) for k, v in truth.items()}
    e = xo.errors(plain, {k: v.astype(xo.LD) for k, v in rounded.items()}, xo.Model(model).groups)
    assert _over_scale(e) <= 1e-11, e
    assert e['P'] > 0.0 or e['logdet'] > 0.0            # two codes, not one compared with itself


@pytest.mark.parametrize('model', ['cv2', 'cv3'])
@pytest.mark.parametrize('update_every', [1, 5])
def test_truth_is_the_reference_cv_filter(model, update_every):
    """The same for ref_kf.run_batch (CVModel with its control u), every step of 64."""
    rng = np.random.default_rng(5)
    cv = ref_kf.CV2 if model == 'cv2' else ref_kf.CV3
    B, T, d = 6, 64, cv.d
    dt_steps = rng.uniform(0.01, 0.2, T)
    x0 = np.concatenate([rng.uniform(-500, 500, (B, d)), np.zeros((B, d))], axis=1)
    u = rng.normal(0, 0.3, (T, d, B))
    z = rng.uniform(-500, 500, (T // update_every, d, B))
    etype, dt, pay = xo.cv_events(model, T, B, dt_steps, z, update_every)
    truth = xo.run_truth(model, x0, cv.P0(), etype, dt, pay, u=u)
    plain = xo.plain_f64_cv(model, x0, dt_steps, u, z, update_every)
    e = xo.errors(plain, {k: v.astype(np.float64).astype(xo.LD) for k, v in truth.items()}, xo.Model(model).groups)
    assert _over_scale(e) <= 1e-11, e


def test_errors_sees_small_components_and_missing_values():
    """A 1e-3 m/s velocity error under positions of hundreds of metres is a velocity-group error
    of 1e-3 / scale, a NaN where a value was read back is an infinite error, and a value that
    was not read back is not judged."""
    x0, P0, etype, dt, pay = _benign('ref15', B=2, T=16)
    truth = xo.run_truth('ref15', x0, P0, etype, dt, pay)
    got = {k: v.astype(np.float64) for k, v in truth.items()}
    got['x'][5, 1, 7] += 1e-3
    G = xo.Model('ref15').groups
    e = xo.errors(got, truth, G)
    scale = float(np.sqrt(1000.0))                      # sqrt(P0_vel): the stream-wide velocity scale
    assert abs(e['vel'] - 1e-3 / scale) <= 1e-9 and e['pos'] <= 1e-15 and e['acc'] <= 1e-15
    got['x'][3, 0, 13] = np.nan
    assert xo.errors(got, truth, G)['acc'] == np.inf
    have = np.ones((16, 2, 15), bool)
    have[3, 0, 13] = False
    assert xo.errors(dict(got, x_have=have), truth, G)['acc'] <= 1e-15


def test_longdouble_against_mpmath():
    """Where float64 NumPy loses its digits — a 120-event ref15 stream with a 300 s gap before an
    IMU event, and a ref8 stream — longdouble's error against the same steps at 40 digits is at
    most 1/256 of the plain float64 reference's error on the same stream."""
    mpmath = pytest.importorskip('mpmath')
    for model in ('ref15', 'ref8'):
        rng = np.random.default_rng(11)
        T, n = (120, 15) if model == 'ref15' else (72, 8)
        etype = rng.choice([0, 1, 1, 1], size=(T, 1)).astype(np.uint8)
        etype[0] = xo.GPS
        dt = rng.uniform(0.0, 0.02, (T, 1))
        dt[0] = 0.0
        dt[T // 2 + 3] = 300.0
        etype[T // 2 + 3] = xo.IMU
        pay = ec._payloads(rng, etype, dt, 1)
        x0 = rng.normal(0, 0.1, (1, n))
        P0 = xo.Model(model).P0()
        with mpmath.workdps(40):
            exact = xo.run_truth(model, x0, P0, etype, dt, pay, arith='mp')
        G = xo.Model(model).groups
        e_ld = xo.errors(xo.run_truth(model, x0, P0, etype, dt, pay), exact, G)
        e_64 = xo.errors(xo.plain_f64(model, x0, P0, etype, dt, pay), exact, G)
        print(f'{model}: longdouble P {e_ld["P"]:.2e} logdet {e_ld["logdet"]:.2e}; float64 P {e_64["P"]:.2e} '
              f'logdet {e_64["logdet"]:.2e}')
        for k in ('P', 'logdet', 'pos', 'vel', 'acc'):
            assert e_ld[k] <= e_64[k] / 256, (model, k, e_ld[k], e_64[k])
        assert e_64['P'] > 1e-7                          # the stream is in the regime where float64 fails


def _assert_capped(e_ref, regime, dtype, what, caps=None):
    cap = ec.CAPS[regime][0 if dtype == 'f64' else 1]
    assert cap is not None, (regime, dtype)
    b = xo.budget(e_ref, dtype, ec.FACTOR[regime])
    over = {k: v for k, v in b.items()
            if v / (e_ref['logdet_scale'] if k == 'logdet' else 1.0) > (caps or {}).get(k, cap)}
    assert not over, (what, regime, dtype, over)


@pytest.mark.parametrize('model', ['ref15', 'ref8'])
@pytest.mark.parametrize('regime,dtype,custom', [('A', 'f64', False), ('B', 'f64', False), ('C', 'f64', False),
                                                 ('A', 'f32', False), ('B', 'f32', False), ('W', 'f32', False),
                                                 ('A', 'f64', True), ('B', 'f64', True)])
def test_event_budgets_are_capped(model, regime, dtype, custom):
    """The budgets of the event routes, for the inputs the GPU test runs: at most 1e-9 of scale
    in fp64 (regimes A, B), 1e-7 in regime C, 1e-4 in fp32."""
    _, e_ref = ec.event_reference(model, regime, custom, dtype)
    _assert_capped(e_ref, regime, dtype, model)


@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_regime_d_is_where_the_reference_form_cancels(model):
    """Regime D has no cap: the plain reference's own error there exceeds the old 1e-6 tolerance
    (which is why the budget's factor is 1), while attitude and rate, which the gap does not
    reach, stay at rounding level."""
    _, e_ref = ec.event_reference(model, 'D', False, 'f64')
    assert e_ref['P'] > 1e-6 and e_ref['logdet'] > 1e-6 and e_ref['vel'] > 1e-6, e_ref
    assert e_ref['att'] <= 1e-12 and e_ref['rate'] <= 1e-12, e_ref


@pytest.mark.parametrize('model', ['cv2', 'cv3'])
@pytest.mark.parametrize('regime', ['A', 'B'])
@pytest.mark.parametrize('update_every', [1, 5])
@pytest.mark.parametrize('dtype,offset', [('f64', False), ('f32', False), ('f64', True)])
def test_cv_budgets_are_capped(model, regime, update_every, dtype, offset):
    """The same for the constant-velocity routes.  With raw-UTM-size coordinates a position is
    rounded by up to half an ulp(4e6 m) = 4.7e-10 m, which a step of 0.1 s turns into 4.7e-9 m/s
    of velocity: over the velocity scale sqrt(P0_vel) that is the rounding-level error of that
    run, so its velocity cap is the budget's factor 8 times it (3.7e-9 for cv2, 1.2e-9 for cv3)
    instead of the table's 1e-9, which no fp64 evaluation can meet there (position, P and log
    det keep 1e-9: their scale grows with the coordinates)."""
    _, e_ref = ec.cv_reference(model, regime, update_every, offset, dtype)
    caps = None
    if offset:
        p0_vel = xo.Model(model).p0[-1]
        caps = {'vel': max(1e-9, 8 * 0.5 * np.spacing(ec.UTM_OFFSET[1]) / 0.1 / np.sqrt(p0_vel))}
    _assert_capped(e_ref, regime, dtype, model, caps)


@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_stream_budgets_are_capped(model):
    _, e_ref = ec.stream_reference(model)
    for regime in 'AB':
        _assert_capped(e_ref[regime], regime, 'f64', model)
