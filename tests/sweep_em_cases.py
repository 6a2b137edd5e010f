"""The cases tests/test_sweep_em_oracle_cpu.py and tests/test_gpu_sweep_em.py share, each computed
once per process — TEST INFRASTRUCTURE ONLY.

E-step cases: tests/test_gpu_smoother.py's (its streams, columns, thresholds and cached oracle
runs), with the statistics of tests/sweep_em_oracle.py on top.

EM-loop cases: the first LOOP_T events of that stream, LOOP_ITERS iterations from constant set
LOOP_SET, ungated and under one finite threshold per model, imu_rows 'measured' and 'all'.  The
finite thresholds were chosen on the longdouble loop so that at EVERY iteration the gate values stay
GATE_MARGIN clear of them (test_sweep_em_oracle_cpu.py asserts it; the constants move from one
iteration to the next and the gate values with them, so a threshold that is clear under the starting
set need not stay clear).
"""
import numpy as np

import sweep_em_oracle as seo
from test_gpu_param_sweep import _events, _sets
from test_gpu_smoother import COLUMNS, GATE_MARGIN, STREAMS, THR, T, _truth, _x0  # noqa: F401 (shared with the tests)
from test_gpu_sweep import INF, _once

MODELS = ['ref15', 'ref8']
LOOP_T = 120
LOOP_ITERS = 4
LOOP_SET = 1
LOOP_THR = {'ref15': [-INF, -10.0], 'ref8': [-INF, -10.0]}
LOOP_IMU_ROWS = ('measured', 'all')


def estep_truth(model, ci, thr, stream='events'):
    """dict(truth, plain: the two smoother runs; em: the longdouble gain-form statistics; em_ref: the
    plain float64 lag-one leg's) for constant set ci under thr."""
    def make():
        et, dt, pay, x0 = STREAMS[stream]()
        K = _sets(model)[ci].oracle()
        truth, plain = _truth(model, ci, thr, stream)
        return dict(truth=truth, plain=plain, em=seo.estep(model, et, dt, truth, K=K),
                    em_ref=seo.estep(model, et, dt, plain, K=K, arith='f64'))
    return _once(('em_truth', model, ci, thr, stream), make)


def loop_events():
    et, dt, pay, x0 = _events(T)
    return et[:LOOP_T], dt[:LOOP_T], pay[:LOOP_T], x0


def loop_truth(model, thr, imu_rows):
    """(longdouble, plain float64) ``sweep_em_oracle.em_loop`` of the loop case."""
    def make():
        et, dt, pay, x0 = loop_events()
        c = _sets(model)[LOOP_SET]
        a = (model, _x0(model, x0), c.P0, et, dt, pay, thr, c.oracle(), LOOP_ITERS, imu_rows)
        return seo.em_loop(*a), seo.em_loop(*a, arith='f64')
    return _once(('em_loop', model, thr, imu_rows), make)


def worst_over(errs):
    """Per group, the worst of a list of error dicts."""
    return {k: max(e[k] for e in errs) for k in errs[0]}


def budget(e_ref):
    """extended_oracle.budget itself on a dict of relative errors: 8 x E_ref, floor 2^-40."""
    import extended_oracle as xo
    return xo.budget(e_ref, 'f64')


assert np.isfinite(GATE_MARGIN)
