"""Shared inputs of the score tests (test_score_oracle_cpu.py, test_gpu_sweep_scores.py): the
parameter-sweep tests' stream and constant sets, imported, the stream's noiseless track, and the
oracle runs, each computed once and never modified."""
import numpy as np

import score_oracle as so
from test_gpu_param_sweep import _events, _sets
from test_gpu_sweep import _once

INF = float('inf')


def track(T):
    """The noiseless positions behind _events(T)'s fixes, every third row NaN (no reference there).
    _stream does not return them: its generator is replayed up to the position draw, and the
    replay is checked against the fixes it produced (position + N(0, 1.5) noise)."""
    def make():
        et, dt, pay, _ = _events(T)
        rng = np.random.default_rng(31)
        rng.random(len(np.arange(0, T, 7)))
        if T >= 100:
            rng.choice(np.arange(1, T), 6, replace=False)
        t = np.arange(T) * 0.005
        pos = np.stack([300 + 3.3 * t, -200 + 2.2 * t, 0.05 * np.cumsum(rng.normal(0, 0.1, T))], 1)
        g = et == so.GPS
        assert np.abs(pay[g, 0:3] - pos[g]).max() < 9.0 and np.abs(pay[g, 0:3] - pos[g]).max() > 0.0
        pos[2::3] = np.nan
        return pos
    return _once(('ptrack', T), make)


def start(model, c, x0):
    """One filter's cold start for the oracle: the stream's first fix, the set's dense P0."""
    n, k = (15, 3) if model == 'ref15' else (8, 2)
    x = np.zeros(n)
    x[0:k] = np.asarray(x0)[0:k]
    return x, np.diag(np.asarray(c.oracle()['p0'], np.float64)[:n])


def case(model, dtype, f, thr=-INF, T=300):
    """Set f of _sets(model) over _events(T) at the gate ``thr``: the truth run under its own gate
    with the floors, and the plain reference of ``dtype`` under the truth's flags.  Returns
    (truth, ref)."""
    def make():
        et, dt, pay, x0 = _events(T)
        c = _sets(model)[f]
        x, P = start(model, c, x0)
        tr = so.run(model, x, P, et, dt, pay, K=c.oracle(), dtype=dtype, thr=thr, track=track(T), floors=True)
        ref = so.run(model, x, P, et, dt, pay, K=c.oracle(), dtype=dtype, arith=dtype, applied=tr['applied'],
                     track=track(T))
        return tr, ref
    return _once(('score_case', model, dtype, f, thr, T), make)
