"""Kernel error per component group against the extended-precision truth — needs an MI355X.

Every other numeric test compares the GPU with float64 NumPy at 1e-6 (1e-3 in fp32), on a
whole-state norm or over max(|ref|, 1): five to eight orders above what the kernels achieve,
blind to small components, and refereed by a reference that loses its own digits after a
logging pause.  Here the kernels and the plain same-precision reference are both measured
against the longdouble filter of extended_oracle.py with one function (``errors``), and the
kernel's error E_gpu must stay within a budget derived from the reference's own error E_ref on
the same inputs:

    fp64:  E_gpu <= max(8 E_ref, 2^-40 scale)        fp32:  E_gpu <= max(8 E_ref32J, 2^-17 scale)

per state group (pos, att, vel, rate, acc), for P (scaled by sqrt(P_ii P_jj)) and for log det.
Two evaluations of one recurrence at one precision share its conditioning and differ in the
constant: three bits of margin.  The floor, for groups where E_ref is at rounding level, is 64
times the documented one-Newton reciprocal error (2^-46), 128 ulp in fp32.  In regime D (a 300 s
gap before an IMU event) the reference's (I - K H) P cancels and E_ref exceeds the old 1e-6; the
factor there is 1: the kernels' P = K R is no worse than the reference's form where it cancels.
test_extended_oracle_cpu.py caps these budgets for the very inputs used here.  The conditions
come from the reference side; none was tuned to a kernel.

Each test prints one line per (route, regime, dtype, group): E_gpu, E_ref, ratio, budget
(``pytest -s``; profiles/error_budget/error_budget.log is one such run).
"""
import numpy as np
import pytest
import torch

import error_budget_cases as ec
import extended_oracle as xo
import kfmi
from kfmi import ref15
from oracle import ref_kf

pytestmark = pytest.mark.gpu
NP = {'f64': np.float64, 'f32': np.float32}
WIDTH = {'ref15': 6, 'ref8': 3}


def _host(t):
    return t.double().cpu().numpy()


def _judge(route, regime, dtype, got, truth, e_ref, groups):
    e_gpu = xo.errors(got, truth, groups)
    over = ec.report(route, regime, dtype, e_gpu, e_ref, xo.budget(e_ref, dtype, ec.FACTOR[regime]))
    assert not over, {k: f'E_gpu {a:.3e} > budget {b:.3e}' for k, (a, b) in over.items()}


def _run_events(model, kernel, dtype, c):
    """The case's streams on one handle in segments of ec.SEGMENT events: the records give
    x[:W], log det and P per event, kf.state() the whole x and P after each segment."""
    etype, dt, pay = c['etype'], c['dt'], c['pay'].astype(NP[dtype])
    T, B = etype.shape
    n = c['x0'].shape[1]
    consts = ref15.ModelConsts(model, **c['K']) if c['K'] is not None else None
    kf = kfmi.BatchedKF(model, B, dtype, params=consts.params() if consts else None,
                        options={'events_kernel': kernel})
    P0b = np.repeat(ref15.to_blocks(c['P0'])[None], B, 0)
    kf.set_state(np.ascontiguousarray(c['x0'].T.astype(NP[dtype])), np.ascontiguousarray(P0b.T.astype(NP[dtype])))
    x = np.full((T, B, n), np.nan)
    have = np.zeros((T, B, n), bool)
    P = np.full((T, B, n, n), np.nan)
    ld = np.full((T, B), np.nan)
    W = WIDTH[model]
    for s in range(0, T, ec.SEGMENT):
        e = min(s + ec.SEGMENT, T)
        tr, l, _, cv = kf.run_events(etype[s:e], dt[s:e], pay[s:e], cov=True)
        x[s:e, :, :W] = _host(tr).transpose(0, 2, 1)
        have[s:e, :, :W] = True
        ld[s:e] = _host(l)
        P[s:e] = ref15.from_blocks(_host(cv).transpose(0, 2, 1))
        xs, Pb = kf.state()
        x[e - 1], have[e - 1] = _host(xs).T, True
        P[e - 1] = ref15.from_blocks(_host(Pb).T)
    status = kf.status().cpu().numpy()
    kf.close()
    assert (status == 0).all()
    return dict(x=x, x_have=have, P=P, logdet=ld)


EVENT_CASES = [(r, 'f64', False) for r in 'ABCD'] + [(r, 'f32', False) for r in 'ABW'] + \
              [(r, 'f64', True) for r in 'AB']


@pytest.mark.parametrize('regime,dtype,custom', EVENT_CASES,
                         ids=[f'{r}-{d}-{"custom" if c else "reference"}' for r, d, c in EVENT_CASES])
@pytest.mark.parametrize('kernel', ['lane', 'chain'])
@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_event_kernels_within_budget(model, kernel, regime, dtype, custom):
    """kf_run_events on the lane and chain kernels, 70 filters (one full wave plus a ragged one;
    nine 8-lane groups), every filter and every component judged: reference constants in fp64
    (regimes A-D) and fp32 (A, B, and W: regime A on tracks out to 600 m), caller constants in fp64
    (A, B)."""
    c = ec.event_case(model, regime, custom)
    truth, e_ref = ec.event_reference(model, regime, custom, dtype)
    got = _run_events(model, kernel, dtype, c)
    route = f'{model}/{kernel}/{"custom" if custom else "reference"}'
    _judge(route, regime, dtype, got, truth, e_ref, xo.Model(model).groups)


@pytest.mark.parametrize('dtype,offset', [('f64', False), ('f32', False), ('f64', True)],
                         ids=['f64', 'f32', 'f64-utm'])
@pytest.mark.parametrize('update_every', [1, 5])
@pytest.mark.parametrize('regime', ['A', 'B'])
@pytest.mark.parametrize('kernel', ['general', 'block2'])
@pytest.mark.parametrize('model', ['cv2', 'cv3'])
def test_cv_kernels_within_budget(model, kernel, regime, update_every, dtype, offset):
    """kf_run on the general and block kernels: steps of 0.1 s (regime B: one of 20 s), a fix
    every step or every fifth; state per group and log det per step, the final P.  The utm runs
    move x0 and the fixes by (5e5, 4e6, 100) m — raw-UTM-size coordinates, in fp64 (fp32 cannot
    hold them to better than 0.25 m) — and are judged on the same budgets."""
    c = ec.cv_case(model, regime, update_every, offset)
    truth, e_ref = ec.cv_reference(model, regime, update_every, offset, dtype)
    M = xo.Model(model)
    T, B, n = ec.CV_T, ec.B, M.n
    kf = kfmi.BatchedKF(model, B, dtype, options={'cv_kernel': kernel})
    P0 = np.repeat(M.P0()[None], B, 0)
    kf.set_state(np.ascontiguousarray(c['x0'].T.astype(NP[dtype])), ref_kf.tri_pack(P0).astype(NP[dtype]))
    tr, ld = kf.run(torch.from_numpy(c['u'].astype(NP[dtype])).cuda(), torch.from_numpy(c['z'].astype(NP[dtype])).cuda(),
                    dt_steps=torch.from_numpy(c['dt_steps']).cuda(), update_every=update_every)
    _, Pp = kf.state()
    status = kf.status().cpu().numpy()
    P = np.full((T, B, n, n), np.nan)
    P[-1] = ref_kf.tri_unpack(_host(Pp), n)
    P_have = np.zeros(T, bool)
    P_have[-1] = True
    got = dict(x=_host(tr).transpose(0, 2, 1), P=P, P_have=P_have, logdet=_host(ld))
    kf.close()
    assert (status == 0).all()
    route = f'{model}/{kernel}/k{update_every}{"/utm" if offset else ""}'
    _judge(route, regime, dtype, got, truth, e_ref, M.groups)


@pytest.mark.parametrize('regime', ['A', 'B'])
@pytest.mark.parametrize('final_pass', [False, True], ids=['maps', 'final-pass'])
@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_stream_route_within_budget(model, final_pass, regime):
    """The time-parallel route, one filter over 3000 events in chunks of 256 with the maps
    warm-up, records from the maps or from a final pass: the same budgets against E_ref over the
    same 3000 events.  Regime A must stand on the chunked records; in regime B (a 20 s gap in
    the middle of chunk 5) the sequential fallback is acceptable, and the line printed says
    which of the two happened."""
    c = ec.stream_case(model)
    truth, e_ref = ec.stream_reference(model)
    f = 'AB'.index(regime)
    et, dt, pay, x0 = c['etype'][:, f], c['dt'][:, f], c['pay'][:, :, f], c['x0'][f]
    P0b = ref15.to_blocks(c['P0'])
    dev = torch.device('cuda', 0)
    opts = {'stream_final': int(final_pass)}
    T, n, W = ec.STREAM_T, x0.shape[0], WIDTH[model]
    if model == 'ref15':
        tr, ld, xs, Pb, cv = ref15.run_stream_parallel(torch.as_tensor(et, device=dev), torch.as_tensor(dt, device=dev),
                                                       torch.as_tensor(pay, device=dev), x0, P0b,
                                                       chunk=ec.STREAM_CHUNK, warmup=-1, cov=True, options=opts)
        chk = dict(ref15.parallel_check)
        tr, ld, xs, Pb, cv = _host(tr), _host(ld), _host(xs), _host(Pb), _host(cv)
    else:
        kf = kfmi.BatchedKF(model, 1, 'f64', options=opts)
        kf.set_state(np.ascontiguousarray(x0[:, None]), np.ascontiguousarray(P0b[:, None]))
        tr, ld, _, cv = kf.run_stream(et, dt, pay, cov=True, chunk=ec.STREAM_CHUNK, warmup=-1)
        xs, Pb = kf.state()
        chk = kf.stream_check()
        tr, ld, xs, Pb, cv = _host(tr)[:, :, 0], _host(ld)[:, 0], _host(xs)[:, 0], _host(Pb)[:, 0], _host(cv)[:, :, 0]
        kf.close()
    print(f'error-budget | {model}/stream/{"final-pass" if final_pass else "maps"} | {regime} | chunked records '
          f'{"stood" if chk["ok"] else "fell back to " + str(chk["fallback"])} | chunks {chk["chunks"]} | '
          f'cov_gap {chk["cov_gap"]:.2e}')
    # warmup = -1 asks for the covariance maps alone: no events of warm-up were run before a chunk
    assert chk['chunks'] > 1 and chk['chunk'] == ec.STREAM_CHUNK and chk['warmup'] == 0, chk
    if regime == 'A':
        assert chk['ok'], chk
    x = np.full((T, 1, n), np.nan)
    have = np.zeros((T, 1, n), bool)
    x[:, 0, :W], have[:, :, :W] = tr, True
    x[-1, 0], have[-1] = xs, True
    P = ref15.from_blocks(cv)[:, None]
    P[-1, 0] = ref15.from_blocks(Pb)
    got = dict(x=x, x_have=have, P=P, logdet=ld[:, None])
    route = f'{model}/stream/{"final-pass" if final_pass else "maps"}'
    _judge(route, regime, 'f64', got, ec.one_filter(truth, f), e_ref[regime], xo.Model(model).groups)
