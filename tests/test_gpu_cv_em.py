"""kf_smooth_run_em (BatchedKF.smooth_run_em / fit_noise, kfmi.cv_em_update): the constant-velocity
smoother with the EM statistics for q_pos, q_vel and R and the smoothed row before step 0 — needs an
MI355X.

Five parts.  (1) Bits, compared with ==: the smoothed outputs are kf_smooth_run_params'; the em rows
do not depend on B (column f of a B = 130 launch == the one-filter launch), on which outputs are NULL
or on running in place; the counts are exact; sm_init_* of a T-step call == row 0 of a call whose
record has the initial row prepended (and the noise rows of the two calls are the same sums).
Shapes: T around the input ring of 4, B around the wave, update_every 1 and 3, each with and without
mask, dt_steps, u, a constants' table and the initial row.  (2) Accuracy by the project's budget
rule against tests/cv_em_oracle.py: per float row the worst relative error over the filters against
the longdouble truth within extended_oracle.budget(E_ref, 'f64') (8 x E_ref, floor 2^-40), E_ref
the plain NumPy float64 leg's (textbook lag-one form); judged end to end (run_scores then
smooth_run_em) and on the truth's filtered record rounded to float64 alone; the smoothed record with
the initial row prepended is judged in test_gpu_cv_smoother.py's groups.  (3) EM: fit_noise's tables
against the longdouble EM loop under the same rule, and the innovation NLL never rising by more than
8 x the plain float64 loop's largest rise (floor 2^-40 |NLL|).  (4) Failure isolation by data.
(5) Refusals, T = 0, graph capture.

Measured on an MI355X over the 16 accuracy and 4 EM cases (each prints its figures with -s;
profiles/cv_em/em_budget.log), the worst E_gpu / budget per group: em rows q_pos 0.00017, q_vel
0.00071 (the gain form against a lag-one E_ref of 5e-12 / 8e-13) and r 0.202 (2.5e-13 against E_ref
1.6e-13); the smoothed record with the initial row pos 0.048, vel 0.080, P 0.059, log det 0.075;
fit_noise's tables over 6 iterations q_pos 0.0045, q_vel 0.0029, r 0.078.  The innovation NLL fell at
every iteration in every filter (largest step -1.9e-4); the float64 oracle loop never rose, so the
slack was the floor, 2^-40 |NLL|.
"""
import functools

import numpy as np
import pytest
import torch

import cv_em_oracle as eo
import cv_smoother_oracle as co
import error_budget_cases as ec
import extended_oracle as xo
import kfmi
from kfmi import _lib
from kfmi.engine import _ptr
from oracle import ref_kf

pytestmark = pytest.mark.gpu
SMOOTH_T = (1, 2, 4, 5, 6, 17)       # around the smoother's ring of 4; T - 1 (+ 1 with the initial row) backward steps
                                     # also lie around the EM instantiations' ring of 2 (KF_CV_EM_DEPTH)
WAVE_B = (1, 63, 64, 65, 130)        # wave edges
KS = (1, 3)
SENTINEL = -777.0
LD = np.longdouble
SETS5 = [(0.0625, 0.5, (2.0, 3.0, 4.0)), (0.5, 0.125, (1.0, 1.0, 1.0)), (0.015625, 2.0, (9.0, 0.5, 3.0)),
         (1.0, 1.0, (4.0, 4.0, 0.25)), (0.25, 0.03125, (0.75, 6.0, 2.5))]
SETS7 = SETS5 + [(0.125, 0.25, (3.0, 3.0, 3.0)), (2.0, 0.0625, (1.5, 8.0, 5.0))]
SM = ('x', 'P', 'logdet', 'status')


def _np(t):
    return None if t is None else t.cpu().numpy()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _table(model, sets, B):
    d = co.axes(model)
    return _dev(eo.cso.table(model, [(qp, qv, tuple(r[:d])) for qp, qv, r in sets], B))


def _inputs(model, T, B, k, general, seed):
    """fast: scalar dt, u, no mask, no table; general: dt_steps, a mask, u = None, a table."""
    d = co.axes(model)
    rng = np.random.default_rng(seed)
    x0 = np.zeros((2 * d, B))
    x0[:d] = rng.uniform(-200, 200, (d, B))
    u = None if general else rng.normal(0, 0.3, (T, d, B))
    z = x0[None, :d] + rng.normal(0, 2.0, (T // k, d, B))
    dts = rng.uniform(0.02, 0.3, T) if general else None
    mask = (rng.random((T // k, B)) < 0.7).astype(np.uint8) if general else None
    if T // k == 0:
        z = mask = None
    x0, u, z, dts, mask = (_dev(a) for a in (x0, u, z, dts, mask))
    return x0, u, z, dts, mask, (_table(model, SETS5, B) if general else None)


def _forward(kf, T, x0, u, z, dts, mask, tab, k):
    """The filtered record (kf_run_scores through the C API: T is explicit) and the state it started
    from, tri-packed."""
    kf.reset(x0)
    init = kf.state()
    tr, cv = kf.empty(T, kf.n, kf.batch), kf.empty(T, 3 * kf.c, kf.batch)
    _lib.check(_lib.lib().kf_run_scores(kf.handle, T, 0.1, _ptr(dts), _ptr(u), _ptr(z), _ptr(mask), k, _ptr(tab), None,
                                        None, _ptr(tr), _ptr(cv), None, kf._stream()))
    assert (_np(kf.status()) == 0).all()
    return tr, cv, init


def _params(kf, T, tr, cv, u, dts, tab):
    """kf_smooth_run_params itself, every output."""
    B = kf.batch
    outs = [kf.empty(T, kf.n, B), kf.empty(T, 3 * kf.c, B), kf.empty(T, B),
            torch.full((B,), 55, dtype=torch.int32, device='cuda')]
    _lib.check(_lib.lib().kf_smooth_run_params(kf.handle, T, 0.1, _ptr(dts), _ptr(u), _ptr(tr), _ptr(cv),
                                               *[_ptr(o) for o in outs], _ptr(tab), kf._stream()))
    return dict(zip(SM, (_np(o) for o in outs)))


def _all(sm):
    return {n: _np(v) for n, v in sm._asdict().items()}


def _counts(T, B, k, mask, init, dts=None):
    U = T // k
    n_fix = np.full(B, U) if mask is None else (_np(mask)[:U] != 0).sum(axis=0)
    n_tr = T - 1 + (1 if init else 0)
    if dts is not None:
        n_tr -= int((_np(dts)[0 if init else 1:] == 0).sum())
    return np.full(B, n_tr), n_fix


# -- 1. bits --------------------------------------------------------------------------------------

@pytest.mark.parametrize('with_init', [False, True], ids=['noinit', 'init'])
@pytest.mark.parametrize('general', [False, True], ids=['fast', 'general'])
@pytest.mark.parametrize('model', ['cv2', 'cv3'])
def test_bits(model, general, with_init):
    d = co.axes(model)
    for k in KS:
        for B in WAVE_B:
            with kfmi.BatchedKF(model, B, 'f64') as kf, kfmi.BatchedKF(model, 1, 'f64') as k1:
                for T in SMOOTH_T:
                    x0, u, z, dts, mask, tab = _inputs(model, T, B, k, general, 1000 * T + 10 * B + k)
                    tr, cv, init = _forward(kf, T, x0, u, z, dts, mask, tab, k)
                    init = init if with_init else None
                    where = (k, B, T)
                    kw = dict(u=u, dt=0.1, dt_steps=dts, update_every=k, mask=mask, init=init, consts=tab)
                    ref = _params(kf, T, tr, cv, u, dts, tab)
                    full = _all(kf.smooth_run_em(tr, cv, z, x=True, P=True, logdet=True, **kw))
                    for n in SM:                                   # the smoother is kf_smooth_run_params
                        assert np.array_equal(full[n], ref[n]), (n,) + where
                    em = full['em']
                    assert (full['status'] == 0).all() and np.isfinite(em).all(), where
                    n_tr, n_fix = _counts(T, B, k, mask, with_init)
                    assert np.array_equal(em[_lib.KF_EM_N_TRANS], n_tr), where
                    assert np.array_equal(em[_lib.KF_EM_N_FIX], n_fix), where
                    assert (em[[_lib.KF_EM_Q_POS, _lib.KF_EM_Q_VEL]] > 0).all() or n_tr[0] == 0, where
                    assert not em[[_lib.KF_EM_Q_POS, _lib.KF_EM_Q_VEL]][:, n_tr == 0].any(), where
                    assert not em[_lib.KF_EM_R:][:, n_fix == 0].any() and (em[_lib.KF_EM_R:][:, n_fix > 0] > 0).all(), where
                    assert (full['init_x'] is not None) == with_init
                    # which outputs are NULL
                    bare = _all(kf.smooth_run_em(tr, cv, z, status=False, init_out=False, **kw))
                    assert [n for n, v in bare.items() if v is not None] == ['em']
                    assert np.array_equal(bare['em'], em), where
                    for only in ('x', 'P', 'logdet'):
                        one = _all(kf.smooth_run_em(tr, cv, z, **{n: n == only for n in ('x', 'P', 'logdet')}, **kw))
                        assert np.array_equal(one[only], full[only]) and np.array_equal(one['em'], em), (only,) + where
                        if with_init:
                            assert np.array_equal(one['init_x'], full['init_x']), (only,) + where
                            assert np.array_equal(one['init_P'], full['init_P']), (only,) + where
                    noem = _all(kf.smooth_run_em(tr, cv, z, x=True, P=True, logdet=True, em=False, **kw))
                    assert noem['em'] is None and all(np.array_equal(noem[n], full[n]) for n in SM), where
                    # z NULL: no fixes counted, the noise rows do not move
                    noz = _all(kf.smooth_run_em(tr, cv, None, **{**kw, 'mask': None}))['em']
                    assert not noz[_lib.KF_EM_N_FIX:].any() and np.array_equal(noz[:_lib.KF_EM_N_FIX], em[:_lib.KF_EM_N_FIX]), where
                    # in place
                    trc, cvc = tr.clone(), cv.clone()
                    inp = kf.smooth_run_em(trc, cvc, z, x=True, P=True, logdet=True, inplace=True, **kw)
                    assert inp.x.data_ptr() == trc.data_ptr() and inp.P.data_ptr() == cvc.data_ptr()
                    inp = _all(inp)
                    for n in SM + ('em',) + (('init_x', 'init_P') if with_init else ()):
                        assert np.array_equal(inp[n], full[n]), (n,) + where
                    # lane-local: the filter alone
                    if B == 130:
                        for f in (0, 64, 129):
                            col = lambda t: None if t is None else t[..., f:f + 1].contiguous()  # noqa: E731
                            one = _all(k1.smooth_run_em(col(tr), col(cv), col(z), x=True, P=True, logdet=True, u=col(u), dt=0.1,
                                                        dt_steps=dts, update_every=k, mask=col(mask), consts=col(tab),
                                                        init=None if init is None else (col(init[0]), col(init[1]))))
                            for n in ('x', 'P', 'logdet', 'em') + (('init_x', 'init_P') if with_init else ()):
                                assert np.array_equal(one[n][..., 0], full[n][..., f]), (n, f) + where
                    if T > 2 and B > 1 and tab is not None:
                        assert not np.array_equal(em[1:3, 0], em[1:3, 1])      # the sets differ
    assert d in (2, 3)


@pytest.mark.parametrize('general', [False, True], ids=['fast', 'general'])
@pytest.mark.parametrize('model', ['cv2', 'cv3'])
def test_init_row_is_the_prepended_record_row(model, general):
    """sm_init_* of a T-step call == row 0 of the (T + 1)-step call over [initial row; record], whose
    step 0 is then never smoothed into (its dt and control are not read); rows 1 .. T == the T-step
    call's rows, and the noise rows are the same sums over the same T transitions."""
    k, B = 3, 130
    rows = None
    with kfmi.BatchedKF(model, B, 'f64') as kf:
        rows = kf._block_rows()
        for T in SMOOTH_T:
            x0, u, z, dts, mask, tab = _inputs(model, T, B, k, general, 17 * T + 3)
            tr, cv, init = _forward(kf, T, x0, u, z, dts, mask, tab, k)
            kw = dict(dt=0.1, consts=tab, x=True, P=True, logdet=True)
            a = _all(kf.smooth_run_em(tr, cv, None, u=u, dt_steps=dts, init=init, **kw))
            tr1 = torch.cat([init[0][None], tr]).contiguous()
            cv1 = torch.cat([init[1][rows][None], cv]).contiguous()
            u1 = None if u is None else torch.cat([torch.full_like(u[:1], 9.0), u]).contiguous()
            dts1 = None if dts is None else torch.cat([torch.full_like(dts[:1], 0.5), dts]).contiguous()
            b = _all(kf.smooth_run_em(tr1, cv1, None, u=u1, dt_steps=dts1, **kw))
            assert np.array_equal(a['init_x'], b['x'][0]) and np.array_equal(a['init_P'], b['P'][0]), T
            for n in ('x', 'P', 'logdet'):
                assert np.array_equal(a[n], b[n][1:]), (n, T)
            assert np.array_equal(a['em'], b['em']), T
            assert (a['em'][_lib.KF_EM_N_TRANS] == T).all() and not a['em'][_lib.KF_EM_N_FIX:].any()
            if T > 2:                                                        # a fix lies ahead: the step did something
                assert not np.array_equal(a['init_P'], _np(init[1][rows]))


def test_a_transition_of_no_duration_is_not_counted():
    model, T, B, k = 'cv3', 9, 65, 2
    x0, u, z, dts, mask, tab = _inputs(model, T, B, k, True, 5)
    dts[0] = 0.0
    dts[4] = 0.0
    with kfmi.BatchedKF(model, B, 'f64') as kf:
        tr, cv, init = _forward(kf, T, x0, u, z, dts, mask, tab, k)
        for with_init in (False, True):
            em = _np(kf.smooth_run_em(tr, cv, z, dt_steps=dts, update_every=k, mask=mask, consts=tab,
                                      init=init if with_init else None).em)
            n_tr, n_fix = _counts(T, B, k, mask, with_init, dts)
            assert n_tr[0] == T - 2
            assert np.array_equal(em[_lib.KF_EM_N_TRANS], n_tr) and np.array_equal(em[_lib.KF_EM_N_FIX], n_fix)
            assert np.isfinite(em).all() and (em[1:3] > 0).all()
        z0 = _np(kf.smooth_run_em(tr, cv, z, dt=0.0, update_every=k, mask=mask, consts=tab, init=init).em)
        assert not z0[:3].any() and np.isfinite(z0).all()                  # scalar dt = 0: nothing counted


# -- 2. accuracy ----------------------------------------------------------------------------------

CASES = [(m, r, k) for m in ('cv2', 'cv3') for r in 'AB' for k in (1, 5)]
CASE_IDS = [f'{m}-{r}-k{k}' for m, r, k in CASES]


@functools.lru_cache(maxsize=None)
def _case(model, regime, k):
    """cv_case's inputs, a 70 % mask and the 7-set table cycled over the filters."""
    c = ec.cv_case(model, regime, k, False)
    rng = np.random.default_rng(ec._seed('cv-em', model, regime, k))
    mask = (rng.random((ec.CV_T // k, ec.B)) < 0.7).astype(np.uint8)
    d = co.axes(model)
    tab = eo.cso.table(model, [(qp, qv, tuple(r[:d])) for qp, qv, r in SETS7], ec.B)
    return c, mask, tab


@functools.lru_cache(maxsize=None)
def _oracle(model, regime, k):
    """The truth and plain float64 legs, computed once: end to end, and the E-step alone over the
    truth's filtered record rounded to float64."""
    c, mask, tab = _case(model, regime, k)
    a = (model, c['x0'], c['dt_steps'], c['u'], c['z'], k, mask, tab)
    fwd, e = eo.iterate(*a)
    _, e64 = eo.iterate(*a, arith='f64')
    rx, rP = fwd['x'].astype(np.float64), fwd['P'].astype(np.float64)
    M = xo.Model(model)
    b = (model, rx, rP, c['dt_steps'], c['u'], c['z'], k, fwd['applied'])
    kw = dict(consts=tab, init=(c['x0'], M.P0()))
    return dict(e=e, e64=e64, rx=rx, rP=rP, b_truth=eo.estep(*b, **kw), b_plain=eo.estep(*b, arith='f64', **kw))


def _with_init_row(o):
    """An oracle leg's smoothed record with the initial row prepended; its log det is not judged."""
    ld = np.concatenate([np.zeros_like(o['logdet'][:1]), o['logdet']])
    return dict(x=np.concatenate([o['init_x'][None], o['x']]), P=np.concatenate([o['init_P'][None], o['P']]), logdet=ld)


def _judge(route, regime, model, sm, truth, plain):
    """The em rows and the smoothed record (initial row included) against one truth; returns the
    worst E_gpu / budget."""
    d = co.axes(model)
    got = _all(sm)
    assert (got['status'] == 0).all()
    T = got['x'].shape[0]
    n_fix = truth['em'][3]
    assert np.array_equal(got['em'][_lib.KF_EM_N_TRANS], truth['em'][0]) and np.array_equal(got['em'][_lib.KF_EM_N_FIX], n_fix)
    e_ref, e_gpu = eo.em_errors(plain['em'], truth['em'], d), eo.em_errors(got['em'], truth['em'], d)
    budget = xo.budget(e_ref, 'f64')
    over = ec.report(route + '/em', regime, 'f64', e_gpu, e_ref, budget)
    worst = max(e_gpu[g] / budget[g] for g in budget)
    assert not over, {g: f'E_gpu {a:.3e} > budget {b:.3e}' for g, (a, b) in over.items()}
    rec = dict(x=np.concatenate([got['init_x'][None], got['x']]).transpose(0, 2, 1),
               P=co.unpack_cov(model, np.concatenate([got['init_P'][None], got['P']])),
               logdet=np.concatenate([np.zeros((1, got['logdet'].shape[1])), got['logdet']]),
               logdet_have=np.arange(T + 1) > 0)
    groups = xo.Model(model).groups
    t1, p1 = _with_init_row(truth), _with_init_row(plain)
    p1['logdet_have'] = rec['logdet_have']
    e_ref, e_gpu = xo.errors(p1, t1, groups), xo.errors(rec, t1, groups)
    budget = xo.budget(e_ref, 'f64')
    over = ec.report(route + '/record', regime, 'f64', e_gpu, e_ref, budget)
    assert not over, {g: f'E_gpu {a:.3e} > budget {b:.3e}' for g, (a, b) in over.items()}
    print(f'cv_em_budget {route} {regime} worst em E_gpu/budget {worst:.3g}')
    return worst


@pytest.mark.parametrize('model,regime,k', CASES, ids=CASE_IDS)
def test_end_to_end_within_budget(model, regime, k):
    """(a) run_scores -> smooth_run_em on cv_case's inputs (T = 64, B = 70)."""
    (c, mask, tab), o = _case(model, regime, k), _oracle(model, regime, k)
    M = xo.Model(model)
    with kfmi.BatchedKF(model, ec.B, 'f64') as kf:
        kf.set_state(np.ascontiguousarray(c['x0'].T), ref_kf.tri_pack(np.repeat(M.P0()[None], ec.B, 0)))
        init = kf.state()
        u, z, dts, md, td = (_dev(a) for a in (c['u'], c['z'], c['dt_steps'], mask, tab))
        sr = kf.run_scores(u, z, consts=td, dt_steps=dts, update_every=k, mask=md, scores=False, traj=True, cov=True)
        assert (_np(kf.status()) == 0).all()          # the precondition
        sm = kf.smooth_run_em(sr.traj, sr.cov, z, u=u, dt_steps=dts, update_every=k, mask=md, init=init, consts=td,
                              x=True, P=True, logdet=True)
        _judge(f'{model}/run_scores+smooth_run_em/k{k}', regime, model, sm, o['e'], o['e64'])


@pytest.mark.parametrize('model,regime,k', CASES, ids=CASE_IDS)
def test_estep_alone_within_budget(model, regime, k):
    """(b) smooth_run_em on the truth's filtered record rounded to float64."""
    (c, mask, tab), o = _case(model, regime, k), _oracle(model, regime, k)
    M = xo.Model(model)
    with kfmi.BatchedKF(model, ec.B, 'f64') as kf:
        fx = np.ascontiguousarray(o['rx'].transpose(0, 2, 1))
        init = (_dev(c['x0'].T), _dev(co.pack_cov(model, np.repeat(M.P0()[None, None], ec.B, 1))[0]))
        sm = kf.smooth_run_em(fx, co.pack_cov(model, o['rP']), c['z'], u=c['u'], dt_steps=c['dt_steps'], update_every=k,
                              mask=mask, init=init, consts=tab, x=True, P=True, logdet=True)
        _judge(f'{model}/smooth_run_em/k{k}', regime, model, sm, o['b_truth'], o['b_plain'])


# -- 3. EM ----------------------------------------------------------------------------------------

EM_ITERS = 6
EM_CASES = [('cv2', 'A', 1), ('cv3', 'A', 5), ('cv2', 'B', 5), ('cv3', 'B', 1)]


@functools.lru_cache(maxsize=None)
def _em_oracle(model, regime, k):
    c, mask, _ = _case(model, regime, k)
    start = eo.cso.table(model, [(5.0, 1.0, 3.0)], ec.B)
    a = (model, c['x0'], c['dt_steps'], c['u'], c['z'], k, mask, start, EM_ITERS)
    return start, eo.em_loop(*a), eo.em_loop(*a, arith='f64')


@pytest.mark.parametrize('model,regime,k', EM_CASES, ids=[f'{m}-{r}-k{k}' for m, r, k in EM_CASES])
def test_fit_noise_follows_the_oracle_loop(model, regime, k):
    """6 iterations from (q_pos, q_vel, r) = (5, 1, 3) at B = 70 with a 70 % mask."""
    (c, mask, _) = _case(model, regime, k)
    start, (t_tabs, t_nll), (p_tabs, p_nll) = _em_oracle(model, regime, k)
    with kfmi.BatchedKF(model, ec.B, 'f64') as kf:
        fit = kf.fit_noise(_dev(c['u']), _dev(c['z']), x0=_dev(c['x0'].T), consts=_dev(start), iters=EM_ITERS,
                           dt_steps=_dev(c['dt_steps']), update_every=k, mask=_dev(mask))
        assert (_np(fit.status) == 0).all()
        hist, nll = _np(fit.history), _np(fit.nll)
        assert np.array_equal(hist[-1], _np(fit.consts)) and np.array_equal(hist[0], start)
    assert hist.shape == t_tabs.shape and nll.shape == t_nll.shape == (EM_ITERS + 1, ec.B)
    e_ref, e_gpu = eo.table_errors(p_tabs, t_tabs), eo.table_errors(hist, t_tabs)
    budget = xo.budget(e_ref, 'f64')
    route = f'{model}/fit_noise/k{k}'
    over = ec.report(route, regime, 'f64', e_gpu, e_ref, budget)
    print(f'cv_em_budget {route} {regime} worst table E_gpu/budget {max(e_gpu[g] / budget[g] for g in budget):.3g}')
    assert not over, {g: f'E_gpu {a:.3e} > budget {b:.3e}' for g, (a, b) in over.items()}
    rise_ref = float(np.maximum(p_nll[1:] - p_nll[:-1], 0).max())
    slack = np.maximum(8.0 * rise_ref, 2.0 ** -40 * np.abs(nll[:-1]))
    step = nll[1:] - nll[:-1]
    print(f'cv_em_nll {route} {regime} NLL {nll[0].sum():.3f} -> {nll[-1].sum():.3f} (truth {float(t_nll[0].sum()):.3f} -> '
          f'{float(t_nll[-1].sum()):.3f}); largest rise {step.max():.3e}, the float64 loop\'s {rise_ref:.3e}, '
          f'smallest slack {slack.min():.3e}')
    assert (step <= slack).all(), float((step - slack).max())


# -- 4. failure isolation -------------------------------------------------------------------------

def test_failure_is_per_filter():
    """A NaN planted in one filter's filt_P row r (data, not a fault): its float rows are NaN, its
    counts still count, its status is KF_ENOTSPD; every neighbour == the clean run."""
    model, T, B, k, r, f = 'cv3', 17, 130, 2, 9, 70
    x0, u, z, dts, mask, tab = _inputs(model, T, B, k, True, 21)
    with kfmi.BatchedKF(model, B, 'f64') as kf:
        tr, cv, init = _forward(kf, T, x0, u, z, dts, mask, tab, k)
        kw = dict(dt_steps=dts, update_every=k, mask=mask, init=init, consts=tab, x=True, P=True, logdet=True)
        clean = _all(kf.smooth_run_em(tr, cv, z, **kw))
        bad_cv = cv.clone()
        bad_cv[r, 4, f] = float('nan')
        bad = _all(kf.smooth_run_em(tr, bad_cv, z, **kw))
    others = np.arange(B) != f
    assert bad['status'][f] == _lib.KF_ENOTSPD and (bad['status'][others] == 0).all() and (clean['status'] == 0).all()
    for n in ('x', 'P', 'logdet', 'em', 'init_x', 'init_P'):
        assert np.array_equal(bad[n][..., others], clean[n][..., others]), n
    for n in ('x', 'P', 'logdet'):
        assert np.isnan(bad[n][:r + 1, ..., f]).all() and np.array_equal(bad[n][r + 1:, ..., f], clean[n][r + 1:, ..., f]), n
    assert np.isnan(bad['init_x'][:, f]).all() and np.isnan(bad['init_P'][:, f]).all()
    em = bad['em'][:, f]
    assert np.isnan(em[[1, 2, 4, 5, 6]]).all()
    assert em[_lib.KF_EM_N_TRANS] == T and em[_lib.KF_EM_N_FIX] == clean['em'][_lib.KF_EM_N_FIX, f] > 0


# -- 5. refusals, T = 0, graph capture ------------------------------------------------------------

def _raw(kf, T, d, td, k=1, z=True, mask=False, init_x=False, init_P=False, sm_init=False):
    """kf_smooth_run_em with sentinel-filled outputs: (rc, outputs)."""
    B = kf.batch
    n = max(T, 1)
    fx, fP = torch.ones(n, 2 * d, B, dtype=td, device='cuda'), torch.ones(n, 3 * d, B, dtype=td, device='cuda')
    zz = torch.zeros(n, d, B, dtype=td, device='cuda') if z else None
    mm = torch.ones(n, B, dtype=torch.uint8, device='cuda') if mask else None
    ix = torch.ones(2 * d, B, dtype=td, device='cuda') if init_x else None
    iP = torch.ones(3 * d, B, dtype=td, device='cuda') if init_P else None
    outs = [torch.full((n, 2 * d, B), SENTINEL, dtype=td, device='cuda'),
            torch.full((n, 3 * d, B), SENTINEL, dtype=td, device='cuda'),
            torch.full((n, B), SENTINEL, dtype=td, device='cuda'),
            torch.full((B,), 55, dtype=torch.int32, device='cuda'),
            torch.full((2 * d, B), SENTINEL, dtype=td, device='cuda'),
            torch.full((3 * d, B), SENTINEL, dtype=td, device='cuda'),
            torch.full((_lib.KF_EM_ROWS(d), B), SENTINEL, dtype=torch.float64, device='cuda')]
    si = [_ptr(outs[4]), _ptr(outs[5])] if sm_init else [None, None]
    rc = _lib.lib().kf_smooth_run_em(kf.handle, T, 0.1, None, None, _ptr(zz), _ptr(mm), k, _ptr(fx), _ptr(fP), _ptr(ix),
                                     _ptr(iP), *[_ptr(o) for o in outs[:4]], *si, None, _ptr(outs[6]), kf._stream())
    torch.cuda.synchronize()
    return rc, outs


def _untouched(outs):
    return all(bool((o == (55 if o.dtype == torch.int32 else SENTINEL)).all()) for o in outs)


@pytest.mark.parametrize('why', ['f32', 'reference_model', 'init_x_alone', 'init_P_alone', 'sm_init_without_init',
                                 'update_every_0', 'mask_without_z', 'negative_T'])
def test_refusals(why):
    model, dtype = ('ref15', 'f64') if why == 'reference_model' else ('cv3', 'f32' if why == 'f32' else 'f64')
    kw = dict(init_x_alone=dict(init_x=True), init_P_alone=dict(init_P=True), sm_init_without_init=dict(sm_init=True),
              update_every_0=dict(k=0), mask_without_z=dict(z=False, mask=True)).get(why, {})
    with kfmi.BatchedKF(model, 8, dtype) as kf:
        rc, outs = _raw(kf, -1 if why == 'negative_T' else 5, 3, torch.float32 if dtype == 'f32' else torch.float64, **kw)
        assert rc == _lib.KF_EINVAL and 'kf_smooth_run_em' in _lib.last_error(), _lib.last_error()
        assert _untouched(outs)
        if why in ('f32', 'reference_model'):
            with pytest.raises(kfmi.KFError) as e:
                kf.smooth_run_em(np.ones((5, 6, 8)), np.ones((5, 9, 8)), None, dt=0.1)
            assert e.value.code == _lib.KF_EINVAL
            with pytest.raises(kfmi.KFError) as e:
                kf.fit_noise(None, np.ones((5, 3, 8)), dt=0.1)
            assert e.value.code == _lib.KF_EINVAL


def test_T0_zeroes_the_table_and_the_handle_is_not_touched():
    with kfmi.BatchedKF('cv3', 65, 'f64') as kf:
        kf.reset()
        before = [_np(t) for t in kf.state()]
        rc, outs = _raw(kf, 0, 3, torch.float64)
        assert rc == _lib.KF_OK, _lib.last_error()
        assert not _np(outs[6]).any() and _untouched(outs[:6])
        rc, outs = _raw(kf, 5, 3, torch.float64, init_x=True, init_P=True, sm_init=True)
        assert rc == _lib.KF_OK and not any(bool((o == SENTINEL).any()) for o in outs)
        assert all(np.array_equal(a, _np(b)) for a, b in zip(before, kf.state())) and (_np(kf.status()) == 0).all()


def test_graph_capture_replays_the_eager_bits():
    """kf_reset + kf_run_scores + kf_smooth_run_em captured into one graph (nothing allocates or
    synchronises) and replayed twice == the eager calls."""
    model, T, B, k = 'cv3', 9, 130, 2
    x0, u, z, _, _, _ = _inputs(model, T, B, k, False, 11)
    tab = _table(model, SETS5, B)
    with kfmi.BatchedKF(model, B, 'f64') as kf:
        tr0, cv0, init = _forward(kf, T, x0, u, z, None, None, tab, k)
        ix, iP = init[0], init[1][kf._block_rows()].contiguous()
        eager = _all(kf.smooth_run_em(tr0, cv0, z, u=u, dt=0.1, update_every=k, init=(ix, iP), consts=tab, x=True, P=True,
                                      logdet=True))
    kf = kfmi.BatchedKF(model, B, 'f64')
    tr, cv = kf.empty(T, 6, B), kf.empty(T, 9, B)
    sx, sP, sl, six, siP = kf.empty(T, 6, B), kf.empty(T, 9, B), kf.empty(T, B), kf.empty(6, B), kf.empty(9, B)
    em = torch.empty(_lib.KF_EM_ROWS(3), B, dtype=torch.float64, device='cuda')
    st = torch.full((B,), 55, dtype=torch.int32, device='cuda')
    L = _lib.lib()

    def calls():
        s = kf._stream()
        _lib.check(L.kf_reset(kf.handle, _ptr(x0), s))
        _lib.check(L.kf_run_scores(kf.handle, T, 0.1, None, _ptr(u), _ptr(z), None, k, _ptr(tab), None, None, _ptr(tr),
                                   _ptr(cv), None, s))
        _lib.check(L.kf_smooth_run_em(kf.handle, T, 0.1, None, _ptr(u), _ptr(z), None, k, _ptr(tr), _ptr(cv), _ptr(ix),
                                      _ptr(iP), _ptr(sx), _ptr(sP), _ptr(sl), _ptr(st), _ptr(six), _ptr(siP), _ptr(tab),
                                      _ptr(em), s))

    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        calls()
    for _ in range(2):
        for t in (tr, cv, sx, sP, sl, six, siP, em):
            t.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        for name, got in (('x', sx), ('P', sP), ('logdet', sl), ('status', st), ('init_x', six), ('init_P', siP),
                          ('em', em)):
            assert np.array_equal(_np(got), eager[name]), name
    kf.close()
