"""kf_run_scores and kf_smooth_run_params (BatchedKF.run_scores, smooth_run(consts=...)): the
constant-velocity run under per-filter q_pos, q_vel and R, scored in the launch, and the RTS
backward pass under the same per-filter Q — needs an MI355X.

Seven parts.  (1) The filter is kf_run_rec: state, status, traj, cov and logdet with ==, consts
NULL and with a table (every column against kf_run_rec on a handle holding that column's values).
(2) The scores: lane-local (column f of a B = 130 launch == the one-filter launch), counts exact,
IMU rows 0, POS_SSE against the launch's own traj in longdouble.  (3) Accuracy by the project's
budget rule against tests/cv_score_oracle.py: per filter and float row E_gpu <= max(8 E_ref,
floor), E_ref the plain reference of the handle's precision on the same rounded inputs, the floor
propagated from extended_oracle.FLOOR through the row's formula.  (4) The smoother under a table.
(5) Failure isolation by data.  (6) Refusals.  (7) Graph capture.

The new instantiations' input ring is 4 deep (kf_run_rec's is 8), so T runs around both.

Measured on an MI355X over the 32 accuracy cases (each prints its figures with -s;
profiles/cv_scores/score_budget.log), the worst E_gpu / budget per row:
f64: gps_nis 0.00023 (2.1e-12 against a floor of 9.3e-9), gps_logdet_s 0.0023, pos_sse 0.00023;
f32: gps_nis 0.035, gps_logdet_s 0.124 (2.9e-5 against E_ref 3.0e-5), pos_sse 0.0093.  The floor
sets nearly every budget; with raw-UTM-size coordinates E_gpu and E_ref agree to three digits.
"""
import functools

import numpy as np
import pytest
import torch

import cv_score_oracle as cso
import cv_smoother_oracle as co
import error_budget_cases as ec
import extended_oracle as xo
import kfmi
from kfmi import _lib
from kfmi.engine import SCORE_ROWS as ROW
from kfmi.engine import _ptr
from oracle import ref_kf

pytestmark = pytest.mark.gpu
NP = {'f64': np.float64, 'f32': np.float32}
REC_T = (1, 3, 4, 5, 7, 8, 9, 17)    # around the rings of 4 (kf_run_scores) and 8 (kf_run_rec)
WAVE_B = (1, 63, 64, 65, 130)        # wave edges
SMOOTH_T = (1, 2, 4, 5, 6, 17)       # T - 1 backward steps around the ring of 4
LD = np.longdouble
SENTINEL = -777.0
# (q_pos, q_vel, r per axis), every value a float32 number so that both dtypes receive it exactly
SETS5 = [(0.0625, 0.5, (2.0, 3.0, 4.0)), (0.5, 0.125, (1.0, 1.0, 1.0)), (0.015625, 2.0, (9.0, 0.5, 3.0)),
         (1.0, 1.0, (4.0, 4.0, 0.25)), (0.25, 0.03125, (0.75, 6.0, 2.5))]
SETS7 = SETS5 + [(0.125, 0.25, (3.0, 3.0, 3.0)), (2.0, 0.0625, (1.5, 8.0, 5.0))]


def _np(t):
    return None if t is None else t.cpu().numpy()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sets(model, sets):
    d = co.axes(model)
    return [(qp, qv, tuple(r[:d])) for qp, qv, r in sets]


def _table(model, sets, B):
    return _dev(cso.table(model, _sets(model, sets), B))


def _params(model, s):
    """kf_params holding one set: the handle kf_run_rec needs to run that column."""
    d = co.axes(model)
    p = kfmi.default_params(model)
    p.q_pos, p.q_vel = s[0], s[1]
    for i in range(d):
        p.r[i * d + i] = s[2][i]
    return p


def _inputs(model, dtype, T, B, k, general, seed):
    """fast: scalar dt, u, no mask; general: dt_steps, a mask, u = None.  The track lies a few
    metres from the fixes' level; every third row is NaN and filter B // 2's column is all NaN."""
    d = co.axes(model)
    rng = np.random.default_rng(seed)
    npd = NP[dtype]
    x0 = np.zeros((2 * d, B), npd)
    x0[:d] = rng.uniform(-200, 200, (d, B))
    u = None if general else rng.normal(0, 0.3, (T, d, B)).astype(npd)
    z = (x0[None, :d] + rng.normal(0, 2.0, (T // k, d, B))).astype(npd)
    dts = rng.uniform(0.02, 0.3, T) if general else None
    mask = (rng.random((T // k, B)) < 0.7).astype(np.uint8) if general else None
    track = (x0[None, :d] + rng.normal(0, 2.0, (T, d, B))).astype(npd)
    track[::3] = np.nan
    track[:, :, B // 2] = np.nan
    return x0, u, (z if T // k else None), dts, mask, track


def _run_rec(kf, x0, u, z, dts, mask, k, T):
    kf.reset(x0)
    tr = kf.empty(T, kf.n, kf.batch)
    cv = kf.empty(T, 3 * kf.c, kf.batch)
    ld = kf.empty(T, kf.batch)
    _lib.check(_lib.lib().kf_run_rec(kf.handle, T, 0.1, _ptr(dts), _ptr(u), _ptr(z), _ptr(mask), k, _ptr(tr), _ptr(cv),
                                     _ptr(ld), kf._stream()))
    x, P = kf.state()
    return dict(traj=_np(tr), cov=_np(cv), logdet=_np(ld), x=_np(x), P=_np(P), status=_np(kf.status()))


def _run_scores(kf, x0, u, z, dts, mask, k, T, consts=None, track=None, scores=True, traj=True, cov=True, logdet=True):
    """kf_run_scores through the C API (T is explicit: T = 1 with k = 2 has no z to infer it from)."""
    kf.reset(x0)
    B = kf.batch
    sc = torch.full((_lib.KF_SCORE_ROWS, B), SENTINEL, dtype=torch.float64, device='cuda') if scores else None
    tr = kf.empty(T, kf.n, B) if traj else None
    cv = kf.empty(T, 3 * kf.c, B) if cov else None
    ld = kf.empty(T, B) if logdet else None
    _lib.check(_lib.lib().kf_run_scores(kf.handle, T, 0.1, _ptr(dts), _ptr(u), _ptr(z), _ptr(mask), k, _ptr(consts),
                                        _ptr(track), _ptr(sc), _ptr(tr), _ptr(cv), _ptr(ld), kf._stream()))
    x, P = kf.state()
    return dict(scores=_np(sc), traj=_np(tr), cov=_np(cv), logdet=_np(ld), x=_np(x), P=_np(P), status=_np(kf.status()))


FILTER = ('traj', 'cov', 'logdet', 'x', 'P', 'status')


def _same(a, b, names, where, cols=None):
    for n in names:
        x, y = a[n], b[n]
        if cols is not None:
            x, y = x[..., cols], y[..., cols]
        assert np.array_equal(x, y, equal_nan=True), (n,) + tuple(where)


# -- 1. the filter is kf_run_rec ------------------------------------------------------------------

@pytest.mark.parametrize('general', [False, True], ids=['fast', 'general'])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('model', ['cv2', 'cv3'])
def test_filter_is_run_rec_without_a_table(model, dtype, general):
    """consts NULL: state, status, traj, cov and logdet == kf_run_rec's with scores on and off and
    the track on and off, and with each record alone."""
    k = 3 if general else 2
    for B in WAVE_B:
        with kfmi.BatchedKF(model, B, dtype) as kf:
            for T in REC_T:
                x0, u, z, dts, mask, track = (_dev(a) for a in _inputs(model, dtype, T, B, k, general, 1000 * T + B))
                a = (kf, x0, u, z, dts, mask, k, T)
                ref = _run_rec(*a)
                assert (ref['status'] == 0).all()
                full = None
                for scores, tk in ((False, None), (True, None), (True, track)):
                    got = _run_scores(*a, track=tk, scores=scores)
                    _same(got, ref, FILTER, (T, B, scores, tk is not None))
                    full = got
                for only in ('traj', 'cov', 'logdet'):
                    got = _run_scores(*a, track=track, **{n: n == only for n in ('traj', 'cov', 'logdet')})
                    assert [n for n in ('traj', 'cov', 'logdet') if got[n] is not None] == [only]
                    _same(got, ref, (only, 'x', 'P', 'status'), (T, B, only))
                    assert np.array_equal(got['scores'], full['scores'], equal_nan=True), (T, B, only)


@pytest.mark.parametrize('general', [False, True], ids=['fast', 'general'])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('model', ['cv2', 'cv3'])
def test_filter_with_a_table_is_run_rec_on_a_handle_of_each_set(model, dtype, general):
    """A table of 5 distinct sets cycled over B = 130: every column == kf_run_rec on a handle whose
    kf_params hold that column's values, whatever the scores and the records."""
    k = 3 if general else 2
    B = 130
    sets = _sets(model, SETS5)
    tab = _table(model, SETS5, B)
    refs = [kfmi.BatchedKF(model, B, dtype, params=_params(model, s)) for s in sets]
    with kfmi.BatchedKF(model, B, dtype) as kf:
        for T in REC_T:
            x0, u, z, dts, mask, track = (_dev(a) for a in _inputs(model, dtype, T, B, k, general, 77 * T + 1))
            a = (x0, u, z, dts, mask, k, T)
            got = _run_scores(kf, *a, consts=tab, track=track)
            bare = _run_scores(kf, *a, consts=tab, scores=False)
            ld_only = _run_scores(kf, *a, consts=tab, track=track, traj=False, cov=False)
            assert (got['status'] == 0).all()
            for s, kr in enumerate(refs):
                ref = _run_rec(kr, *a)
                cols = np.arange(s, B, len(sets))
                _same(got, ref, FILTER, (T, s), cols)
                _same(bare, ref, FILTER, (T, s, 'bare'), cols)
                _same(ld_only, ref, ('logdet', 'x', 'P', 'status'), (T, s, 'logdet only'), cols)
            assert np.array_equal(ld_only['scores'], got['scores'], equal_nan=True), T
            if T >= 3:
                assert not np.array_equal(got['cov'][-1][:, 0], got['cov'][-1][:, 1])     # the sets differ
    for kr in refs:
        kr.close()


# -- 2. the scores --------------------------------------------------------------------------------

@pytest.mark.parametrize('general', [False, True], ids=['fast', 'general'])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('model', ['cv2', 'cv3'])
def test_scores_are_lane_local_and_counts_exact(model, dtype, general):
    """Column f of a B = 130 launch == the one-filter launch, records on and off; counts exact
    against the mask and the track's NaN rows; IMU rows exactly 0; POS_SSE against the same launch's
    own traj in longdouble: |delta| <= (3 pos_n + 8) 2^-53 sse (each scored step adds d squares and
    one running sum, every one of them a rounding of at most 2^-53 of the sum so far, and the
    difference of the two doubles one more per term: under 3 per step and a few for the ends)."""
    k = 3 if general else 2
    B, d = 130, co.axes(model)
    tab = _table(model, SETS5, B)
    with kfmi.BatchedKF(model, B, dtype) as kf, kfmi.BatchedKF(model, 1, dtype) as k1:
        for T in REC_T:
            x0, u, z, dts, mask, track = (_dev(a) for a in _inputs(model, dtype, T, B, k, general, 31 * T + 5))
            a = (x0, u, z, dts, mask, k, T)
            got = _run_scores(kf, *a, consts=tab, track=track)
            norec = _run_scores(kf, *a, consts=tab, track=track, traj=False, cov=False, logdet=False)
            assert np.array_equal(got['scores'], norec['scores']), T
            sc = got['scores']
            assert np.isfinite(sc).all() and (got['status'] == 0).all()
            for f in (0, 63, 64, 129):
                col = lambda t: None if t is None else t[..., f:f + 1].contiguous()  # noqa: E731
                one = _run_scores(k1, col(x0), col(u), col(z), dts, col(mask), k, T, consts=col(tab), track=col(track))
                assert np.array_equal(one['scores'][:, 0], sc[:, f]), (T, f)
            U = T // k
            n_fix = np.full(B, U) if mask is None else (_np(mask)[:U] != 0).sum(axis=0)
            assert np.array_equal(sc[ROW['gps_n']], n_fix), T
            n_pos = np.full(B, T - len(range(0, T, 3)))
            n_pos[B // 2] = 0
            assert np.array_equal(sc[ROW['pos_n']], n_pos), T
            assert sc[ROW['pos_sse'], B // 2] == 0.0
            assert not sc[[ROW['imu_n'], ROW['imu_nis'], ROW['imu_logdet_s']]].any()
            assert not sc[[ROW['gps_nis'], ROW['gps_logdet_s']]][:, n_fix == 0].any()
            tk = _np(track).astype(LD)
            e = got['traj'][:, :d].astype(LD) - tk
            have = ~np.isnan(tk).any(axis=1)
            sse = np.where(have, (e * e).sum(axis=1), 0).sum(axis=0)
            delta = np.abs(sc[ROW['pos_sse']].astype(LD) - sse)
            bound = (3 * n_pos + 8) * LD(2.0) ** -53 * sse
            assert (delta <= bound).all(), (T, float((delta / np.maximum(bound, LD(1e-300))).max()))
            # without a track both rows are 0, and the innovation rows do not move
            nt = _run_scores(kf, *a, consts=tab)['scores']
            assert not nt[[ROW['pos_n'], ROW['pos_sse']]].any() and np.array_equal(nt[:6], sc[:6])


def test_T0_zeroes_the_table():
    with kfmi.BatchedKF('cv3', 65, 'f64') as kf:
        sc = torch.full((_lib.KF_SCORE_ROWS, 65), SENTINEL, dtype=torch.float64, device='cuda')
        before = [_np(t) for t in kf.state()]
        rc = _lib.lib().kf_run_scores(kf.handle, 0, 0.1, None, None, None, None, 1, None, None, _ptr(sc), None, None,
                                      None, kf._stream())
        assert rc == _lib.KF_OK, _lib.last_error()
        assert not _np(sc).any()
        assert all(np.array_equal(a, _np(b)) for a, b in zip(before, kf.state()))


def test_engine_run_scores_and_nll():
    """BatchedKF.run_scores is the C call; innovation_nll is its formula on the table."""
    model, T, B, k = 'cv3', 9, 65, 2
    x0, u, z, dts, mask, track = (_dev(a) for a in _inputs(model, 'f64', T, B, k, False, 3))
    tab = _table(model, SETS5, B)
    with kfmi.BatchedKF(model, B, 'f64') as kf:
        raw = _run_scores(kf, x0, u, z, dts, mask, k, T, consts=tab, track=track)
        kf.reset(x0)
        sr = kf.run_scores(u, z, consts=tab, track=track, dt=0.1, update_every=k, traj=True, cov=True, logdet=True)
        assert np.array_equal(_np(sr.scores), raw['scores'])
        for n in ('traj', 'cov', 'logdet'):
            assert np.array_equal(_np(getattr(sr, n)), raw[n]), n
        kf.reset(x0)
        assert kf.run_scores(u, z, dt=0.1, update_every=k).traj is None
        nll = kfmi.innovation_nll(sr.scores, model, 'gps')
        s = raw['scores']
        want = 0.5 * (s[ROW['gps_nis']] + s[ROW['gps_logdet_s']] + s[ROW['gps_n']] * 3 * np.log(2 * np.pi))
        np.testing.assert_allclose(_np(nll), want, rtol=1e-15)


# -- 3. accuracy ----------------------------------------------------------------------------------

CASES = [(m, r, k, off) for m in ('cv2', 'cv3') for r in 'AB' for k in (1, 5) for off in (False, True)]
CASE_IDS = [f'{m}-{r}-k{k}{"-utm" if off else ""}' for m, r, k, off in CASES]


@functools.lru_cache(maxsize=None)
def _accuracy_case(model, regime, k, offset):
    """cv_case's inputs, the 7-set table cycled over the filters and a seeded track within a few
    metres of the fixes (each step against the fix its update interval ends with)."""
    c = ec.cv_case(model, regime, k, offset)
    d = co.axes(model)
    rng = np.random.default_rng(ec._seed('cv-scores', model, regime, k, offset))
    U = ec.CV_T // k
    track = c['z'][np.minimum(np.arange(ec.CV_T) // k, U - 1)] + rng.normal(0, 2.0, (ec.CV_T, d, ec.B))
    return c, cso.table(model, _sets(model, SETS7), ec.B), track


@functools.lru_cache(maxsize=None)
def _accuracy_oracle(model, regime, k, offset, dtype):
    c, tab, track = _accuracy_case(model, regime, k, offset)
    a = (model, c['x0'], c['dt_steps'], c['u'], c['z'], k)
    kw = dict(consts=tab, track=track, dtype=dtype)
    truth = cso.run(*a, arith='longdouble', floors=True, **kw)
    plain = cso.run(*a, arith=dtype, **kw)
    return truth, plain


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('model,regime,k,offset', CASES, ids=CASE_IDS)
def test_scores_within_budget(model, regime, k, offset, dtype):
    """Per filter and float row: E_gpu <= max(8 E_ref, floor) against the longdouble truth."""
    c, tab, track = _accuracy_case(model, regime, k, offset)
    truth, plain = _accuracy_oracle(model, regime, k, offset, dtype)
    M = xo.Model(model)
    npd = NP[dtype]
    tag = f'{model}/{regime}/k{k}{"/utm" if offset else ""}/{dtype}'
    with kfmi.BatchedKF(model, ec.B, dtype) as kf:
        kf.set_state(np.ascontiguousarray(c['x0'].T).astype(npd),
                     ref_kf.tri_pack(np.repeat(M.P0()[None], ec.B, 0)).astype(npd))
        sr = kf.run_scores(_dev(c['u'].astype(npd)), _dev(c['z'].astype(npd)), consts=_dev(tab),
                           track=_dev(track.astype(npd)), dt_steps=_dev(c['dt_steps']), update_every=k)
        assert (_np(kf.status()) == 0).all()          # the precondition
        sc = _np(sr.scores)
    assert np.array_equal(sc[ROW['gps_n']], truth['scores'][0]) and np.array_equal(sc[ROW['pos_n']], truth['scores'][6])
    fails = []
    for i in cso.FLOAT_ROWS:
        t = truth['scores'][i]
        e_gpu = np.abs(sc[i].astype(LD) - t).astype(np.float64)
        e_ref = np.abs(plain['scores'][i].astype(LD) - t).astype(np.float64)
        budget = np.maximum(8.0 * e_ref, truth['floor'][i].astype(np.float64))
        ratio = e_gpu / budget
        f = int(np.argmax(ratio))
        print(f'cv_score_budget {tag} {cso.ROWS[i]:13s} worst filter {f:2d} truth {float(t[f]): .9e} E_gpu {e_gpu[f]:.3e} '
              f'E_ref {e_ref[f]:.3e} floor {float(truth["floor"][i][f]):.3e} budget {budget[f]:.3e} '
              f'E_gpu/budget {ratio[f]:.3g}')
        if not (e_gpu <= budget).all():
            fails.append((cso.ROWS[i], f, e_gpu[f], budget[f]))
    assert not fails, fails


# -- 4. the smoother under a table ----------------------------------------------------------------

@pytest.mark.parametrize('general', [False, True], ids=['fast', 'general'])
@pytest.mark.parametrize('model', ['cv2', 'cv3'])
def test_smoother_with_a_table(model, general):
    """Column f == kf_smooth_run on a handle of that set; consts NULL == kf_smooth_run; in place ==
    out of place."""
    k = 3 if general else 2
    B = 130
    sets = _sets(model, SETS5)
    tab = _table(model, SETS5, B)
    refs = [kfmi.BatchedKF(model, B, 'f64', params=_params(model, s)) for s in sets]
    with kfmi.BatchedKF(model, B, 'f64') as kf:
        for T in SMOOTH_T:
            x0, u, z, dts, mask, _ = (_dev(a) for a in _inputs(model, 'f64', T, B, k, general, 13 * T + 2))
            rec = _run_scores(kf, x0, u, z, dts, mask, k, T, consts=tab, scores=False)
            tr, cv = _dev(rec['traj']), _dev(rec['cov'])
            kw = dict(u=u, dt=0.1, dt_steps=dts, x=True, P=True, logdet=True)
            got = {n: _np(v) for n, v in kf.smooth_run(tr, cv, consts=tab, **kw)._asdict().items()}
            assert (got['status'] == 0).all() and all(np.isfinite(got[n]).all() for n in ('x', 'P', 'logdet'))
            for s, kr in enumerate(refs):
                ref = {n: _np(v) for n, v in kr.smooth_run(tr, cv, **kw)._asdict().items()}
                cols = np.arange(s, B, len(sets))
                _same(got, ref, ('x', 'P', 'logdet', 'status'), (T, s), cols)
            if T > 2:
                assert not np.array_equal(got['P'][0][:, 0], got['P'][0][:, 1])
            # consts NULL through the new entry point == kf_smooth_run
            plain = {n: _np(v) for n, v in kf.smooth_run(tr, cv, **kw)._asdict().items()}
            outs = [kf.empty(T, kf.n, B), kf.empty(T, 3 * kf.c, B), kf.empty(T, B),
                    torch.full((B,), 55, dtype=torch.int32, device='cuda')]
            _lib.check(_lib.lib().kf_smooth_run_params(kf.handle, T, 0.1, _ptr(dts), _ptr(u), _ptr(tr), _ptr(cv),
                                                       *[_ptr(o) for o in outs], None, kf._stream()))
            for n, o in zip(('x', 'P', 'logdet', 'status'), outs):
                assert np.array_equal(_np(o), plain[n]), (n, T)
            trc, cvc = tr.clone(), cv.clone()
            inp = kf.smooth_run(trc, cvc, consts=tab, inplace=True, **kw)
            assert inp.x.data_ptr() == trc.data_ptr() and inp.P.data_ptr() == cvc.data_ptr()
            for n in ('x', 'P', 'logdet'):
                assert np.array_equal(_np(getattr(inp, n)), got[n]), (n, T)
        # run_smoothed(consts) is the two calls
        T = 9
        x0, u, z, dts, mask, _ = (_dev(a) for a in _inputs(model, 'f64', T, B, k, False, 9))
        rec = _run_scores(kf, x0, u, z, None, None, k, T, consts=tab, scores=False)
        sm = kf.smooth_run(_dev(rec['traj']), _dev(rec['cov']), u=u, dt=0.1, consts=tab)
        kf.reset(x0)
        rs = kf.run_smoothed(u, z, dt=0.1, update_every=k, consts=tab)
        assert np.array_equal(_np(rs.traj), rec['traj']) and np.array_equal(_np(rs.cov), rec['cov'])
        assert torch.equal(rs.smoothed.x, sm.x)
    for kr in refs:
        kr.close()


# -- 5. failure isolation -------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_failure_is_per_filter(dtype):
    """One column's r = -1e9 (data, not a fault): that filter's first innovation pivot is negative, so
    it gets KF_ENOTSPD, NaN state and NaN float rows while its counts still count; every neighbour ==
    the clean run."""
    model, T, B, k, f = 'cv3', 17, 130, 2, 70
    x0, u, z, dts, mask, track = (_dev(a) for a in _inputs(model, dtype, T, B, k, False, 21))
    tab = _table(model, SETS5, B)
    bad_tab = tab.clone()
    bad_tab[_lib.KF_CV_CONST_R + 1, f] = -1.0e9
    with kfmi.BatchedKF(model, B, dtype) as kf:
        a = (kf, x0, u, z, dts, mask, k, T)
        clean = _run_scores(*a, consts=tab, track=track)
        bad = _run_scores(*a, consts=bad_tab, track=track)
    others = np.arange(B) != f
    assert bad['status'][f] == _lib.KF_ENOTSPD and (bad['status'][others] == 0).all()
    _same(bad, clean, FILTER + ('scores',), ('neighbours',), others)
    for n in ('traj', 'cov', 'logdet'):
        assert np.isnan(bad[n][k - 1:, ..., f]).all(), n              # from the first update on
        assert np.array_equal(bad[n][:k - 1, ..., f], clean[n][:k - 1, ..., f]), n
    assert np.isnan(bad['x'][:, f]).all()
    sc = bad['scores'][:, f]
    assert np.isnan(sc[[ROW['gps_nis'], ROW['gps_logdet_s'], ROW['pos_sse']]]).all()
    assert sc[ROW['gps_n']] == T // k and sc[ROW['pos_n']] == clean['scores'][ROW['pos_n'], f] > 0
    assert not sc[[ROW['imu_n'], ROW['imu_nis'], ROW['imu_logdet_s']]].any()


# -- 6. refusals ----------------------------------------------------------------------------------

def _raw(kf, T, d, td, consts=None, track=False, scores=True, k=1):
    """kf_run_scores with sentinel-filled outputs: (rc, outputs)."""
    B = kf.batch
    u = torch.zeros(max(T, 1), d, B, dtype=td, device='cuda')
    z = torch.zeros(max(T, 1), d, B, dtype=td, device='cuda')
    tk = torch.zeros(max(T, 1), d, B, dtype=td, device='cuda') if track else None
    n = max(T, 1)
    outs = [torch.full((n, 2 * d, B), SENTINEL, dtype=td, device='cuda'),
            torch.full((n, 3 * d, B), SENTINEL, dtype=td, device='cuda'),
            torch.full((n, B), SENTINEL, dtype=td, device='cuda')]
    sc = torch.full((_lib.KF_SCORE_ROWS, B), SENTINEL, dtype=torch.float64, device='cuda')
    rc = _lib.lib().kf_run_scores(kf.handle, T, 0.1, None, _ptr(u), _ptr(z), None, k, _ptr(consts), _ptr(tk),
                                  _ptr(sc) if scores else None, *[_ptr(o) for o in outs], kf._stream())
    torch.cuda.synchronize()
    return rc, outs + [sc]


def _untouched(outs):
    return all(bool((o == SENTINEL).all()) for o in outs)


@pytest.mark.parametrize('why', ['reference_model', 'offblock_P', 'nondiagonal_R', 'track_without_scores', 'negative_T'])
def test_refusals(why):
    B, T = 8, 5
    if why == 'reference_model':
        with kfmi.BatchedKF('ref15', B, 'f64') as kf:
            rc, outs = _raw(kf, T, 3, torch.float64)
            assert rc == _lib.KF_EINVAL and 'kf_run_scores' in _lib.last_error() and _untouched(outs)
            with pytest.raises(kfmi.KFError) as e:
                kf.run_scores(None, np.zeros((T, 3, B)), dt=0.1)
            assert e.value.code == _lib.KF_EINVAL
        return
    params = kfmi.default_params('cv3')
    if why == 'nondiagonal_R':
        params.r[1] = params.r[3] = 0.5
    with kfmi.BatchedKF('cv3', B, 'f64', params=params) as kf:
        kf.reset()
        x, P = kf.state()
        if why == 'offblock_P':
            P[1] = 0.25                                  # P[0][1]: couples axes 0 and 1
            kf.set_state(x, P)
        before = [_np(t) for t in kf.state()]
        rc, outs = _raw(kf, -1 if why == 'negative_T' else T, 3, torch.float64, track=why == 'track_without_scores',
                        scores=why != 'track_without_scores')
        assert rc == _lib.KF_EINVAL and 'kf_run_scores' in _lib.last_error(), _lib.last_error()
        assert _untouched(outs)
        assert all(np.array_equal(a, _np(b)) for a, b in zip(before, kf.state()))
        assert (_np(kf.status()) == 0).all()
        if why == 'nondiagonal_R':
            # with a table the handle's R is not read: accepted, and the run is the table's
            tab = _table('cv3', SETS5, B)
            rc, outs = _raw(kf, T, 3, torch.float64, consts=tab, track=True)
            assert rc == _lib.KF_OK, _lib.last_error()
            assert all(bool(torch.isfinite(o).all()) and not bool((o == SENTINEL).any()) for o in outs)
            with kfmi.BatchedKF('cv3', B, 'f64') as kd:
                kd.reset()
                rc, want = _raw(kd, T, 3, torch.float64, consts=tab, track=True)
                assert rc == _lib.KF_OK
            assert all(torch.equal(a, b) for a, b in zip(outs, want))


# -- 7. graph capture -----------------------------------------------------------------------------

def test_graph_capture_replays_the_eager_bits():
    """kf_reset + kf_run_scores + kf_smooth_run_params captured into one graph (nothing allocates
    or synchronises) and replayed twice == the eager calls."""
    model, T, B, k = 'cv3', 9, 130, 2
    x0, u, z, _, _, track = (_dev(a) for a in _inputs(model, 'f64', T, B, k, False, 11))
    tab = _table(model, SETS5, B)
    with kfmi.BatchedKF(model, B, 'f64') as kf:
        eager = _run_scores(kf, x0, u, z, None, None, k, T, consts=tab, track=track)
        sm = {n: _np(v) for n, v in kf.smooth_run(_dev(eager['traj']), _dev(eager['cov']), u=u, dt=0.1, x=True, P=True,
                                                  logdet=True, consts=tab)._asdict().items()}
    kf = kfmi.BatchedKF(model, B, 'f64')
    tr, cv, ld = kf.empty(T, 6, B), kf.empty(T, 9, B), kf.empty(T, B)
    sx, sP, sl = kf.empty(T, 6, B), kf.empty(T, 9, B), kf.empty(T, B)
    sc = torch.empty(_lib.KF_SCORE_ROWS, B, dtype=torch.float64, device='cuda')
    st = torch.full((B,), 55, dtype=torch.int32, device='cuda')
    L = _lib.lib()

    def calls():
        s = kf._stream()
        _lib.check(L.kf_reset(kf.handle, _ptr(x0), s))
        _lib.check(L.kf_run_scores(kf.handle, T, 0.1, None, _ptr(u), _ptr(z), None, k, _ptr(tab), _ptr(track), _ptr(sc),
                                   _ptr(tr), _ptr(cv), _ptr(ld), s))
        _lib.check(L.kf_smooth_run_params(kf.handle, T, 0.1, None, _ptr(u), _ptr(tr), _ptr(cv), _ptr(sx), _ptr(sP),
                                          _ptr(sl), _ptr(st), _ptr(tab), s))

    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        calls()
    for _ in range(2):
        for t in (tr, cv, ld, sx, sP, sl, sc):
            t.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        for name, got, want in (('traj', tr, eager['traj']), ('cov', cv, eager['cov']), ('logdet', ld, eager['logdet']),
                                ('scores', sc, eager['scores']), ('sm_x', sx, sm['x']), ('sm_P', sP, sm['P']),
                                ('sm_logdet', sl, sm['logdet']), ('sm_status', st, sm['status'])):
            assert np.array_equal(_np(got), want), name
    x, P = kf.state()
    assert np.array_equal(_np(x), eager['x']) and np.array_equal(_np(P), eager['P'])
    kf.close()
