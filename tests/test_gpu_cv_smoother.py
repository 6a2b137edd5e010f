"""kf_run_rec and kf_smooth_run (BatchedKF.run_rec / smooth_run / run_smoothed): the fused
constant-velocity run with a covariance record, and the RTS backward pass over it — needs an
MI355X.

Four parts.  kf_run_rec against kf_run with == (both dtypes, the fast and the general shape, the
input ring's and the wave's edge sizes).  Accuracy, judged as the filter kernels' is
(tests/test_gpu_error_budget.py): the error per group against the longdouble truth of
tests/cv_smoother_oracle.py within extended_oracle.budget(E_ref, 'f64') (8 x E_ref, floor 2^-40),
E_ref the plain NumPy float64 smoother's own error on the same inputs; (a) end to end, run_rec then
smooth_run, against forward + backward in longdouble, E_ref from forward + backward in float64;
(b) the backward pass alone on the truth's filtered record rounded to float64, against the
longdouble backward pass over that same rounded record, E_ref from the float64 backward pass over
it (the rule of extended_oracle: truth and reference see the inputs the kernel receives).  Bits:
everything that should be the same bits is compared with ==.  Failure isolation and refusals.

Measured on an MI355X over the 24 accuracy cases (each prints its figures with -s;
profiles/cv_smoother/smoother_budget.log): the worst E_gpu / budget is 0.001 (pos), 0.176 (vel:
1.4e-10 against E_ref 9.6e-11), 0.130 (P: 1.5e-13 against 1.5e-13) and 0.064 (log det: 3.0e-13
against 2.8e-13); P_f / P_s reaches 3,982.

kf_run_rec is compared with the kf_run call that writes both of its records.  In fp64 kf_run with a
record missing is not bit for bit kf_run with both (it takes another kernel, whose Q dt + P is one
fma); kf_run_rec's bits do not depend on which records are asked for.
"""
import functools

import numpy as np
import pytest
import torch

import cv_smoother_oracle as co
import error_budget_cases as ec
import extended_oracle as xo
import kfmi
from kfmi import _lib
from kfmi.engine import _ptr
from oracle import ref_kf

pytestmark = pytest.mark.gpu
NP = {'f64': np.float64, 'f32': np.float32}
DEPTH_REC, DEPTH_SMOOTH = 8, 4       # the kernels' input rings (cv_rec_kernel, KF_CV_SMOOTH_DEPTH)
REC_T = (1, 7, 8, 9, 17)             # around the forward ring of 8
WAVE_B = (1, 63, 64, 65, 130)        # wave edges
SMOOTH_T = (1, 2, 4, 5, 6, 17)       # T - 1 backward steps around the ring of 4: 0, 1, 3, 4, 5, 16


def _np(t):
    return None if t is None else t.cpu().numpy()


def _tri(n, i, j):
    return i * n - i * (i - 1) // 2 + (j - i)


def _block_rows(d):
    """rows of the tri-packed P [n (n + 1) / 2, B] that the covariance record holds, in its order"""
    n = 2 * d
    return [r for i in range(d) for r in (_tri(n, i, i), _tri(n, i, d + i), _tri(n, d + i, d + i))]


def _inputs(model, dtype, T, B, k, general, seed):
    d = co.axes(model)
    rng = np.random.default_rng(seed)
    npd = NP[dtype]
    x0 = np.zeros((2 * d, B), npd)
    x0[:d] = rng.uniform(-200, 200, (d, B))
    u = None if general else rng.normal(0, 0.3, (T, d, B)).astype(npd)
    z = (x0[None, :d] + rng.normal(0, 2.0, (T // k, d, B))).astype(npd)
    dts = rng.uniform(0.02, 0.3, T) if general else None
    mask = None
    if general:
        mask = (rng.random((T // k, B)) < 0.7).astype(np.uint8)
    return x0, u, z, dts, mask


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _kf_run(kf, T, x0, u, z, dts, mask, k, traj=True, logdet=True):
    """kf_run through the C API (BatchedKF.run cannot pass u = None)."""
    kf.reset(x0)
    tr = kf.empty(T, kf.n, kf.batch) if traj else None
    ld = kf.empty(T, kf.batch) if logdet else None
    rc = _lib.lib().kf_run(kf.handle, T, 0.1, _ptr(dts), _ptr(u), _ptr(z), _ptr(mask), k, _ptr(tr), _ptr(ld),
                           kf._stream())
    assert rc == _lib.KF_OK, _lib.last_error()
    x, P = kf.state()
    return _np(tr), _np(ld), _np(x), _np(P), _np(kf.status())


def _kf_run_rec(kf, T, x0, u, z, dts, mask, k, traj=True, cov=True, logdet=True):
    kf.reset(x0)
    tr, cv, ld = kf.run_rec(u, z, dt=0.1, dt_steps=dts, update_every=k, mask=mask, traj=traj, cov=cov, logdet=logdet)
    x, P = kf.state()
    return _np(tr), _np(cv), _np(ld), _np(x), _np(P), _np(kf.status())


@pytest.mark.parametrize('general', [False, True], ids=['fast', 'general'])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('model', ['cv2', 'cv3'])
def test_run_rec_equals_run(model, dtype, general):
    """State, status, traj and logdet of kf_run_rec == kf_run's, on kf_run's default kernel and on
    its general kernel; cov[T - 1] == the same-axis entries of kf_get_state's P; cov[t] for a mid t
    == those of a kf_run of t + 1 steps; each record alone == all three.  fast: scalar dt, u, no
    mask, a fix every 2nd step; general: dt_steps, a mask, u = None, a fix every 3rd step."""
    d = co.axes(model)
    k = 3 if general else 2
    rows = _block_rows(d)
    for B in WAVE_B:
        kf = kfmi.BatchedKF(model, B, dtype)
        kg = kfmi.BatchedKF(model, B, dtype, options={'cv_kernel': 'general'})
        for T in REC_T:
            x0, u, z, dts, mask = (_dev(a) for a in _inputs(model, dtype, T, B, k, general, 1000 * T + B))
            if T // k == 0:
                z = None
            tr, cv, ld, x, P, st = _kf_run_rec(kf, T, x0, u, z, dts, mask, k)
            for other in (kf, kg):
                tr0, ld0, x0_, P0_, st0 = _kf_run(other, T, x0, u, z, dts, mask, k)
                for name, a, b in (('traj', tr, tr0), ('logdet', ld, ld0), ('x', x, x0_), ('P', P, P0_),
                                   ('status', st, st0)):
                    assert np.array_equal(a, b), (name, T, B)
            assert (st == 0).all() and np.isfinite(cv).all()
            assert np.array_equal(cv[T - 1], P[rows]), (T, B)
            t = T // 2                      # cov[t] == the state of a run of t + 1 steps
            U1 = (t + 1) // k
            _, _, _, Pt, _ = _kf_run(kf, t + 1, x0, None if u is None else u[:t + 1].contiguous(),
                                     z[:U1].contiguous() if U1 else None, None if dts is None else dts[:t + 1].contiguous(),
                                     mask[:U1].contiguous() if (mask is not None and U1) else None, k)
            assert np.array_equal(cv[t], Pt[rows]), (T, B, t)
            for only in ('traj', 'cov', 'logdet'):
                a = _kf_run_rec(kf, T, x0, u, z, dts, mask, k, **{n: n == only for n in ('traj', 'cov', 'logdet')})
                got = dict(traj=a[0], cov=a[1], logdet=a[2])
                assert [n for n in got if got[n] is not None] == [only]
                assert np.array_equal(got[only], dict(traj=tr, cov=cv, logdet=ld)[only]), (only, T, B)
                assert np.array_equal(a[3], x) and np.array_equal(a[4], P) and np.array_equal(a[5], st), (only, T, B)
        kf.close()
        kg.close()


# -- accuracy -------------------------------------------------------------------------------------

CASES = [(m, r, k, off) for m in ('cv2', 'cv3') for r in 'AB' for (k, off) in ((1, False), (5, False), (5, True))]
CASE_IDS = [f'{m}-{r}-k{k}{"-utm" if off else ""}' for m, r, k, off in CASES]


@functools.lru_cache(maxsize=None)
def _oracle(model, regime, k, offset):
    """The case's truth and plain float64 legs, computed once: end to end (filtered and smoothed)
    and the backward pass alone over the truth's filtered record rounded to float64."""
    c = ec.cv_case(model, regime, k, offset)
    a = (model, c['x0'], c['dt_steps'], c['u'], c['z'], k)
    filt, sm = co.smoothed(*a)
    _, sm64 = co.smoothed(*a, arith='f64')
    rx, rP = filt['x'].astype(np.float64), filt['P'].astype(np.float64)
    b_truth = co.backward(model, rx, rP, c['dt_steps'], c['u'])
    b_plain = co.backward(model, rx, rP, c['dt_steps'], c['u'], arith='f64')
    return dict(sm=sm, sm64=sm64, rx=rx, rP=rP, b_truth=b_truth, b_plain=b_plain,
                ratio=float((np.diagonal(filt['P'], axis1=2, axis2=3) / np.diagonal(sm['P'], axis1=2, axis2=3)).max()))


def _judge(route, regime, got, truth, plain, model):
    groups = xo.Model(model).groups
    e_ref = xo.errors(plain, truth, groups)
    e_gpu = xo.errors(got, truth, groups)
    over = ec.report(route, regime, 'f64', e_gpu, e_ref, xo.budget(e_ref, 'f64'))
    assert not over, {g: f'E_gpu {a:.3e} > budget {b:.3e}' for g, (a, b) in over.items()}


def _record(sm, model):
    return dict(x=_np(sm.x).transpose(0, 2, 1), P=co.unpack_cov(model, _np(sm.P)), logdet=_np(sm.logdet))


@pytest.mark.parametrize('model,regime,k,offset', CASES, ids=CASE_IDS)
def test_end_to_end_within_budget(model, regime, k, offset):
    """(a) run_rec -> smooth_run on error_budget_cases.cv_case's inputs (T = 64, B = 70)."""
    c, o = ec.cv_case(model, regime, k, offset), _oracle(model, regime, k, offset)
    M = xo.Model(model)
    with kfmi.BatchedKF(model, ec.B, 'f64') as kf:
        kf.set_state(np.ascontiguousarray(c['x0'].T), ref_kf.tri_pack(np.repeat(M.P0()[None], ec.B, 0)))
        u, dts = _dev(c['u']), _dev(c['dt_steps'])
        tr, cv, _ = kf.run_rec(u, _dev(c['z']), dt_steps=dts, update_every=k, logdet=False)
        assert (_np(kf.status()) == 0).all()          # the precondition
        sm = kf.smooth_run(tr, cv, u=u, dt_steps=dts, x=True, P=True, logdet=True)
        assert (_np(sm.status) == 0).all()
        print(f'cv-smoother | {model}/{regime}/k{k}{"/utm" if offset else ""} | max P_f / P_s {o["ratio"]:.0f}')
        _judge(f'{model}/run_rec+smooth_run/k{k}{"/utm" if offset else ""}', regime, _record(sm, model), o['sm'],
               o['sm64'], model)


@pytest.mark.parametrize('model,regime,k,offset', CASES, ids=CASE_IDS)
def test_backward_pass_alone_within_budget(model, regime, k, offset):
    """(b) smooth_run on the truth's filtered record rounded to float64."""
    c, o = ec.cv_case(model, regime, k, offset), _oracle(model, regime, k, offset)
    with kfmi.BatchedKF(model, ec.B, 'f64') as kf:
        fx = np.ascontiguousarray(o['rx'].transpose(0, 2, 1))
        sm = kf.smooth_run(fx, co.pack_cov(model, o['rP']), u=c['u'], dt_steps=c['dt_steps'], x=True, P=True, logdet=True)
        assert (_np(sm.status) == 0).all()
        _judge(f'{model}/smooth_run/k{k}{"/utm" if offset else ""}', regime, _record(sm, model), o['b_truth'],
               o['b_plain'], model)


# -- bits -----------------------------------------------------------------------------------------

def _filtered(model, T, B, general, seed=7):
    """A filtered record from run_rec: (kf, traj, cov, u, dts) on the device."""
    k = 3 if general else 2
    x0, u, z, dts, mask = (_dev(a) for a in _inputs(model, 'f64', T, B, k, general, seed))
    if not general:
        dts = None
    kf = kfmi.BatchedKF(model, B, 'f64')
    kf.reset(x0)
    tr, cv, _ = kf.run_rec(u, z if T // k else None, dt=0.1, dt_steps=dts, update_every=k, mask=mask, logdet=False)
    return kf, tr, cv, u, dts


def _all(sm):
    return {n: _np(v) for n, v in sm._asdict().items()}


@pytest.mark.parametrize('general', [False, True], ids=['fast', 'general'])
@pytest.mark.parametrize('model', ['cv2', 'cv3'])
def test_smooth_run_bits(model, general):
    """Row T - 1 == the filtered row; T = 1 copies it; in place == out of place; each output alone
    == all; filter f of a B = 130 call == the same filter alone at B = 1."""
    B = 130
    for T in SMOOTH_T:
        kf, tr, cv, u, dts = _filtered(model, T, B, general)
        kw = dict(u=u, dt=0.1, dt_steps=dts)
        full = _all(kf.smooth_run(tr, cv, x=True, P=True, logdet=True, **kw))
        assert (full['status'] == 0).all() and all(np.isfinite(full[n]).all() for n in ('x', 'P', 'logdet'))
        assert np.array_equal(full['x'][T - 1], _np(tr)[T - 1]) and np.array_equal(full['P'][T - 1], _np(cv)[T - 1])
        if T > 2:
            assert not np.array_equal(full['P'][0], _np(cv)[0])           # the pass did something
        for only in ('x', 'P', 'logdet'):
            one = _all(kf.smooth_run(tr, cv, **{n: n == only for n in ('x', 'P', 'logdet')}, **kw))
            assert np.array_equal(one[only], full[only]), (only, T)
            assert np.array_equal(one['status'], full['status'])
        nos = kf.smooth_run(tr, cv, x=True, status=False, **kw)
        assert nos.status is None and np.array_equal(_np(nos.x), full['x'])
        for f in (0, 64, 129):
            with kfmi.BatchedKF(model, 1, 'f64') as k1:
                one = _all(k1.smooth_run(tr[:, :, f:f + 1].contiguous(), cv[:, :, f:f + 1].contiguous(),
                                         u=None if u is None else u[:, :, f:f + 1].contiguous(), dt=0.1, dt_steps=dts,
                                         x=True, P=True, logdet=True))
            for n in ('x', 'P', 'logdet'):
                assert np.array_equal(one[n][..., 0], full[n][..., f]), (n, T, f)
        trc, cvc = tr.clone(), cv.clone()
        inp = kf.smooth_run(trc, cvc, x=True, P=True, logdet=True, inplace=True, **kw)
        assert inp.x.data_ptr() == trc.data_ptr() and inp.P.data_ptr() == cvc.data_ptr()
        for n in ('x', 'P', 'logdet'):
            assert np.array_equal(_np(getattr(inp, n)), full[n]), (n, T)
        kf.close()


def test_run_smoothed_is_run_rec_then_smooth_run():
    kf, tr, cv, u, dts = _filtered('cv3', 9, 65, False)
    x0, u, z, _, _ = (_dev(a) for a in _inputs('cv3', 'f64', 9, 65, 2, False, 7))
    sm = kf.smooth_run(tr, cv, u=u, dt=0.1)
    kf.reset(x0)
    rs = kf.run_smoothed(u, z, dt=0.1, update_every=2)
    assert torch.equal(rs.traj, tr) and torch.equal(rs.cov, cv) and torch.equal(rs.smoothed.x, sm.x)
    kf.close()


def test_graph_capture_replays_the_eager_bits():
    """kf_reset + kf_run_rec + kf_smooth_run captured into one graph (nothing allocates or
    synchronises) and replayed twice == the eager calls."""
    T, B, k = 9, 130, 2
    x0, u, z, _, _ = (_dev(a) for a in _inputs('cv3', 'f64', T, B, k, False, 11))
    kf = kfmi.BatchedKF('cv3', B, 'f64')
    eager = _kf_run_rec(kf, T, x0, u, z, None, None, k)
    sm = _all(kf.smooth_run(_dev(eager[0]), _dev(eager[1]), u=u, dt=0.1, x=True, P=True, logdet=True))
    kf.close()
    kf = kfmi.BatchedKF('cv3', B, 'f64')
    tr, cv, ld = kf.empty(T, 6, B), kf.empty(T, 9, B), kf.empty(T, B)
    sx, sP, sl = kf.empty(T, 6, B), kf.empty(T, 9, B), kf.empty(T, B)
    st = torch.full((B,), 55, dtype=torch.int32, device='cuda')
    L = _lib.lib()

    def calls():
        s = kf._stream()
        _lib.check(L.kf_reset(kf.handle, _ptr(x0), s))
        _lib.check(L.kf_run_rec(kf.handle, T, 0.1, None, _ptr(u), _ptr(z), None, k, _ptr(tr), _ptr(cv), _ptr(ld), s))
        _lib.check(L.kf_smooth_run(kf.handle, T, 0.1, None, _ptr(u), _ptr(tr), _ptr(cv), _ptr(sx), _ptr(sP), _ptr(sl),
                                   _ptr(st), s))

    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        calls()
    for _ in range(2):
        for t in (tr, cv, ld, sx, sP, sl):
            t.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        for name, got, want in (('traj', tr, eager[0]), ('cov', cv, eager[1]), ('logdet', ld, eager[2]),
                                ('sm_x', sx, sm['x']), ('sm_P', sP, sm['P']), ('sm_logdet', sl, sm['logdet']),
                                ('sm_status', st, sm['status'])):
            assert np.array_equal(_np(got), want), name
    x, P = kf.state()
    assert np.array_equal(_np(x), eager[3]) and np.array_equal(_np(P), eager[4])
    kf.close()


# -- failure isolation ----------------------------------------------------------------------------

@pytest.mark.parametrize('plant', ['nan', 'negative_pp'])
def test_failure_is_per_filter(plant):
    """A NaN, or a negative pp, planted in one filter's filt_P row r (data, not a fault): that
    filter's rows <= r are NaN and its status KF_ENOTSPD; its rows > r and every neighbour == the
    clean run."""
    T, B, r, f = 17, 130, 9, 70
    kf, tr, cv, u, dts = _filtered('cv3', T, B, False)
    kw = dict(u=u, dt=0.1, x=True, P=True, logdet=True)
    clean = _all(kf.smooth_run(tr, cv, **kw))
    bad_cv = cv.clone()
    bad_cv[r, 4 if plant == 'nan' else 0, f] = float('nan') if plant == 'nan' else -1.0e6
    bad = _all(kf.smooth_run(tr, bad_cv, **kw))
    kf.close()
    others = np.arange(B) != f
    assert bad['status'][f] == _lib.KF_ENOTSPD and (bad['status'][others] == 0).all()
    for n in ('x', 'P', 'logdet'):
        assert np.isnan(bad[n][:r + 1, ..., f]).all(), n
        assert np.array_equal(bad[n][r + 1:, ..., f], clean[n][r + 1:, ..., f]), n
        assert np.array_equal(bad[n][..., others], clean[n][..., others]), n


# -- refusals -------------------------------------------------------------------------------------

SENTINEL = -777.0


def _smooth_raw(kf, T, d, npd):
    """kf_smooth_run through the C API with sentinel-filled outputs: (rc, outputs)."""
    B = kf.batch
    fx = torch.ones(T, 2 * d, B, dtype=npd, device='cuda')
    fP = torch.ones(T, 3 * d, B, dtype=npd, device='cuda')
    outs = [torch.full((T, 2 * d, B), SENTINEL, dtype=npd, device='cuda'),
            torch.full((T, 3 * d, B), SENTINEL, dtype=npd, device='cuda'),
            torch.full((T, B), SENTINEL, dtype=npd, device='cuda'),
            torch.full((B,), 55, dtype=torch.int32, device='cuda')]
    rc = _lib.lib().kf_smooth_run(kf.handle, T, 0.1, None, None, _ptr(fx), _ptr(fP), *[_ptr(o) for o in outs], kf._stream())
    torch.cuda.synchronize()
    return rc, outs


@pytest.mark.parametrize('model,dtype', [('cv3', 'f32'), ('ref15', 'f64')])
def test_smooth_run_refuses_f32_and_reference_models(model, dtype):
    with kfmi.BatchedKF(model, 8, dtype) as kf:
        rc, outs = _smooth_raw(kf, 5, 3, torch.float32 if dtype == 'f32' else torch.float64)
        assert rc == _lib.KF_EINVAL and 'kf_smooth_run' in _lib.last_error()
        assert all(bool((o == (55 if o.dtype == torch.int32 else SENTINEL)).all()) for o in outs)
        with pytest.raises(kfmi.KFError) as e:
            kf.smooth_run(np.ones((5, 6, 8)), np.ones((5, 9, 8)), dt=0.1)
        assert e.value.code == _lib.KF_EINVAL


@pytest.mark.parametrize('why', ['offblock_P', 'nondiagonal_R'])
def test_run_rec_refuses_what_the_record_cannot_hold(why):
    B, T = 8, 5
    params = kfmi.default_params('cv3')
    if why == 'nondiagonal_R':
        params.r[1] = params.r[3] = 0.5
    with kfmi.BatchedKF('cv3', B, 'f64', params=params) as kf:
        kf.reset()
        x, P = kf.state()
        if why == 'offblock_P':
            P[_tri(6, 0, 1)] = 0.25                  # couples axes 0 and 1
            kf.set_state(x, P)
        before = [_np(t) for t in kf.state()]
        u = torch.zeros(T, 3, B, dtype=torch.float64, device='cuda')
        z = torch.zeros(T, 3, B, dtype=torch.float64, device='cuda')
        outs = [torch.full(s, SENTINEL, dtype=torch.float64, device='cuda') for s in ((T, 6, B), (T, 9, B), (T, B))]
        rc = _lib.lib().kf_run_rec(kf.handle, T, 0.1, None, _ptr(u), _ptr(z), None, 1, *[_ptr(o) for o in outs],
                                   kf._stream())
        torch.cuda.synchronize()
        assert rc == _lib.KF_EINVAL and 'kf_run_rec' in _lib.last_error()
        assert all(bool((o == SENTINEL).all()) for o in outs)
        assert all(np.array_equal(a, _np(b)) for a, b in zip(before, kf.state()))
        with pytest.raises(kfmi.KFError) as e:
            kf.run_rec(u, z, dt=0.1)
        assert e.value.code == _lib.KF_EINVAL
        kf.run(u, z, dt=0.1)                         # kf_run itself still takes the handle


def test_run_rec_refuses_reference_models_and_T0_is_ok():
    with kfmi.BatchedKF('ref8', 4, 'f64') as kf:
        rc = _lib.lib().kf_run_rec(kf.handle, 3, 0.1, None, None, None, None, 1, None, None, None, kf._stream())
        assert rc == _lib.KF_EINVAL and 'kf_run_rec' in _lib.last_error()
    with kfmi.BatchedKF('cv2', 4, 'f64') as kf:
        L = _lib.lib()
        assert L.kf_run_rec(kf.handle, 0, 0.1, None, None, None, None, 1, None, None, None, kf._stream()) == _lib.KF_OK
        assert L.kf_smooth_run(kf.handle, 0, 0.1, None, None, None, None, None, None, None, None,
                               kf._stream()) == _lib.KF_OK
        assert L.kf_smooth_run(kf.handle, 3, 0.1, None, None, None, None, None, None, None, None,
                               kf._stream()) == _lib.KF_EINVAL   # T > 0 needs a record
