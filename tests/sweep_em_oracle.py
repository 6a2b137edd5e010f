"""EM for the reference models' diagonal Q, R_imu and R_gps on ``smoother_oracle.run``, one filter at
a time, in two arithmetics — TEST INFRASTRUCTURE ONLY (no GPU, nothing of kfmi).

``estep`` reads one ``smoother_oracle.run`` (its xp, Pp, F, z, applied, xf, Pf, xs, Ps) and gathers
kf_smooth_sweep_em's statistics.  Event 0 starts the interval: neither its transition nor its update
is counted.  For t >= 1 with etype[t] != NONE and d = dt[t] != 0 the noise of the transition into
event t is w = x[t] - F x[t - 1], and

    form 'gain':     J = Q d P_p^-1,  E[w] = J (x_s[t] - x_p),  Var[w] = Q d + J (P_s[t] - P_p) J^T
    form 'lag_one':  L = C_{t-1} P_s[t] (= Cov(x[t - 1], x[t] | all)),  e = x_s[t] - F x_s[t - 1],
                     E[w w^T] = e e^T + P_s[t] + F P_s[t - 1] F^T - F L - L^T F^T       (the textbook's)

and state i adds E[w w^T]_ii / d.  An applied update at t >= 1 adds (z_i - x_s[t]_i)^2 + P_s[t]_ii per
measured state, z the measurement the forward pass used (``run``'s z: a fix, or the IMU
pseudo-measurement built from the predicted state).

Rows of ``em`` [3 + 2 n + m] (kf.h's KF_REF_EM_*): N_TRANS, Q [n], N_IMU, R_IMU [n], N_GPS, R_GPS [m].

``arith='longdouble'`` is the truth (form 'gain' unless asked otherwise; sums in longdouble);
``arith='f64'`` is plain NumPy float64 in the textbook form (``np.linalg.inv``; sums in float64), whose
own error against the truth is the E_ref that sets a kernel's budget.

``joint_cov`` is an independent derivation for the CPU test: ``smoother_oracle.batch_solve``'s
information matrix over all T states, inverted whole, so that its off-diagonal blocks are the
lag-one covariances without any recursion.

``em_loop`` iterates forward run + backward pass (``smoother_oracle.run``), the innovation negative
log-likelihood of that forward run (``score_oracle.run``), ``estep`` and ``mstep``; the constants
are rounded to float64 wherever a kernel would receive them.
"""
import numpy as np

import extended_oracle as xo
import score_oracle as sco
import smoother_oracle as so
from smoother_oracle import GPS, IMU, LD, NONE, _arith, _inv_apply

GROUPS = ('q', 'r_imu', 'r_gps')
# the states whose IMU pseudo-measurement row is the sensor's own value (attitude, rate, acceleration)
IMU_MEASURED = {'ref15': (3, 4, 5, 9, 10, 11, 12, 13, 14), 'ref8': (2, 5, 6, 7)}


def dims(model):
    return (15, 3) if model == 'ref15' else (8, 2)


def rows(model):
    """Where the blocks of em start, and its height."""
    n, m = dims(model)
    return dict(n_trans=0, q=1, n_imu=1 + n, r_imu=2 + n, n_gps=2 + 2 * n, r_gps=3 + 2 * n, rows=3 + 2 * n + m)


def float_rows(model):
    n, m = dims(model)
    r = rows(model)
    return {'q': list(range(r['q'], r['q'] + n)), 'r_imu': list(range(r['r_imu'], r['r_imu'] + n)),
            'r_gps': list(range(r['r_gps'], r['r_gps'] + m))}


def _acc(arith):
    return LD if arith == 'longdouble' else np.float64


def counts(model, etype, dt, applied):
    """(N_TRANS, N_IMU, N_GPS) from the stream and the applied flags alone."""
    etype, dt, applied = np.asarray(etype), np.asarray(dt), np.asarray(applied, bool)
    later = np.arange(len(etype)) >= 1
    n_tr = int(np.sum(later & (etype != NONE) & (dt != 0)))
    n_imu = int(np.sum(later & applied & (etype == IMU)))
    n_gps = int(np.sum(later & applied & (etype == GPS)))
    return n_tr, n_imu, n_gps


def estep(model, etype, dt, r, K=None, arith='longdouble', form=None):
    """One filter: etype [T], dt [T], r = ``smoother_oracle.run``'s dict in the same arithmetic, K the
    constants it ran under.  Returns em [3 + 2 n + m] in the accumulator's dtype."""
    A = _arith(arith)
    form = form or ('gain' if arith == 'longdouble' else 'lag_one')
    M = xo._rounded_model(model, K, 'f64')
    etype = np.asarray(etype)
    T, n, m = len(etype), M.n, M.m
    R = rows(model)
    acc = _acc(arith)
    q = A.conv(M.q)
    dts = A.conv(np.asarray(dt, np.float64))
    em = np.zeros(R['rows'], dtype=acc)
    xs, Ps, xf, Pf, xp, Pp, Fs = (r[k] for k in ('xs', 'Ps', 'xf', 'Pf', 'xp', 'Pp', 'F'))
    assert xs.dtype == A.dtype
    for t in range(1, T):
        if etype[t] == NONE:
            continue
        d = dts[t]
        if d != 0:
            F = Fs[t][None]
            Qd = np.zeros((1, n, n), dtype=A.dtype)
            for i in range(n):
                Qd[0, i, i] = q[i] * d
            if form == 'gain':
                J = _inv_apply(A, Pp[t][None], Qd)
                ew = xo._mv(J, (xs[t] - xp[t])[None])
                W = ew[:, :, None] * ew[:, None, :] + Qd + np.matmul(np.matmul(J, (Ps[t] - Pp[t])[None]), xo._T(J))
            else:
                C = _inv_apply(A, Pp[t][None], np.matmul(Pf[t - 1][None], xo._T(F)))
                L = np.matmul(C, Ps[t][None])
                e = (xs[t][None] - xo._mv(F, xs[t - 1][None]))
                FL = np.matmul(F, L)
                W = e[:, :, None] * e[:, None, :] + Ps[t][None] + np.matmul(np.matmul(F, Ps[t - 1][None]), xo._T(F)) \
                    - FL - xo._T(FL)
            for i in range(n):
                em[R['q'] + i] += acc(W[0, i, i] / d)
            em[R['n_trans']] += 1
        if r['applied'][t]:
            z = r['z'][t]
            base, cnt, k = (R['r_gps'], R['n_gps'], m) if etype[t] == GPS else (R['r_imu'], R['n_imu'], n)
            for i in range(k):
                em[base + i] += acc((z[i] - xs[t, i]) ** 2 + Ps[t, i, i])
            em[cnt] += 1
    return em


def table(K, model):
    """The constants as one column of run_sweep's table: q [n], r_imu [n], r_gps [m] (float64)."""
    n, m = dims(model)
    M = xo.Model(model, K)
    return np.concatenate([M.q[:n], M.r_imu[:n], M.r_gps[:m]]).astype(np.float64)


def consts_of(tab, model, p0):
    """The K dict of a table column (rounded to float64, as a kernel would receive it)."""
    n, m = dims(model)
    t = np.asarray(tab).astype(np.float64)
    return dict(q=t[:n], r_imu=t[n:2 * n], r_gps=t[2 * n:], p0=np.asarray(p0, np.float64))


def mstep(em, tab, model, imu_rows='measured'):
    """The new table column [2 n + m] from em [ROWS] and the old column: q_i = Q_i / N_TRANS, r = R / N.
    A zero count keeps the old values; a q whose old value is 0 stays 0; imu_rows 'measured' | 'all' |
    'none' as kfmi.ref_em_update.  In em's dtype."""
    n, m = dims(model)
    R = rows(model)
    em = np.asarray(em)
    new = np.asarray(tab).astype(em.dtype).copy()
    if em[R['n_trans']] > 0:
        for i in range(n):
            if new[i] != 0:
                new[i] = em[R['q'] + i] / em[R['n_trans']]
    if em[R['n_imu']] > 0 and imu_rows != 'none':
        for i in (range(n) if imu_rows == 'all' else IMU_MEASURED[model]):
            new[n + i] = em[R['r_imu'] + i] / em[R['n_imu']]
    if em[R['n_gps']] > 0:
        for i in range(m):
            new[2 * n + i] = em[R['r_gps'] + i] / em[R['n_gps']]
    return new


def nll(scores, model):
    """The GPS + IMU innovation negative log-likelihood from ``score_oracle.run``'s scores [8]."""
    n, m = dims(model)
    two_pi = 2 * np.arccos(np.asarray(-1, dtype=scores.dtype))
    return (scores[1] + scores[2] + scores[0] * m * np.log(two_pi) +
            scores[4] + scores[5] + scores[3] * n * np.log(two_pi)) / 2


def em_loop(model, x0, P0, etype, dt, pay, thr, K, iters, imu_rows='measured', arith='longdouble', form=None):
    """``iters`` EM iterations of one filter from the constants K under the gate thr.  Returns
    dict(tables [iters + 1, 2 n + m] (the column every forward run used, then the result), nll
    [iters + 1] (of every forward run; the last one scores the result), margin [iters + 1] (the
    distance of thr from the run's gate values; inf for thr = -inf), applied [iters + 1, T])."""
    acc = _acc(arith)
    tab = table(K, model).astype(acc)
    p0 = np.asarray(K['p0'] if K is not None else xo.Model(model).p0, np.float64)
    tabs, nlls, margins, applied = [tab], [], [], []

    def forward(tab):
        Kc = consts_of(tab, model, p0)
        r = so.run(model, x0, P0, etype, dt, pay, thr=thr, K=Kc, arith=arith)
        s = sco.run(model, x0, P0, etype, dt, pay, K=Kc, arith=arith, applied=r['applied'])
        nlls.append(nll(s['scores'], model))
        g = r['gate'][~np.isnan(r['gate'].astype(np.float64))]
        margins.append(float(np.min(np.abs(g - thr))) if np.isfinite(thr) and len(g) else np.inf)
        applied.append(r['applied'].copy())
        return Kc, r

    for _ in range(iters):
        Kc, r = forward(tab)
        tab = mstep(estep(model, etype, dt, r, K=Kc, arith=arith, form=form), tab, model, imu_rows)
        tabs.append(tab)
    forward(tab)
    return dict(tables=np.stack(tabs), nll=np.stack(nlls), margin=np.array(margins), applied=np.stack(applied))


def _rel(got, truth):
    t = np.asarray(truth).astype(LD)
    with np.errstate(divide='ignore', invalid='ignore'):
        err = np.abs(np.asarray(got).astype(LD) - t) / np.abs(t)
    err = np.where(t == 0, np.where(np.asarray(got).astype(LD) == 0, 0, np.inf), err)
    return np.where(np.isfinite(err), err, np.inf)


def em_errors(got, truth, model):
    """{group: the worst relative error of got's float rows against truth's}, both [ROWS] or [ROWS, B],
    over the entries whose truth is not zero (a zero truth wants an exact zero); a non-finite entry is
    an infinite error."""
    err = _rel(got, truth)
    return {g: float(err[rr].max()) for g, rr in float_rows(model).items()}


def table_errors(got, truth, model):
    """The same for [..., 2 n + m] or [..., 2 n + m, B] constants' tables (the axis of length 2 n + m is
    found from the model): groups q, r_imu, r_gps."""
    n, m = dims(model)
    err = _rel(got, truth)
    ax = [i for i, s in enumerate(err.shape) if s == 2 * n + m][-1]
    err = np.moveaxis(err, ax, 0)
    return {'q': float(err[:n].max()), 'r_imu': float(err[n:2 * n].max()), 'r_gps': float(err[2 * n:].max())}


def joint_cov(model, etype, dt, r, K=None):
    """``smoother_oracle.batch_solve``'s joint Gaussian over x_0 .. x_{T-1} (the same prior, links and
    applied measurements, in longdouble), returned whole: (mean [T, n], cov [T n, T n]).  Needs dt > 0
    after event 0 and no NONE event."""
    A = xo._LongDouble
    M = xo._rounded_model(model, K, 'f64')
    T, n = len(etype), M.n
    assert not np.any(np.asarray(etype) == NONE) and np.all(np.asarray(dt)[1:] > 0)
    q, rg, ri = A.conv(M.q), A.conv(M.r_gps), A.conv(M.r_imu)
    dts = A.conv(np.asarray(dt, np.float64))
    N = T * n
    Lam, eta = np.zeros((N, N), LD), np.zeros(N, LD)
    eye = np.zeros((1, n, n), LD)
    for i in range(n):
        eye[:, i, i] = 1
    P0i = _inv_apply(A, r['Pp'][0][None], eye)[0]
    Lam[:n, :n] += P0i
    eta[:n] += P0i @ r['xp'][0]
    for t in range(1, T):
        F = so._F(M, A, dts[t:t + 1])[0]
        Qi = np.zeros((n, n), LD)
        for i in range(n):
            Qi[i, i] = 1 / (q[i] * dts[t])
        a, b = slice((t - 1) * n, t * n), slice(t * n, (t + 1) * n)
        Lam[a, a] += F.T @ Qi @ F
        Lam[a, b] -= F.T @ Qi
        Lam[b, a] -= Qi @ F
        Lam[b, b] += Qi
    for t in range(T):
        if r['applied'][t]:
            k, rr = (M.m, rg) if etype[t] == GPS else (n, ri)
            for i in range(k):
                Lam[t * n + i, t * n + i] += 1 / rr[i]
                eta[t * n + i] += r['z'][t][i] / rr[i]
    Lc = xo._chol(A, Lam[None])
    rhs = np.zeros((1, N, N + 1), LD)
    rhs[0, :, 0] = eta
    for i in range(N):
        rhs[0, i, i + 1] = 1
    sol = xo._chol_solve(A, Lc, rhs)[0]
    return sol[:, 0].reshape(T, n), sol[:, 1:]
