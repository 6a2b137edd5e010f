"""EM for the constant-velocity models' noise constants on ``cv_score_oracle`` / ``cv_smoother_oracle``
/ ``extended_oracle``, batched over filters, in two arithmetics — TEST INFRASTRUCTURE ONLY (no GPU,
nothing of kfmi).

``estep`` is ``cv_smoother_oracle.backward`` with per-filter q, the row before step 0 and
kf_smooth_run_em's statistics.  With (x_f, P_f) the filtered row t (t = -1: the state the forward run
started from), d = dt[t + 1], x_p, P_p and C as there, the noise of the transition into step t + 1 is
w = x[t + 1] - F x[t] - G u[t + 1], and

    form 'gain':     J = Q d P_p^-1,  E[w] = J (x_s[t + 1] - x_p),  Var[w] = Q d + J (P_s[t + 1] - P_p) J^T
    form 'lag_one':  L = C P_s[t + 1] (= Cov(x[t], x[t + 1] | all)),  e = x_s[t + 1] - F x_s[t] - G u[t + 1],
                     E[w w^T] = e e^T + P_s[t + 1] + F P_s[t] F^T - F L - L^T F^T          (the textbook's)

Rows of ``em`` [4 + d, B] (kf.h's KF_EM_*): transitions counted (d != 0), sum of sum_axis E[w_pos^2] / d,
the same for the velocities, fixes applied, then per axis the sum over the applied fixes of
(z - p_s)^2 + P_s[pp] of the smoothed row.

``arith='longdouble'`` is the truth (form 'gain' unless asked otherwise; sums in longdouble);
``arith='f64'`` is plain NumPy float64 in the textbook form (``np.linalg.inv``; sums in float64), whose
own error against the truth is the E_ref that sets a kernel's budget.

``joint_solve`` is an independent derivation for the CPU test: ``cv_smoother_oracle.batch_solve``
extended by x_{-1} ~ N(x0, P0), so that the joint (x[t - 1], x[t]) blocks of ONE information-form solve
give E[w w^T] without any recursion.

``em_loop`` iterates forward run (``cv_score_oracle.run``, which also gives the innovation negative
log-likelihood), ``estep`` and ``mstep``; the table is rounded to float64 wherever a kernel would
receive it.
"""
import numpy as np

import cv_score_oracle as cso
import cv_smoother_oracle as cvo
import extended_oracle as xo
from smoother_oracle import _arith, _sym

LD = xo.LD
GROUPS = ('q_pos', 'q_vel', 'r')


def float_rows(d):
    return {'q_pos': [1], 'q_vel': [2], 'r': list(range(4, 4 + d))}


def _acc(arith):
    return LD if arith == 'longdouble' else np.float64


def _diag(A, v):
    """[B, n] -> [B, n, n] diagonal matrices."""
    B, n = v.shape
    out = np.zeros((B, n, n), dtype=A.dtype)
    for i in range(n):
        out[:, i, i] = v[:, i]
    return out


def estep(model, xf, Pf, dt_steps, u, z, update_every, applied, consts=None, init=None, arith='longdouble', form=None):
    """xf [T, B, n], Pf [T, B, n, n] the filtered record; u [T, d, B] | None; z [T // k, d, B] | None;
    applied [T, B] bool: the steps that ended with an applied fix; consts [2 + d, B] | None (the
    model's); init (x [B, n], P [B, n, n]) | None.  Returns dict(em [4 + d, B], x [T, B, n],
    P [T, B, n, n], logdet [T, B], and with init: init_x [B, n], init_P [B, n, n])."""
    A = _arith(arith)
    form = form or ('gain' if arith == 'longdouble' else 'lag_one')
    M = xo._rounded_model(model, None, 'f64')
    T, B, n = xf.shape
    d, k = M.m, update_every
    qf, _ = cso._consts(model, 'f64', B, None if consts is None else np.asarray(consts, np.float64), None)
    q = A.conv(qf)
    dts = A.conv(np.asarray(dt_steps, np.float64))
    us = A.conv(u) if u is not None else None
    zs = A.conv(z) if z is not None else None
    xf, Pf = A.conv(xf), A.conv(Pf)
    xs, Ps = xf.copy(), Pf.copy()
    acc = _acc(arith)
    em = np.zeros((4 + d, B), dtype=acc)
    out = {}

    def fix(t, x, P):
        if zs is None:
            return
        g = np.asarray(applied[t], bool)
        if not g.any():
            return
        zt = xo._T(zs[t // k])                                         # [B, d]
        for i in range(d):
            term = (zt[:, i] - x[:, i]) ** 2 + P[:, i, i]
            em[4 + i] += np.where(g, term.astype(acc), 0)
        em[3] += g

    fix(T - 1, xs[T - 1], Ps[T - 1])
    for t in range(T - 2, -2 if init is not None else -1, -1):
        xft, Pft = (xf[t], Pf[t]) if t >= 0 else (A.conv(init[0]), A.conv(np.broadcast_to(init[1], (B, n, n))))
        dd = dts[t + 1]
        F, G = cvo._FG(M, A, dd, B)
        Gu = xo._mv(G, xo._T(us[t + 1])) if us is not None else np.zeros((B, n), dtype=A.dtype)
        xp = xo._mv(F, xft) + Gu
        Qd = _diag(A, q * dd)
        Pp = np.matmul(np.matmul(F, Pft), xo._T(F)) + Qd
        C = cvo._right_inverse(A, Pp, np.matmul(Pft, xo._T(F)))
        xn, Pn = xs[t + 1], Ps[t + 1]
        xt = xft + xo._mv(C, xn - xp)
        Pt = Pft + np.matmul(np.matmul(C, Pn - Pp), xo._T(C))
        if dd != 0:
            if form == 'gain':
                J = cvo._right_inverse(A, Pp, Qd)
                ew = xo._mv(J, xn - xp)
                W = ew[:, :, None] * ew[:, None, :] + Qd + np.matmul(np.matmul(J, Pn - Pp), xo._T(J))
            else:
                L = np.matmul(C, Pn)
                e = xn - xo._mv(F, xt) - Gu
                FL = np.matmul(F, L)
                W = e[:, :, None] * e[:, None, :] + Pn + np.matmul(np.matmul(F, Pt), xo._T(F)) - FL - xo._T(FL)
            for i in range(d):
                em[1] += (W[:, i, i] / dd).astype(acc)
                em[2] += (W[:, d + i, d + i] / dd).astype(acc)
            em[0] += 1
        if t >= 0:
            xs[t], Ps[t] = xt, Pt
            fix(t, xt, Pt)
        else:
            out['init_x'], out['init_P'] = xt, Pt
    lds = np.stack([xo._logdet(A, _sym(A, Ps[t])) for t in range(T)])
    out.update(em=em, x=xs, P=Ps, logdet=lds)
    return out


def mstep(em, consts, d):
    """The new [2 + d, B] table: q = row / (d N_TRANS), r_i = row / N_FIX; a zero count keeps the
    old value.  In em's dtype."""
    em = np.asarray(em)
    new = np.asarray(consts).astype(em.dtype).copy()
    tr, fx = em[0] > 0, em[3] > 0
    new[0] = np.where(tr, em[1] / np.where(tr, d * em[0], 1), new[0])
    new[1] = np.where(tr, em[2] / np.where(tr, d * em[0], 1), new[1])
    new[2:] = np.where(fx, em[4:] / np.where(fx, em[3], 1), new[2:])
    return new


def nll(scores, d):
    """The innovation negative log-likelihood per filter from ``cv_score_oracle.run``'s scores."""
    two_pi = 2 * np.arccos(np.asarray(-1, dtype=scores.dtype))
    return (scores[1] + scores[2] + scores[0] * d * np.log(two_pi)) / 2


def iterate(model, x0, dt_steps, u, z, update_every, mask, consts, arith='longdouble', use_init=True, form=None):
    """One forward run under ``consts`` and its E-step: (forward dict, estep dict)."""
    M = xo._rounded_model(model, None, 'f64')
    fwd = cso.run(model, x0, dt_steps, u, z, update_every, mask=mask, consts=np.asarray(consts, np.float64),
                  dtype='f64', arith=arith)
    x0r, = xo.kernel_inputs('f64', x0)
    e = estep(model, fwd['x'], fwd['P'], dt_steps, u, z, update_every, fwd['applied'], consts=consts,
              init=(x0r, M.P0()) if use_init else None, arith=arith, form=form)
    return fwd, e


def em_loop(model, x0, dt_steps, u, z, update_every, mask, consts, iters, arith='longdouble', use_init=True, form=None):
    """``iters`` EM iterations from ``consts`` [2 + d, B].  Returns (tables [iters + 1, 2 + d, B], the
    table every forward run used, and nll [iters + 1, B]; the last forward run scores the result)."""
    d = cvo.axes(model)
    acc = _acc(arith)
    tab = np.asarray(consts).astype(acc)
    tabs, nlls = [tab], []
    for _ in range(iters):
        fwd, e = iterate(model, x0, dt_steps, u, z, update_every, mask, tab, arith, use_init, form)
        nlls.append(nll(fwd['scores'], d))
        tab = mstep(e['em'], tab, d)
        tabs.append(tab)
    fwd = cso.run(model, x0, dt_steps, u, z, update_every, mask=mask, consts=np.asarray(tab, np.float64), dtype='f64',
                  arith=arith)
    nlls.append(nll(fwd['scores'], d))
    return np.stack(tabs), np.stack(nlls)


def em_errors(got, truth, d):
    """{group: the worst relative error of got's float rows against truth's}, both [4 + d, B]; a
    non-finite entry is an infinite error."""
    t = np.asarray(truth).astype(LD)
    err = np.abs(np.asarray(got).astype(LD) - t) / np.abs(t)
    err = np.where(np.isfinite(err), err, np.inf)
    return {g: float(err[rows].max()) for g, rows in float_rows(d).items()}


def table_errors(got, truth):
    """The same for [..., 2 + d, B] constants' tables: groups q_pos, q_vel, r."""
    t = np.asarray(truth).astype(LD)
    err = np.abs(np.asarray(got).astype(LD) - t) / np.abs(t)
    err = np.where(np.isfinite(err), err, np.inf)
    return {'q_pos': float(err[..., 0, :].max()), 'q_vel': float(err[..., 1, :].max()), 'r': float(err[..., 2:, :].max())}


def joint_solve(model, x0, dt_steps, u, z, update_every, f, mask=None, consts=None, use_init=True):
    """Filter f from ONE linear solve in longdouble: the joint Gaussian over x_{-1}, x_0 .. x_{T-1} in
    information form, from x_{-1} ~ N(x0, P0), the links x_t = F_t x_{t-1} + G_t u_t + w_t, w_t ~ N(0, Q
    dt_t), and the fixes that were applied.  Returns dict(em [4 + d] (without the transition into step
    0 when use_init is False), x [T + 1, n], P [T + 1, n, n]; row 0 is x_{-1}).  Needs every dt > 0."""
    A = xo._LongDouble
    M = xo._rounded_model(model, None, 'f64')
    T, n, m = len(dt_steps), M.n, M.m
    B = x0.shape[0]
    assert np.all(np.asarray(dt_steps) > 0)
    etype, _, pay = cvo.events(model, dt_steps, z, update_every, B, mask)
    x0r, payr, ur = xo.kernel_inputs('f64', x0, pay, u)
    qf, rf = cso._consts(model, 'f64', B, None if consts is None else np.asarray(consts, np.float64), None)
    q, rg = A.conv(qf[f]), A.conv(rf[f])
    dts = A.conv(np.asarray(dt_steps, np.float64))
    us = A.conv(ur)[:, :, f] if ur is not None else np.zeros((T, M.c), LD)
    N = (T + 1) * n
    Lam, eta = np.zeros((N, N), LD), np.zeros(N, LD)
    eye = np.zeros((1, n, n), LD)
    for i in range(n):
        eye[:, i, i] = 1
    P0i = cvo._right_inverse(A, A.conv(M.P0())[None], eye)[0]
    Lam[:n, :n] += P0i
    eta[:n] += P0i @ A.conv(x0r[f])
    Fs, bs = [], []
    for t in range(T):
        F, G = cvo._FG(M, A, dts[t], 1)
        F, b = F[0], G[0] @ us[t]
        Fs.append(F)
        bs.append(b)
        Qi = np.zeros((n, n), LD)
        for i in range(n):
            Qi[i, i] = 1 / (q[i] * dts[t])
        lo, hi = slice(t * n, (t + 1) * n), slice((t + 1) * n, (t + 2) * n)
        Lam[lo, lo] += F.T @ Qi @ F
        Lam[lo, hi] -= F.T @ Qi
        Lam[hi, lo] -= Qi @ F
        Lam[hi, hi] += Qi
        eta[lo] -= F.T @ Qi @ b
        eta[hi] += Qi @ b
    zs = A.conv(payr)
    for t in range(T):
        if etype[t, f] == xo.GPS:
            for i in range(m):
                Lam[(t + 1) * n + i, (t + 1) * n + i] += 1 / rg[i]
                eta[(t + 1) * n + i] += zs[t, i, f] / rg[i]
    Lc = xo._chol(A, Lam[None])
    rhs = np.zeros((1, N, N + 1), LD)
    rhs[0, :, 0] = eta
    for i in range(N):
        rhs[0, i, i + 1] = 1
    sol = xo._chol_solve(A, Lc, rhs)[0]
    mean, cov = sol[:, 0].reshape(T + 1, n), sol[:, 1:]
    em = np.zeros(4 + m, LD)
    for t in range(0 if use_init else 1, T):
        a, b = slice(t * n, (t + 1) * n), slice((t + 1) * n, (t + 2) * n)
        F = Fs[t]
        e = mean[t + 1] - F @ mean[t] - bs[t]
        FSab = F @ cov[a, b]
        W = np.outer(e, e) + cov[b, b] + F @ cov[a, a] @ F.T - FSab - FSab.T
        for i in range(m):
            em[1] += W[i, i] / dts[t]
            em[2] += W[m + i, m + i] / dts[t]
        em[0] += 1
    for t in range(T):
        if etype[t, f] == xo.GPS:
            b = slice((t + 1) * n, (t + 2) * n)
            for i in range(m):
                em[4 + i] += (zs[t, i, f] - mean[t + 1, i]) ** 2 + cov[b, b][i, i]
            em[3] += 1
    return dict(em=em, x=mean, P=np.stack([cov[t * n:(t + 1) * n, t * n:(t + 1) * n] for t in range(T + 1)]))
