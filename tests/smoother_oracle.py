"""The dense gated filter plus the Rauch-Tung-Striebel backward pass on ``extended_oracle``'s
models, in two arithmetics — TEST INFRASTRUCTURE ONLY.

``run(model, x0, P0, etype, dt, pay, thr, K, arith)`` runs ONE filter over one stream:

forward, per event t (``extended_oracle._run``'s step): a NONE event changes nothing; otherwise
``x_p = F x``, ``P_p = F P F^T + Q dt``, the gate value ``logdet(P_p)``, and a GPS / IMU event is
applied where the gate value ``> thr`` (``thr = -inf``: always);

backward, for t = T - 2 .. 0: a NONE event at t + 1 copies row t + 1; otherwise
``C = P_f[t] F^T P_p[t + 1]^-1``, ``x_s[t] = x_f[t] + C (x_s[t + 1] - x_p[t + 1])``,
``P_s[t] = P_f[t] + C (P_s[t + 1] - P_p[t + 1]) C^T``.

``arith='longdouble'`` is the truth (x87 extended; the inverses are Cholesky solves written out,
log det from the Cholesky diagonal); ``arith='f64'`` is plain NumPy float64 (``np.linalg.inv`` /
``slogdet``, the simple-form update), whose own error against the truth is the E_ref that sets a
kernel's budget.  Inputs are first rounded to what the kernel receives (float64).

``batch_solve`` is an independent derivation of the smoothed moments for the CPU test: the
information-form solve over all T states at once.
"""
import numpy as np

import extended_oracle as xo
from extended_oracle import GPS, IMU, LD, NONE, PREDICT  # noqa: F401 (re-exported for the tests)


class _Float64:
    dtype = np.float64
    own_linalg = False
    conv = staticmethod(lambda a: np.asarray(a).astype(np.float64))


def _arith(name):
    return _Float64 if name == 'f64' else xo._arith(name)


def _F(M, A, d):
    F = np.zeros((1, M.n, M.n), dtype=A.dtype)
    for i in range(M.n):
        F[:, i, i] = 1
    for (i, j) in M.lin:
        F[:, i, j] = d
    for (i, j) in M.quad:
        F[:, i, j] = A.conv(0.5)[()] * d ** 2
    return F


def _inv_apply(A, S, Y):
    """Y S^-1 for the SPD [1, n, n] matrix S."""
    if A.own_linalg:
        return xo._T(xo._chol_solve(A, xo._chol(A, S), xo._T(Y)))
    return np.matmul(Y, np.linalg.inv(S))


def _sym(A, P):
    return (P + xo._T(P)) * A.conv(0.5)[()] if A.own_linalg else P


def run(model, x0, P0, etype, dt, pay, thr=-np.inf, K=None, arith='longdouble'):
    """x0 [n], P0 [n, n], etype [T], dt [T], pay [T, 9]; thr: the gate threshold; K: caller
    constants (``ModelConsts.oracle()``) or None.  Returns a dict of arrays in the arithmetic's
    dtype: xf [T, n], Pf [T, n, n], ldf [T] (the filtered record and its log det), xs, Ps, lds (the
    smoothed), gate [T] (logdet(P_pred); NaN at NONE events), applied [T] bool, and the forward
    pass' own xp [T, n], Pp [T, n, n], z (a list: the measurement an applied event used)."""
    A = _arith(arith)
    M = xo._rounded_model(model, K, 'f64')
    x0, P0, pay = xo.kernel_inputs('f64', x0, P0, pay)
    etype = np.asarray(etype)
    T, n = len(etype), M.n
    q, rg, ri = A.conv(M.q), A.conv(M.r_gps), A.conv(M.r_imu)
    dts, pays = A.conv(np.asarray(dt, np.float64)), A.conv(pay)
    x, P = A.conv(x0)[None].copy(), A.conv(P0)[None].copy()
    xf, Pf = np.zeros((T, n), A.dtype), np.zeros((T, n, n), A.dtype)
    xp, Pp = np.zeros((T, n), A.dtype), np.zeros((T, n, n), A.dtype)
    Fs = np.zeros((T, n, n), A.dtype)
    gate, applied, zs = np.full(T, np.nan, A.dtype), np.zeros(T, bool), [None] * T
    for t in range(T):
        if etype[t] != NONE:
            d = dts[t:t + 1]
            F = _F(M, A, d)
            xq = xo._mv(F, x)
            Pq = np.matmul(np.matmul(F, P), xo._T(F))
            for i in range(n):
                Pq[:, i, i] = Pq[:, i, i] + q[i] * d
            Fs[t], xp[t], Pp[t] = F[0], xq[0], Pq[0]
            gate[t] = xo._logdet(A, _sym(A, Pq))[0]
            x, P = xq, Pq
            if etype[t] in (GPS, IMU) and gate[t] > thr:
                applied[t] = True
                if etype[t] == GPS:
                    k, r, z = M.m, rg, pays[t:t + 1, :M.m]
                else:
                    k, r, z = n, ri, M.imu_z(xq, pays[t:t + 1], d)
                zs[t] = z[0].copy()
                x, P = xo._update(A, xq, Pq, k, r, z, False)
        xf[t], Pf[t] = x[0], P[0]
    xs, Ps = xf.copy(), Pf.copy()
    for t in range(T - 2, -1, -1):
        if etype[t + 1] == NONE:
            xs[t], Ps[t] = xs[t + 1], Ps[t + 1]
            continue
        C = _inv_apply(A, Pp[t + 1][None], np.matmul(Pf[t][None], xo._T(Fs[t + 1][None])))
        xs[t] = xf[t] + xo._mv(C, (xs[t + 1] - xp[t + 1])[None])[0]
        Ps[t] = Pf[t] + np.matmul(np.matmul(C, (Ps[t + 1] - Pp[t + 1])[None]), xo._T(C))[0]
    ldf = np.array([xo._logdet(A, _sym(A, Pf[t][None]))[0] for t in range(T)], A.dtype)
    lds = np.array([xo._logdet(A, _sym(A, Ps[t][None]))[0] for t in range(T)], A.dtype)
    return dict(xf=xf, Pf=Pf, ldf=ldf, xs=xs, Ps=Ps, lds=lds, gate=gate, applied=applied, xp=xp, Pp=Pp, z=zs, F=Fs)


def as_records(r, which):
    """``extended_oracle.errors``' dict(x [T, 1, n], P [T, 1, n, n], logdet [T, 1]) of the
    filtered (which = 'f') or smoothed ('s') record of one ``run``."""
    return dict(x=r['x' + which][:, None], P=r['P' + which][:, None], logdet=r['ld' + which][:, None])


def batch_solve(model, etype, dt, r, K=None):
    """The smoothed means and covariances of every state from ONE linear solve, in longdouble:
    the joint Gaussian over x_0 .. x_{T-1} in information form, built from the prior on x_0 (the
    forward pass' predicted (x_p, P_p) of event 0), the links x_t = F_t x_{t-1} + w_t, w_t ~ N(0, Q
    dt_t), and the measurements the forward pass applied (``r`` = ``run``'s truth: its z, applied,
    xp[0], Pp[0]).  Needs dt > 0 after event 0 and no NONE event.  Returns (x [T, n], P [T, n, n])."""
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
        F = _F(M, A, dts[t:t + 1])[0]
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
    cov = sol[:, 1:]
    return sol[:, 0].reshape(T, n), np.stack([cov[t * n:(t + 1) * n, t * n:(t + 1) * n] for t in range(T)])
