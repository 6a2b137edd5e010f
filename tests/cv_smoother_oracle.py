"""The constant-velocity models' fused run plus the Rauch-Tung-Striebel backward pass on
``extended_oracle``'s models, in two arithmetics, batched over filters — TEST INFRASTRUCTURE ONLY.

``forward`` is ``extended_oracle._run`` on ``cv_events`` (step t predicts with ``u[t]`` and ends
with the fix ``z[t // k]`` when ``(t + 1) % k == 0``; a masked fix is a predict-only event for that
filter).  ``backward`` is the dense pass over a filtered record ``(x_f [T, B, n], P_f [T, B, n, n])``:
row T - 1 is the filtered row, and for t = T - 2 .. 0, with d = dt[t + 1],

    x_p = F x_f[t] + G u[t + 1],   P_p = F P_f[t] F^T + Q d,   C = P_f[t] F^T P_p^-1,
    x_s[t] = x_f[t] + C (x_s[t + 1] - x_p),   P_s[t] = P_f[t] + C (P_s[t + 1] - P_p) C^T.

``arith='longdouble'`` is the truth (x87 extended; Cholesky solves written out, log det from the
Cholesky diagonal); ``arith='f64'`` is plain NumPy float64 (``np.linalg.inv`` / ``slogdet``, the
simple-form update), whose own error against the truth is the E_ref that sets a kernel's budget.
Inputs are first rounded to what the kernel receives (float64).

``batch_solve`` is an independent derivation of the smoothed moments for the CPU test: the
information-form solve over all T states of one filter at once (prior, F / Q / G-u links, the
fixes the forward pass applied).
"""
import numpy as np

import extended_oracle as xo
from extended_oracle import GPS, LD, PREDICT
from smoother_oracle import _arith, _sym


def axes(model):
    return 2 if model == 'cv2' else 3


def events(model, dt_steps, z, update_every, B, mask=None):
    """``extended_oracle.cv_events`` with a mask [U, B] (0: that filter's fix is dropped)."""
    T = len(dt_steps)
    etype, dt, pay = xo.cv_events(model, T, B, dt_steps, z, update_every)
    if mask is not None:
        for t in range(T):
            if etype[t, 0] == GPS:
                etype[t, np.asarray(mask)[t // update_every] == 0] = PREDICT
    return etype, dt, pay


def forward(model, x0, dt_steps, u, z, update_every, mask=None, arith='longdouble'):
    """dict(x [T, B, n], P [T, B, n, n], logdet [T, B]) of the filtered run, in the arithmetic's
    dtype; x0 [B, n], u [T, d, B] or None, z [T // k, d, B]."""
    A = _arith(arith)
    M = xo._rounded_model(model, None, 'f64')
    B = x0.shape[0]
    etype, dt, pay = events(model, dt_steps, z, update_every, B, mask)
    x0r, payr, ur = xo.kernel_inputs('f64', x0, pay, u)
    xs, Ps, lds = xo._run(M, A, x0r, M.P0(), etype, dt, payr, ur)
    return dict(x=xs, P=Ps, logdet=lds, etype=etype)


def _FG(M, A, d, B):
    n = M.n
    F = np.zeros((B, n, n), dtype=A.dtype)
    for i in range(n):
        F[:, i, i] = 1
    for (i, j) in M.lin:
        F[:, i, j] = d
    G = np.zeros((B, n, M.c), dtype=A.dtype)
    for (i, j) in M.ctl_quad:
        G[:, i, j] = A.conv(0.5)[()] * d ** 2
    for (i, j) in M.ctl_lin:
        G[:, i, j] = d
    return F, G


def _right_inverse(A, S, Y):
    """Y S^-1 for the SPD [B, n, n] matrices S."""
    if A.own_linalg:
        return xo._T(xo._chol_solve(A, xo._chol(A, S), xo._T(Y)))
    return np.matmul(Y, np.linalg.inv(S))


def backward(model, xf, Pf, dt_steps, u=None, arith='longdouble'):
    """The backward pass over the record (xf [T, B, n], Pf [T, B, n, n], float64 or longdouble
    values; a float64 record is what a kernel receives).  Returns dict(x, P, logdet) smoothed."""
    A = _arith(arith)
    M = xo._rounded_model(model, None, 'f64')
    T, B, n = xf.shape
    q = A.conv(M.q)
    dts = A.conv(np.asarray(dt_steps, np.float64))
    us = A.conv(u) if u is not None else None
    xf, Pf = A.conv(xf), A.conv(Pf)
    xs, Ps = xf.copy(), Pf.copy()
    for t in range(T - 2, -1, -1):
        d = dts[t + 1]
        F, G = _FG(M, A, d, B)
        xp = xo._mv(F, xf[t])
        if us is not None:
            xp = xp + xo._mv(G, xo._T(us[t + 1]))
        Pp = np.matmul(np.matmul(F, Pf[t]), xo._T(F))
        for i in range(n):
            Pp[:, i, i] = Pp[:, i, i] + q[i] * d
        C = _right_inverse(A, Pp, np.matmul(Pf[t], xo._T(F)))
        xs[t] = xf[t] + xo._mv(C, xs[t + 1] - xp)
        Ps[t] = Pf[t] + np.matmul(np.matmul(C, Ps[t + 1] - Pp), xo._T(C))
    lds = np.stack([xo._logdet(A, _sym(A, Ps[t])) for t in range(T)])
    return dict(x=xs, P=Ps, logdet=lds)


def smoothed(model, x0, dt_steps, u, z, update_every, mask=None, arith='longdouble'):
    """(filtered, smoothed) of forward then backward in one arithmetic."""
    f = forward(model, x0, dt_steps, u, z, update_every, mask, arith)
    return f, backward(model, f['x'], f['P'], dt_steps, u, arith)


def pack_cov(model, P):
    """[T, B, n, n] -> the kernels' block-packed [T, 3 d, B]: axis i's (pp, pv, vv) in rows 3 i .."""
    d = axes(model)
    rows = []
    for i in range(d):
        rows += [P[:, :, i, i], P[:, :, i, d + i], P[:, :, d + i, d + i]]
    return np.stack(rows, axis=1)


def unpack_cov(model, cov):
    """The kernels' [T, 3 d, B] -> full symmetric [T, B, n, n] (entries that couple two axes 0)."""
    d = axes(model)
    T, _, B = cov.shape
    P = np.zeros((T, B, 2 * d, 2 * d), dtype=cov.dtype)
    for i in range(d):
        P[:, :, i, i] = cov[:, 3 * i]
        P[:, :, i, d + i] = P[:, :, d + i, i] = cov[:, 3 * i + 1]
        P[:, :, d + i, d + i] = cov[:, 3 * i + 2]
    return P


def batch_solve(model, x0, dt_steps, u, z, update_every, f, mask=None):
    """Filter f's smoothed means [T, n] and covariances [T, n, n] from ONE linear solve, in
    longdouble: the joint Gaussian over x_0 .. x_{T-1} in information form, from the prior on x_0
    (step 0's prediction from (x0, P0)), the links x_t = F_t x_{t-1} + G_t u_t + w_t, w_t ~ N(0, Q
    dt_t), and the fixes that were applied.  Needs every dt > 0."""
    A = xo._LongDouble
    M = xo._rounded_model(model, None, 'f64')
    T, n, m = len(dt_steps), M.n, M.m
    assert np.all(np.asarray(dt_steps) > 0)
    etype, _, pay = events(model, dt_steps, z, update_every, x0.shape[0], mask)
    x0r, payr, ur = xo.kernel_inputs('f64', x0, pay, u)
    q, rg = A.conv(M.q), A.conv(M.r_gps)
    dts = A.conv(np.asarray(dt_steps, np.float64))
    us = A.conv(ur)[:, :, f] if ur is not None else np.zeros((T, M.c), LD)
    N = T * n
    Lam, eta = np.zeros((N, N), LD), np.zeros(N, LD)
    eye = np.zeros((1, n, n), LD)
    for i in range(n):
        eye[:, i, i] = 1
    F, G = _FG(M, A, dts[0], 1)
    xp0 = F[0] @ A.conv(x0r[f]) + G[0] @ us[0]
    Pp0 = F[0] @ A.conv(M.P0()) @ F[0].T
    for i in range(n):
        Pp0[i, i] += q[i] * dts[0]
    P0i = _right_inverse(A, Pp0[None], eye)[0]
    Lam[:n, :n] += P0i
    eta[:n] += P0i @ xp0
    for t in range(1, T):
        F, G = _FG(M, A, dts[t], 1)
        F, b = F[0], G[0] @ us[t]
        Qi = np.zeros((n, n), LD)
        for i in range(n):
            Qi[i, i] = 1 / (q[i] * dts[t])
        lo, hi = slice((t - 1) * n, t * n), slice(t * n, (t + 1) * n)
        Lam[lo, lo] += F.T @ Qi @ F
        Lam[lo, hi] -= F.T @ Qi
        Lam[hi, lo] -= Qi @ F
        Lam[hi, hi] += Qi
        eta[lo] -= F.T @ Qi @ b
        eta[hi] += Qi @ b
    zs = A.conv(payr)
    for t in range(T):
        if etype[t, f] == GPS:
            for i in range(m):
                Lam[t * n + i, t * n + i] += 1 / rg[i]
                eta[t * n + i] += zs[t, i, f] / rg[i]
    Lc = xo._chol(A, Lam[None])
    rhs = np.zeros((1, N, N + 1), LD)
    rhs[0, :, 0] = eta
    for i in range(N):
        rhs[0, i, i + 1] = 1
    sol = xo._chol_solve(A, Lc, rhs)[0]
    cov = sol[:, 1:]
    return sol[:, 0].reshape(T, n), np.stack([cov[t * n:(t + 1) * n, t * n:(t + 1) * n] for t in range(T)])
