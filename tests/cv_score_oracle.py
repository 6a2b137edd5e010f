"""The constant-velocity models' fused run with kf_run_scores' score rows, per-filter constants,
control and mask, batched over filters, as truth and as plain references — TEST INFRASTRUCTURE
ONLY (no GPU, nothing of kfmi).

``run`` is ``extended_oracle._run`` restricted to ``cv_events`` (step t predicts with ``u[t]`` and
ends with the fix ``z[t // k]`` when ``(t + 1) % k == 0``; a masked fix is a predict-only step for
that filter), with filter f's q and r taken from column f of a ``[2 + d, B]`` table (rows q_pos,
q_vel, r per axis) or from one set ``K = (q_pos, q_vel, r[d])`` for every filter; without either
the model's own.  It runs in the three arithmetics of ``score_oracle.run``: ``'longdouble'`` (the
truth: Cholesky solves written out, simple-form update), ``'f64'`` (ordinary NumPy float64,
``np.linalg.inv`` / ``slogdet``, simple form) and ``'f32'`` (ordinary NumPy float32, Joseph's
form).  For every applied fix it accumulates the step's own innovation statistics, S = H P_pred
H^T + R and y = z - H x_pred, and after every step whose track row holds no NaN for the filter the
squared position error.  The plain references form each term in their own precision and sum in
float64 (the scores are doubles whatever the filter's dtype); the truth sums in longdouble.

With ``floors=True`` (the truth run) it also returns each float row's floor, propagated from
``extended_oracle.FLOOR[dtype]`` through the row's formula exactly as ``score_oracle.run`` does:
the allowed state error is FLOOR times the component group's scale (the stream-wide max of
max(|x|, sd)), the allowed covariance error FLOOR times sd_i sd_j, and
    NIS       sum_t 2 |S^-1 y|^T dy + |S^-1 y|^T dS |S^-1 y|
    logdet S  sum_t sum_ab |S^-1_ab| dS_ab
    pos_sse   sum_t 2 |e|^T dx_pos
"""
import numpy as np

import cv_smoother_oracle as cvo
import extended_oracle as xo
import score_oracle as so

LD = xo.LD
GPS = xo.GPS
ROWS = so.ROWS
FLOAT_ROWS = (1, 2, 7)          # the live float rows; 0 and 6 are the live counts, 3 .. 5 stay 0
LIVE_ROWS = (0, 1, 2, 6, 7)


def table(model, sets, B=None):
    """[2 + d, B] float64 from (q_pos, q_vel, r[d]) tuples, cycled over B filters."""
    d = cvo.axes(model)
    B = len(sets) if B is None else B
    tab = np.empty((2 + d, B))
    for f in range(B):
        q_pos, q_vel, r = sets[f % len(sets)]
        tab[0, f], tab[1, f], tab[2:, f] = q_pos, q_vel, np.broadcast_to(r, (d,))
    return tab


def _consts(model, dtype, B, consts, K):
    """(q [B, n], r [B, d]) as the kernel receives them, float64 values."""
    M = xo._rounded_model(model, None, dtype)
    d = M.m
    if K is not None:
        assert consts is None
        consts = table(model, [K], B)
    if consts is None:
        return np.tile(M.q, (B, 1)), np.tile(M.r_gps, (B, 1))
    consts = np.asarray(consts, np.float64)
    assert consts.shape == (2 + d, B)
    q = np.concatenate([np.repeat(consts[0:1], d, 0), np.repeat(consts[1:2], d, 0)]).T
    q, r = xo.kernel_inputs(dtype, q, consts[2:].T)
    return q, r


def _update(A, x, P, k, r, z, joseph):
    """``extended_oracle._update`` with R = diag(r[f]) per filter, r [B, k]."""
    n = P.shape[-1]
    S = P[:, :k, :k].copy()
    for i in range(k):
        S[:, i, i] = S[:, i, i] + r[:, i]
    PHt = P[:, :, :k]
    if A.own_linalg:
        K = xo._T(xo._chol_solve(A, xo._chol(A, S), xo._T(PHt)))
    else:
        K = np.matmul(PHt, np.linalg.inv(S))
    xn = x + xo._mv(K, z - x[:, :k])
    IKH = np.zeros(P.shape, dtype=A.dtype)
    for i in range(n):
        IKH[:, i, i] = 1
    IKH[:, :, :k] = IKH[:, :, :k] - K
    Pn = np.matmul(IKH, P)
    if joseph:
        Pn = np.matmul(Pn, xo._T(IKH)) + np.matmul(K * r[:, None, :], xo._T(K))
    return xn, Pn


def run(model, x0, dt_steps, u, z, update_every, mask=None, consts=None, K=None, track=None, dtype='f64',
        arith='longdouble', floors=False):
    """x0 [B, n], dt_steps [T], u [T, d, B] | None, z [T // k, d, B], mask [T // k, B] | None,
    consts [2 + d, B] | None, K one set | None, track [T, d, B] | None.  Inputs are rounded to the
    kernel's ``dtype`` first (dt and the constants' table stay float64 until each is used as the
    kernel uses it).  Returns dict(scores [8, B] (longdouble for the truth, float64 otherwise),
    x [T, B, n], P [T, B, n, n], applied [T, B] bool, and with floors=True floor [8, B])."""
    A = so._arith(arith)
    joseph = arith == 'f32'
    M = xo._rounded_model(model, None, dtype)
    B, n, m = x0.shape[0], M.n, M.m
    T = len(dt_steps)
    etype, dt, pay = cvo.events(model, dt_steps, z, update_every, B, mask)
    x0r, payr, ur, trk = xo.kernel_inputs(dtype, x0, pay, u, track)
    qf, rf = _consts(model, dtype, B, consts, K)
    q, r = A.conv(qf), A.conv(rf)
    x = A.conv(x0r).copy()
    P = A.conv(np.broadcast_to(M.P0(), (B, n, n))).copy()
    dts, pays = A.conv(dt), A.conv(payr)
    us = A.conv(ur) if ur is not None else None
    half = A.conv(0.5)[()]
    acc = LD if arith == 'longdouble' else np.float64
    sc = np.zeros((8, B), dtype=acc)
    xs = np.zeros((T, B, n), dtype=A.dtype)
    Ps = np.zeros((T, B, n, n), dtype=A.dtype)
    applied = np.zeros((T, B), bool)
    rec_upd, rec_pos = [], []
    eye = so._eye(A, m)
    for t in range(T):
        et, d = etype[t], dts[t]
        F = np.zeros((B, n, n), dtype=A.dtype)
        for i in range(n):
            F[:, i, i] = 1
        for (i, j) in M.lin:
            F[:, i, j] = d
        xp = xo._mv(F, x)
        if us is not None:
            G = np.zeros((B, n, M.c), dtype=A.dtype)
            for (i, j) in M.ctl_quad:
                G[:, i, j] = half * d ** 2
            for (i, j) in M.ctl_lin:
                G[:, i, j] = d
            xp = xp + xo._mv(G, xo._T(us[t]))
        Pp = np.matmul(np.matmul(F, P), xo._T(F))
        for i in range(n):
            Pp[:, i, i] = Pp[:, i, i] + q[:, i] * d
        g = et == GPS
        x, P = xp, Pp
        if g.any():
            zt = xo._T(pays[t])[:, :m]
            S = Pp[:, :m, :m].copy()
            for i in range(m):
                S[:, i, i] = S[:, i, i] + r[:, i]
            y = zt - xp[:, :m]
            if A.own_linalg:
                L = xo._chol(A, S)
                Si = xo._chol_solve(A, L, np.broadcast_to(eye, (B, m, m)))
                Siy = xo._mv(Si, y)
                nis = (y * Siy).sum(axis=1)
                lds = 2 * A.log(np.stack([L[:, i, i] for i in range(m)], axis=1)).sum(axis=1)
                idx = np.arange(m)
                rec_upd.append((g.copy(), np.abs(Siy), np.abs(Si), np.sqrt(Pp[:, idx, idx])))
            else:
                nis = (xo._mv(np.linalg.inv(S), y) * y).sum(axis=1)
                lds = np.linalg.slogdet(S)[1]
                assert nis.dtype == A.dtype and lds.dtype == A.dtype
            sc[0] += g
            sc[1] += np.where(g, nis.astype(acc), 0)
            sc[2] += np.where(g, lds.astype(acc), 0)
            xg, Pg = _update(A, xp, Pp, m, r, zt, joseph)
            x, P = np.where(g[:, None], xg, xp), np.where(g[:, None, None], Pg, Pp)
            applied[t] = g
        xs[t], Ps[t] = x, P
        if trk is not None:
            tk = np.asarray(trk[t], np.float64).T                       # [B, d]
            have = ~np.isnan(tk).any(axis=1)
            e = x[:, :m].astype(acc) - np.where(have[:, None], tk, 0.0).astype(acc)
            sc[6] += have
            sc[7] += np.where(have, (e * e).sum(axis=1), 0)
            rec_pos.append((have, np.abs(e)))
    out = dict(scores=sc, x=xs, P=Ps, applied=applied)
    if floors:
        assert arith == 'longdouble'
        fl = LD(xo.FLOOR[dtype])
        sdmax = np.zeros((B, n), dtype=LD)
        for g, _, _, sd in rec_upd:
            sdmax[:, :m] = np.where(g[:, None], np.maximum(sdmax[:, :m], sd), sdmax[:, :m])
        comp = np.maximum(np.abs(xs).max(axis=0), sdmax)                # [B, n]
        scale = np.zeros((B, n), dtype=LD)
        for ii in M.groups.values():
            scale[:, ii] = comp[:, ii].max(axis=1, keepdims=True)
        dx = fl * scale
        floor = np.zeros((8, B), dtype=LD)
        for g, aSiy, aSi, sd in rec_upd:
            dy = dx[:, :m]
            dS = fl * sd[:, :, None] * sd[:, None, :]
            nis_f = 2 * (aSiy * dy).sum(axis=1) + (aSiy[:, :, None] * dS * aSiy[:, None, :]).sum(axis=(1, 2))
            floor[1] += np.where(g, nis_f, 0)
            floor[2] += np.where(g, (aSi * dS).sum(axis=(1, 2)), 0)
        for have, ae in rec_pos:
            floor[7] += np.where(have, 2 * (ae * dx[:, :m]).sum(axis=1), 0)
        out['floor'] = floor
    return out


def joint_fixes(model, x0, dt_steps, u, update_every, K=None):
    """Filter 0's stacked fixes as one Gaussian, from F, Q, G u, P0 and R alone (no filter), in
    longdouble: (mean [U d], covariance [U d, U d]).  x_t = F_t x_{t-1} + G_t u_t + w_t, w_t ~ N(0,
    Q dt_t), x_{-1} ~ N(x0, P0); fix j observes the positions of step (j + 1) k - 1 with noise R."""
    A = xo._LongDouble
    M = xo._rounded_model(model, None, 'f64')
    n, m = M.n, M.m
    qf, rf = _consts(model, 'f64', 1, None, K)
    q, r = A.conv(qf[0]), A.conv(rf[0])
    T, k = len(dt_steps), update_every
    dts = A.conv(np.asarray(dt_steps, np.float64))
    us = A.conv(np.asarray(u, np.float64))[:, :, 0] if u is not None else np.zeros((T, M.c), LD)
    mean, Sig = A.conv(x0[0]).copy(), A.conv(M.P0()).copy()
    Fs, means, Sigs = [], [], []
    for t in range(T):
        F, G = cvo._FG(M, A, dts[t], 1)
        F, G = F[0], G[0]
        mean = F @ mean + G @ us[t]
        Sig = F @ Sig @ F.T
        for i in range(n):
            Sig[i, i] += q[i] * dts[t]
        Fs.append(F)
        means.append(mean.copy())
        Sigs.append(Sig.copy())
    steps = [t for t in range(T) if (t + 1) % k == 0]
    U = len(steps)
    mu = np.concatenate([means[t][:m] for t in steps])
    C = np.zeros((U * m, U * m), LD)
    for a, ta in enumerate(steps):
        for b in range(a, U):
            tb = steps[b]
            Phi = np.zeros((n, n), LD)
            for i in range(n):
                Phi[i, i] = 1
            for t in range(ta + 1, tb + 1):
                Phi = Fs[t] @ Phi
            blk = (Phi @ Sigs[ta])[:m, :m]                              # Cov(x_tb, x_ta), positions
            C[b * m:(b + 1) * m, a * m:(a + 1) * m] = blk
            C[a * m:(a + 1) * m, b * m:(b + 1) * m] = blk.T
        for i in range(m):
            C[a * m + i, a * m + i] += r[i]
    return mu, C
