"""The dense gated filter with kf_run_sweep_scores' eight score rows, as truth and as plain
references — TEST INFRASTRUCTURE ONLY (no GPU, nothing of kfmi).

``run`` is one filter of ``extended_oracle``'s models over one event stream, in one of its three
arithmetics: ``'longdouble'`` (the truth: Cholesky solves written out, simple-form update),
``'f64'`` (ordinary NumPy float64: ``np.linalg.inv`` / ``slogdet``, simple form) and ``'f32'``
(ordinary NumPy float32, Joseph's form, as ``run_plain_f32``).  It gates by its own
``logdet(P_pred) > thr`` or by a caller-given ``applied`` mask, and accumulates, for every applied
update, the innovation statistics of the step itself — S = H P_pred H^T + R, y = z - H x_pred with
z the fix or the IMU pseudo-measurement from the predicted state — and, after every event whose
track row holds no NaN in the columns the model reads, the squared position error.  The plain
references form each term in their own precision and sum in float64 (the scores are doubles
whatever the filter's dtype); the truth sums in longdouble.

With ``floors=True`` (the truth run) it also returns each float row's floor scale: the first-order
effect on that row of the state and covariance errors the project already accepts per component,
``extended_oracle.FLOOR[dtype]`` times the component group's scale for a state (``errors()``'s
scale_g) and times ``sd_i sd_j`` for a covariance entry:
    NIS       sum_t 2 |S^-1 y|^T dy + |S^-1 y|^T dS |S^-1 y|
    logdet S  sum_t sum_ab |S^-1_ab| dS_ab
    pos_sse   sum_t 2 |e|^T dx_pos
dy_a being the sum of the allowed errors of the state components y_a reads (a fix row: its
position; an IMU position row: position and velocity, the pseudo-measurement being position +
velocity dt; every other IMU row: its own component).  An innovation of 1.5 m between 300 m
coordinates carries the 300 m's digits, which is why the floor is propagated through the rows'
formulas and the state budgets' floor is not reused as it stands.
"""
import numpy as np

import extended_oracle as xo

LD = xo.LD
GPS, IMU, PREDICT, NONE = xo.GPS, xo.IMU, xo.PREDICT, xo.NONE
ROWS = ('gps_n', 'gps_nis', 'gps_logdet_s', 'imu_n', 'imu_nis', 'imu_logdet_s', 'pos_n', 'pos_sse')
FLOAT_ROWS = (1, 2, 4, 5, 7)


class _Float64:
    dtype = np.float64
    own_linalg = False
    conv = staticmethod(lambda a: np.asarray(a).astype(np.float64))


def _arith(name):
    return _Float64 if name == 'f64' else xo._arith(name)


def _eye(A, n):
    I = np.zeros((1, n, n), dtype=A.dtype)
    for i in range(n):
        I[:, i, i] = 1
    return I


def _group_of(M):
    g = np.zeros(M.n, int)
    for k, ii in enumerate(M.groups.values()):
        g[ii] = k
    return g


def run(model, x0, P0, etype, dt, pay, K=None, dtype='f64', arith='longdouble', thr=-np.inf, applied=None,
        track=None, floors=False, keep_innov=False):
    """One filter: x0 [n], P0 [n, n], etype [T], dt [T], pay [T, 9], track [T, 3] | None.  Inputs are
    rounded to the kernel's ``dtype`` first (dt and the track stay float64).  Returns a dict:
    scores [8] (longdouble for the truth, float64 otherwise), applied [T] bool, gate [T] (the gate
    quantity logdet(P_pred) at GPS / IMU events, NaN elsewhere), x [T, n], x_end, P_end, and with
    floors=True floor [8] (0 in the count rows), with keep_innov=True innov: a list of (sensor, y,
    S) as float64 per applied update."""
    A = _arith(arith)
    joseph = arith == 'f32'
    M = xo._rounded_model(model, K, dtype)
    x0, P0, pay = xo.kernel_inputs(dtype, x0, P0, pay)
    etype, dts = np.asarray(etype), A.conv(np.asarray(dt, np.float64))
    T, n, m = len(etype), M.n, M.m
    x = A.conv(x0).reshape(1, n).copy()
    P = A.conv(P0).reshape(1, n, n).copy()
    q, rg, ri = A.conv(M.q), A.conv(M.r_gps), A.conv(M.r_imu)
    pays = A.conv(pay)
    half = A.conv(0.5)[()]
    acc = LD if arith == 'longdouble' else np.float64
    sc = np.zeros(8, dtype=acc)
    flags, gate = np.zeros(T, bool), np.full(T, np.nan, dtype=LD)
    xs = np.zeros((T, n), dtype=A.dtype)
    innov = []
    # the floor's ingredients, per event (longdouble runs only): |S^-1 y|, |S^-1|, sd of P_pred, |e|
    rec = []
    I = _eye(A, n)
    for t in range(T):
        et, d = int(etype[t]), dts[t]
        if et != NONE:
            F = I.copy()
            for (i, j) in M.lin:
                F[:, i, j] = d
            for (i, j) in M.quad:
                F[:, i, j] = half * d ** 2
            xp = xo._mv(F, x)
            Pp = np.matmul(np.matmul(F, P), xo._T(F))
            for i in range(n):
                Pp[:, i, i] = Pp[:, i, i] + q[i] * d
            x, P = xp, Pp
            if et in (GPS, IMU):
                if applied is not None:
                    on = bool(applied[t])
                else:
                    gate[t] = LD(xo._logdet(A, (Pp + xo._T(Pp)) * half if A.own_linalg else Pp)[0])
                    on = bool(gate[t] > thr)
                if on:
                    k, r = (m, rg) if et == GPS else (n, ri)
                    z = pays[t][None, :m] if et == GPS else M.imu_z(xp, pays[t][None, :], np.atleast_1d(d))
                    S = Pp[:, :k, :k].copy()
                    for i in range(k):
                        S[:, i, i] = S[:, i, i] + r[i]
                    y = z - xp[:, :k]
                    if A.own_linalg:
                        L = xo._chol(A, S)
                        Si = xo._chol_solve(A, L, _eye(A, k))
                        Siy = xo._mv(Si, y)
                        nis = (y * Siy).sum()
                        lds = 2 * A.log(np.stack([L[0, i, i] for i in range(k)])).sum()
                        rec.append((t, et, np.abs(Siy[0]), np.abs(Si[0]), np.sqrt(Pp[0, np.arange(k), np.arange(k)])))
                    else:
                        nis = xo._mv(np.linalg.inv(S), y)[0].dot(y[0])
                        lds = np.linalg.slogdet(S)[1][0]
                        assert nis.dtype == A.dtype and lds.dtype == A.dtype
                    base = 0 if et == GPS else 3
                    sc[base] += 1
                    sc[base + 1] += acc(nis)
                    sc[base + 2] += acc(lds)
                    if keep_innov:
                        innov.append(('gps' if et == GPS else 'imu', np.asarray(y[0], np.float64),
                                      np.asarray(S[0], np.float64)))
                    x, P = xo._update(A, xp, Pp, k, r, z, joseph)
                    flags[t] = True
        xs[t] = x[0]
        if track is not None and not np.isnan(track[t, :m]).any():
            e = x[0, :m].astype(acc) - np.asarray(track[t, :m], np.float64).astype(acc)
            sc[6] += 1
            sc[7] += (e * e).sum()
            if floors:
                rec.append((t, 'pos', np.abs(e)))
    out = dict(scores=sc, applied=flags, gate=gate, x=xs, x_end=x[0].copy(), P_end=P[0].copy())
    if keep_innov:
        out['innov'] = innov
    if floors:
        assert arith == 'longdouble'
        fl = LD(xo.FLOOR[dtype])
        # errors()'s state scale: per group, the stream-wide max of max(|x|, sd); sd here from the
        # predicted covariances the innovations see and the end covariance
        sdmax = np.zeros(n, dtype=LD)
        for r_ in rec:
            if r_[1] != 'pos':
                k = len(r_[4])
                sdmax[:k] = np.maximum(sdmax[:k], r_[4])
        g = _group_of(M)
        comp = np.maximum(np.abs(xs).max(axis=0), sdmax)
        scale = np.array([comp[g == g[i]].max() for i in range(n)], dtype=LD)
        dx = fl * scale
        # the components an IMU row's y reads beyond its own: a position row also reads its velocity
        vel_of = {i: j for (i, j) in M.lin if i < m}
        floor = np.zeros(8, dtype=LD)
        for r_ in rec:
            if r_[1] == 'pos':
                floor[7] += 2 * (r_[2] * dx[:m]).sum()
                continue
            _, et, aSiy, aSi, sd = r_
            k = len(sd)
            dy = dx[:k].copy()
            if et == IMU:
                for i, j in vel_of.items():
                    dy[i] = dy[i] + dx[j]
            dS = fl * sd[:, None] * sd[None, :]
            base = 0 if et == GPS else 3
            floor[base + 1] += 2 * (aSiy * dy).sum() + aSiy.dot(dS).dot(aSiy)
            floor[base + 2] += (aSi * dS).sum()
        out['floor'] = floor
    return out


def innovation_nll(scores, model, sensor):
    """0.5 (NIS + logdet_S + n m log 2 pi) from a [8] score vector (the formula the engine states)."""
    m = {'ref15': (3, 15), 'ref8': (2, 8)}[model][sensor == 'imu']
    b = 0 if sensor == 'gps' else 3
    return 0.5 * (scores[b + 1] + scores[b + 2] + scores[b] * m * np.log(2 * np.pi))
