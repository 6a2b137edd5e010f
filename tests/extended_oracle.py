"""Extended-precision truth for the filter kernels, the plain same-precision references, and
the per-component error measure that judges both — TEST INFRASTRUCTURE ONLY.

``run_truth`` restates the formulas of ``oracle/ref_kf.py`` (``F_*``, ``Q_*``,
``predict_covariance``, ``update``, ``imu_pseudo_measurement15/8``, ``consts_matrices`` and
``CVModel`` with its control ``u``) in ``np.longdouble`` (x87 extended, 64-bit significand),
vectorised over filters.  The gain comes from an in-file Cholesky solve and log det from the
Cholesky diagonal (``np.linalg`` has no longdouble).  Every input is first rounded to the dtype
the kernel receives.  The same code runs on ``mpmath`` numbers (``arith='mp'``), which is how
``test_extended_oracle_cpu.py`` checks that longdouble is accurate enough to referee.

The plain references are the same steps at the kernel's own precision: ``plain_f64`` is
``ref_kf`` itself (simple form ``(I - K H) P``, ``np.linalg.inv`` / ``slogdet``), ``run_plain_f32``
is ordinary NumPy ``float32`` in Joseph's form (the fp32 kernels' form; the simple form loses
1e-3 of P in plain float32).

``errors(got, truth, groups)`` is one code path for kernel and plain reference:
* state, per component group g: max over steps and components of ``|x - x_truth| / scale_g(f)``,
  ``scale_g(f)`` the stream-wide max over the group of ``max(|x_truth|, sqrt(P_truth,ii))``;
* covariance: ``|P - P_truth| / sqrt(P_ii P_jj)``, max over entries;
* log det: absolute error; its scale is ``max(n, max |logdet_truth|)`` (log det is a sum of n
  pivot logarithms, so a relative pivot error eps moves it by up to n eps).
"""
import numpy as np

from oracle import ref_kf

LD = np.longdouble
if np.finfo(LD).nmant < 63:
    raise ImportError(
        f'extended_oracle: np.longdouble has a {np.finfo(LD).nmant + 1}-bit significand on this platform; the truth '
        f'needs the 64-bit x87 extended format (a double-width "truth" would referee nothing)')

GPS, IMU, PREDICT, NONE = 0, 1, 2, 255


# --------------------------------------------------------------------------------------------
# Models: index lists instead of matrices, so one description serves every arithmetic
# --------------------------------------------------------------------------------------------

class Model:
    """n states, GPS observes states 0..m-1, the IMU pseudo-measurement observes all (H = I).
    ``lin`` / ``quad``: the (i, j) with F[i, j] = dt / dt^2/2.  ``K``: caller constants as
    ``ref_kf.consts_matrices`` takes them (dict of q, r_imu, r_gps, p0), None = the reference's."""

    def __init__(self, name, K=None):
        self.name, self.K = name, K
        if name == 'ref15':
            self.n, self.m, self.c = 15, 3, 0
            self.lin = [(i, 6 + i) for i in range(3)] + [(3 + i, 9 + i) for i in range(3)] + \
                       [(6 + i, 12 + i) for i in range(3)]
            self.quad = [(i, 12 + i) for i in range(3)]
            q, r_imu, r_gps, p0 = ref_kf._Q15, ref_kf._RIMU15, [3.0] * 3, np.diag(ref_kf.P0_REF15)
            self.groups = {'pos': [0, 1, 2], 'att': [3, 4, 5], 'vel': [6, 7, 8], 'rate': [9, 10, 11],
                           'acc': [12, 13, 14]}
        elif name == 'ref8':
            self.n, self.m, self.c = 8, 2, 0
            self.lin = [(0, 3), (1, 4), (2, 5), (3, 6), (4, 7)]
            self.quad = [(0, 6), (1, 7)]
            q, r_imu, r_gps, p0 = ref_kf._Q8, ref_kf._RIMU8, [3.0] * 2, np.diag(ref_kf.P0_REF8)
            self.groups = {'pos': [0, 1], 'att': [2], 'vel': [3, 4], 'rate': [5], 'acc': [6, 7]}
        elif name in ('cv2', 'cv3'):
            cv = ref_kf.CV2 if name == 'cv2' else ref_kf.CV3
            d = cv.d
            self.cv = cv
            self.n, self.m, self.c = 2 * d, d, d
            self.lin = [(i, d + i) for i in range(d)]
            self.quad = []
            self.ctl_quad = [(i, i) for i in range(d)]       # G[i, i] = dt^2 / 2
            self.ctl_lin = [(d + i, i) for i in range(d)]    # G[d + i, i] = dt
            q, r_imu, r_gps = np.diag(cv.Q(1.0)), None, np.diag(cv.R())
            p0 = np.diag(cv.P0())
            self.groups = {'pos': list(range(d)), 'vel': list(range(d, 2 * d))}
        else:
            raise ValueError(name)
        if K is not None:
            q, r_imu, r_gps, p0 = (np.asarray(K[k], np.float64) for k in ('q', 'r_imu', 'r_gps', 'p0'))
            q, r_imu, p0 = q[:self.n], r_imu[:self.n], p0[:self.n]
        self.q = np.asarray(q, np.float64)
        self.r_imu = None if r_imu is None else np.asarray(r_imu, np.float64)
        self.r_gps = np.asarray(r_gps, np.float64)
        self.p0 = np.asarray(p0, np.float64)

    def P0(self):
        return np.diag(self.p0)

    def imu_z(self, xp, pay, dt):
        """imu_pseudo_measurement15 / 8: Z from the predicted state and the payload, [B, n]."""
        dtc = dt[:, None]
        if self.name == 'ref15':
            a = pay[:, 6:9]
            V = xp[:, 6:9] + a * dtc
            X = xp[:, 0:3] + V * dtc
            return np.concatenate([X, pay[:, 0:3], V, pay[:, 3:6], a], axis=1)
        a = pay[:, 6:8]
        V = xp[:, 3:5] + a * dtc
        X = xp[:, 0:2] + V * dtc
        return np.concatenate([X, pay[:, 2:3], V, pay[:, 5:6], a], axis=1)


# --------------------------------------------------------------------------------------------
# Arithmetics
# --------------------------------------------------------------------------------------------

class _LongDouble:
    dtype = LD
    own_linalg = True
    conv = staticmethod(lambda a: np.asarray(a).astype(LD))
    sqrt = staticmethod(np.sqrt)
    log = staticmethod(np.log)


class _Float32:
    dtype = np.float32
    own_linalg = False                  # ordinary NumPy: np.linalg.inv / slogdet in float32
    conv = staticmethod(lambda a: np.asarray(a).astype(np.float32))


def _mp_arith():
    import mpmath

    class _MP:
        dtype = object
        own_linalg = True
        _mpf = np.frompyfunc(lambda v: mpmath.mpf(float(v)), 1, 1)
        conv = staticmethod(lambda a: np.asarray(_MP._mpf(np.asarray(a, np.float64)), dtype=object))
        sqrt = staticmethod(np.frompyfunc(mpmath.sqrt, 1, 1))
        log = staticmethod(np.frompyfunc(mpmath.log, 1, 1))
    return _MP


def _arith(name):
    return {'longdouble': _LongDouble, 'f32': _Float32}[name] if name != 'mp' else _mp_arith()


def _T(a):
    return np.swapaxes(a, -1, -2)


def _mv(M, v):
    return np.matmul(M, v[..., None])[..., 0]


def _chol(A, S):
    """Lower Cholesky factor of the SPD [B, k, k] matrices S (their lower triangles are read)."""
    k = S.shape[-1]
    L = np.zeros(S.shape, dtype=A.dtype)
    for j in range(k):
        col = S[:, j:, j] - _mv(L[:, j:, :j], L[:, j, :j]) if j else S[:, j:, j].copy()
        d = A.sqrt(col[:, 0])
        L[:, j, j] = d
        L[:, j + 1:, j] = col[:, 1:] / d[:, None]
    return L


def _chol_solve(A, L, Y):
    """S^-1 Y for S = L L^T; Y [B, k, r]."""
    k = L.shape[-1]
    W = np.zeros(Y.shape, dtype=A.dtype)
    for i in range(k):                                  # L W = Y
        acc = Y[:, i, :] - np.matmul(L[:, i:i + 1, :i], W[:, :i, :])[:, 0, :] if i else Y[:, i, :]
        W[:, i, :] = acc / L[:, i, i][:, None]
    X = np.zeros(Y.shape, dtype=A.dtype)
    for i in range(k - 1, -1, -1):                      # L^T X = W
        acc = W[:, i, :] - np.matmul(_T(L[:, i + 1:, i:i + 1]), X[:, i + 1:, :])[:, 0, :] if i < k - 1 else W[:, i, :]
        X[:, i, :] = acc / L[:, i, i][:, None]
    return X


def _logdet(A, P):
    if not A.own_linalg:
        return np.linalg.slogdet(P)[1].astype(A.dtype)
    L = _chol(A, P)
    d = np.stack([L[:, i, i] for i in range(P.shape[-1])], axis=1)
    return 2 * A.log(d).sum(axis=1)


def _update(A, x, P, k, r, z, joseph):
    """``ref_kf.update`` with H = the first k rows of I and R = diag(r): K = (P H^T) inv(H P H^T
    + R), x += K (z - H x), P = (I - K H) P, or Joseph's (I - K H) P (I - K H)^T + K R K^T."""
    n = P.shape[-1]
    S = P[:, :k, :k].copy()
    for i in range(k):
        S[:, i, i] = S[:, i, i] + r[i]
    PHt = P[:, :, :k]
    if A.own_linalg:
        K = _T(_chol_solve(A, _chol(A, S), _T(PHt)))    # S symmetric: (P H^T) S^-1 = (S^-1 H P^T)^T
    else:
        K = np.matmul(PHt, np.linalg.inv(S))
    xn = x + _mv(K, z - x[:, :k])
    IKH = np.zeros(P.shape, dtype=A.dtype)
    for i in range(n):
        IKH[:, i, i] = 1
    IKH[:, :, :k] = IKH[:, :, :k] - K
    Pn = np.matmul(IKH, P)
    if joseph:
        Pn = np.matmul(Pn, _T(IKH)) + np.matmul(K * r[None, None, :], _T(K))
    return xn, Pn


def _run(M, A, x0, P0, etype, dt, pay, u=None, joseph=False):
    """x0 [B, n], P0 [B, n, n] | [n, n], etype [T, B], dt [T, B], pay [T, 9, B] (GPS: rows 0..m-1;
    IMU: roll, pitch, yaw, wx, wy, wz, ax, ay, az), u [T, c, B] | None, all already rounded to
    what the kernel receives.  Returns x [T, B, n], P [T, B, n, n], logdet [T, B] after each
    event, in the arithmetic's dtype."""
    T, B = etype.shape
    n = M.n
    x = A.conv(x0).copy()
    P = A.conv(np.broadcast_to(P0, (B, n, n))).copy()
    q, rg = A.conv(M.q), A.conv(M.r_gps)
    ri = A.conv(M.r_imu) if M.r_imu is not None else None
    dts, pays = A.conv(dt), A.conv(pay)
    us = A.conv(u) if u is not None else None
    half = A.conv(0.5)[()]
    xs = np.zeros((T, B, n), dtype=A.dtype)
    Ps = np.zeros((T, B, n, n), dtype=A.dtype)
    lds = np.zeros((T, B), dtype=A.dtype)
    for t in range(T):
        et, d = etype[t], dts[t]
        F = np.zeros((B, n, n), dtype=A.dtype)
        for i in range(n):
            F[:, i, i] = 1
        for (i, j) in M.lin:
            F[:, i, j] = d
        for (i, j) in M.quad:
            F[:, i, j] = half * d ** 2
        xp = _mv(F, x)
        if us is not None:
            G = np.zeros((B, n, M.c), dtype=A.dtype)
            for (i, j) in M.ctl_quad:
                G[:, i, j] = half * d ** 2
            for (i, j) in M.ctl_lin:
                G[:, i, j] = d
            xp = xp + _mv(G, _T(us[t]))
        Pp = np.matmul(np.matmul(F, P), _T(F))
        for i in range(n):
            Pp[:, i, i] = Pp[:, i, i] + q[i] * d
        p = _T(pays[t])                                 # [B, 9]
        xn, Pn = xp, Pp
        g, im = et == GPS, et == IMU
        if g.any():
            xg, Pg = _update(A, xp, Pp, M.m, rg, p[:, :M.m], joseph)
            xn, Pn = np.where(g[:, None], xg, xn), np.where(g[:, None, None], Pg, Pn)
        if im.any():
            xi, Pi = _update(A, xp, Pp, n, ri, M.imu_z(xp, p, d), joseph)
            xn, Pn = np.where(im[:, None], xi, xn), np.where(im[:, None, None], Pi, Pn)
        idle = et == NONE
        x, P = np.where(idle[:, None], x, xn), np.where(idle[:, None, None], P, Pn)
        xs[t], Ps[t] = x, P
        lds[t] = _logdet(A, (P + _T(P)) * half if A.own_linalg else P)
    return xs, Ps, lds


def kernel_inputs(dtype, *arrays):
    """The values the kernel receives: state, payloads, controls and fixes in its own dtype
    ('f64' | 'f32'), as float64 arrays (dt stays float64 in both and is not passed here)."""
    npd = {'f64': np.float64, 'f32': np.float32}[dtype]
    return tuple(None if a is None else np.asarray(a, np.float64).astype(npd).astype(np.float64) for a in arrays)


def _rounded_model(model, K, dtype):
    M = Model(model, K)
    M.q, M.r_gps, M.p0 = kernel_inputs(dtype, M.q, M.r_gps, M.p0)
    if M.r_imu is not None:
        M.r_imu, = kernel_inputs(dtype, M.r_imu)
    return M


def run_truth(model, x0, P0, etype, dt, pay, u=None, K=None, dtype='f64', arith='longdouble'):
    """The filter in extended precision on the inputs rounded to the kernel's ``dtype``.
    Returns dict(x [T, B, n], P [T, B, n, n], logdet [T, B]) of np.longdouble."""
    A = _arith(arith)
    M = _rounded_model(model, K, dtype)
    x0, P0, pay, u = kernel_inputs(dtype, x0, P0, pay, u)
    xs, Ps, lds = _run(M, A, x0, P0, np.asarray(etype), np.asarray(dt, np.float64), pay, u)
    if arith == 'mp':
        import mpmath
        # keep what longdouble can hold: the comparison is longdouble's error against these digits
        tolong = np.frompyfunc(lambda v: LD(mpmath.nstr(v, 25)), 1, 1)
        xs, Ps, lds = (tolong(a).astype(LD) for a in (xs, Ps, lds))
    return dict(x=xs, P=Ps, logdet=lds)


def run_plain_f32(model, x0, P0, etype, dt, pay, u=None, K=None):
    """The same steps in ordinary NumPy float32, Joseph's form (the fp32 kernels' form)."""
    M = _rounded_model(model, K, 'f32')
    x0, P0, pay, u = kernel_inputs('f32', x0, P0, pay, u)
    xs, Ps, lds = _run(M, _Float32, x0, P0, np.asarray(etype), np.asarray(dt, np.float64), pay, u, joseph=True)
    assert xs.dtype == np.float32 and Ps.dtype == np.float32 and lds.dtype == np.float32
    return dict(x=xs, P=Ps, logdet=lds)


def plain_f64(model, x0, P0, etype, dt, pay, K=None):
    """``ref_kf.step15`` / ``step8`` themselves, one filter at a time (float64, simple form,
    np.linalg.inv and slogdet); PREDICT events with ``predict_covariance`` alone."""
    step, Ff, Qf = ((ref_kf.step15, ref_kf.F_ref15, ref_kf.Q_ref15) if model == 'ref15' else
                    (ref_kf.step8, ref_kf.F_ref8, ref_kf.Q_ref8))
    T, B = etype.shape
    n = 15 if model == 'ref15' else 8
    if K is not None:
        Qf = ref_kf.consts_matrices(K, n)[0]
    xs, Ps, lds = np.zeros((T, B, n)), np.zeros((T, B, n, n)), np.zeros((T, B))
    P0 = np.broadcast_to(np.asarray(P0, np.float64), (B, n, n))
    for f in range(B):
        x, P = np.array(x0[f], np.float64), P0[f].copy()
        for t in range(T):
            ty, d, p = etype[t, f], dt[t, f], pay[t, :, f]
            if ty == GPS:
                x, P = step(x, P, 'GPS', {'easting': p[0], 'northing': p[1], 'altitude': p[2]}, d, K)
            elif ty == IMU:
                x, P = step(x, P, 'IMU', ['t', *p], d, K)
            elif ty == PREDICT:
                F = Ff(d)
                x, P = np.dot(F, x), ref_kf.predict_covariance(P, F, Qf(d))
            xs[t, f], Ps[t, f], lds[t, f] = x, P, np.linalg.slogdet(P)[1]
    return dict(x=xs, P=Ps, logdet=lds)


def plain_f64_cv(model, x0, dt_steps, u, z, update_every):
    """``ref_kf.run_batch`` itself: x per step, log det per step, the final P."""
    cv = ref_kf.CV2 if model == 'cv2' else ref_kf.CV3
    tr, ld, _, P = ref_kf.run_batch(cv, x0, cv.P0(), dt_steps, u, z, update_every)
    T = len(dt_steps)
    have = np.zeros(T, bool)
    have[-1] = True
    Ps = np.zeros((T,) + P.shape)
    Ps[-1] = P
    return dict(x=np.transpose(tr, (0, 2, 1)), P=Ps, logdet=ld, P_have=have)


def cv_events(model, T, B, dt_steps, z, update_every):
    """The fused run as an event stream: step t predicts with u[t]; it ends with the fix
    z[t // k] when (t + 1) % k == 0 (``ref_kf.is_update_step``)."""
    m = 2 if model == 'cv2' else 3
    etype = np.full((T, B), PREDICT, np.uint8)
    pay = np.zeros((T, 9, B))
    for t in range(T):
        if ref_kf.is_update_step(t, update_every):
            etype[t] = GPS
            pay[t, :m] = z[t // update_every]
    return etype, np.repeat(np.asarray(dt_steps, np.float64)[:, None], B, 1), pay


# --------------------------------------------------------------------------------------------
# The error measure
# --------------------------------------------------------------------------------------------

def _worst(err, have):
    """max of err over the entries ``have`` marks; a non-finite entry there is an infinite error."""
    err = np.where(np.isfinite(err), err, np.inf)
    sel = err[np.broadcast_to(have, err.shape)]
    return float(sel.max()) if sel.size else 0.0


def errors(got, truth, groups):
    """got: dict(x [T, B, n], P [T, B, n, n], logdet [T, B]) of any float dtype, with optional
    masks x_have [T] | [T, B] | [T, B, n], P_have [T] | [T, B], logdet_have [T] | [T, B] marking
    what was read back (default: everything).  truth: ``run_truth``'s dict.
    Returns {group: state error over scale, 'P': scaled covariance error, 'logdet': absolute
    error, 'logdet_scale': the smallest per-filter log-det scale}."""
    xt, Pt, lt = truth['x'], truth['P'], truth['logdet']
    T, B, n = xt.shape
    idx = np.arange(n)
    sd = np.sqrt(Pt[:, :, idx, idx])                                   # [T, B, n]
    out = {}

    def mask(key, ndim):
        h = np.asarray(got.get(key, True), bool)
        return h.reshape(h.shape + (1,) * (ndim - h.ndim))

    ex = np.abs(np.asarray(got['x']).astype(LD) - xt)
    xh = np.broadcast_to(mask('x_have', 3), ex.shape)
    for g, ii in groups.items():
        scale = np.maximum(np.abs(xt[:, :, ii]), sd[:, :, ii]).max(axis=(0, 2))   # [B]
        out[g] = _worst(ex[:, :, ii] / scale[None, :, None], xh[:, :, ii])
    eP = np.abs(np.asarray(got['P']).astype(LD) - Pt) / (sd[:, :, :, None] * sd[:, :, None, :])
    out['P'] = _worst(eP, mask('P_have', 4))
    out['logdet'] = _worst(np.abs(np.asarray(got['logdet']).astype(LD) - lt), mask('logdet_have', 2))
    out['logdet_scale'] = float(np.maximum(np.abs(lt).max(axis=0), n).min())
    return out


FLOOR = {'f64': 2.0 ** -40, 'f32': 2.0 ** -17}


def budget(e_ref, dtype, factor=8.0):
    """The budget per group from the plain reference's own error on the same inputs:
    max(factor * E_ref, floor * scale), the floor 2^-40 in fp64 (64 times the one-Newton
    reciprocal's 2^-46) and 2^-17 in fp32 (128 ulp).  State and P errors are already over their
    scale; log det's floor is multiplied by its scale."""
    fl = FLOOR[dtype]
    return {k: max(factor * v, fl * (e_ref['logdet_scale'] if k == 'logdet' else 1.0))
            for k, v in e_ref.items() if k != 'logdet_scale'}
