"""Dense NumPy restatement of the adaptive-threshold (gated) filter over event ARRAYS: the checker
of kf_run_events' gated one-filter runs (the chunked route, the chain kernel, the look-ahead
kernel) on streams too long for the list-form oracle's tests.  Shared by test_gated_oracle_cpu.py
and test_gpu_gated_oracle.py; no GPU, no library, nothing of kfmi.

Everything is fp64 and dense (15x15 / 8x8), built from oracle/ref_kf.py's matrices and steps in
the order oracle.ref_kf.run_adaptive_threshold (kf_workers.py:959-1058) and ref_kf.step8
(hw5_2.py:336-366) apply them: predict over dt, gate on sign * logdet(P_pred) > threshold
(kf_workers.py:1023-1025), then the GPS or the IMU pseudo-measurement update.  F(dt) and Q(dt) are
built once per distinct dt (the same matrices, not recomputed), and an event whose gate stays shut
records logdet(P_pred), which is the log-determinant of the covariance it leaves: the same calls on
the same numbers as the list-form oracle, so the two agree bit for bit where both apply.
"""
from collections import namedtuple

import numpy as np

from oracle import ref_kf

# include/kf.h KF_EVENT_*
GPS, IMU, PREDICT, NONE = 0, 1, 2, 255

GatedRun = namedtuple('GatedRun', 'traj logdet updated x P margin gate cov')
GatedRun.__doc__ = """run_gated's outputs: traj [T, 6] (ref8: [T, 3]) the leading states after each event,
logdet [T] the post-event slogdet, updated [T] uint8, the final dense x and P, margin the smallest
|sign * logdet(P_pred) - threshold| over the gated events (inf for a non-finite threshold), gate [T]
the gate quantity sign * logdet(P_pred) per event (NaN where none was evaluated: NONE and PREDICT
events, a non-finite threshold), cov [T, n, n] the post-event covariances or None."""


def _model(model, K):
    if model == 'ref15':
        n, w, g = 15, 6, 3
        Ff, Qf, Hg, Hi, Rg, Ri = (ref_kf.F_ref15, ref_kf.Q_ref15, ref_kf.H_gps15(), ref_kf.H_imu15(),
                                  ref_kf.R_gps15(), ref_kf.R_imu15())
        pseudo = ref_kf.imu_pseudo_measurement15
    elif model == 'ref8':
        n, w, g = 8, 3, 2
        Ff, Qf, Hg, Hi, Rg, Ri = (ref_kf.F_ref8, ref_kf.Q_ref8, ref_kf.H_gps8(), ref_kf.H_imu8(),
                                  ref_kf.R_gps8(), ref_kf.R_imu8())
        pseudo = ref_kf.imu_pseudo_measurement8
    else:
        raise ValueError(f'gated_oracle: {model!r} is not a reference model')
    if K is not None:
        Qf, Rg, Ri, _ = ref_kf.consts_matrices(K, n)
    return n, w, g, Ff, Qf, Hg, Hi, Rg, Ri, pseudo


def predicted_logdet(model, P, dt, K=None):
    """sign * logdet of the covariance P predicted over dt: the gate quantity of one event."""
    _, _, _, Ff, Qf, _, _, _, _, _ = _model(model, K)
    F = Ff(dt)
    sgn, ld = np.linalg.slogdet(ref_kf.predict_covariance(np.asarray(P, np.float64), F, Qf(dt)))
    return float(sgn * ld)


def run_gated(model, et, dt, pay, x0, P0, threshold, K=None, cov=False):
    """One gated filter over T events: et [T] uint8 (KF_EVENT_*), dt [T], pay [T, 9] (GPS: e, n,
    alt; IMU: roll, pitch, yaw, wx, wy, wz, ax, ay, az), from the dense x0 [n] and P0 [n, n].
    threshold: -inf always updates and +inf or NaN never does, neither evaluating the gate.  K:
    custom diagonal constants (ref_kf.consts_matrices) in place of the reference's getters.  GPS
    and IMU events predict and, where the gate opens, update; KF_EVENT_PREDICT only predicts;
    KF_EVENT_NONE leaves the filter unchanged and still writes its record.  cov: also every
    post-event covariance.  Returns a GatedRun."""
    n, w, g, Ff, Qf, Hg, Hi, Rg, Ri, pseudo = _model(model, K)
    et = np.asarray(et)
    dt = np.asarray(dt, np.float64)
    pay = np.asarray(pay, np.float64)
    T = len(et)
    thr = float(threshold)
    finite = np.isfinite(thr)
    always = thr == -np.inf
    x = np.array(x0, dtype=np.float64)
    P = np.array(P0, dtype=np.float64)
    traj = np.empty((T, w))
    logdet = np.empty(T)
    updated = np.zeros(T, np.uint8)
    gate = np.full(T, np.nan)
    covs = np.empty((T, n, n)) if cov else None
    margin = np.inf
    fq = {}
    ld_post = np.linalg.slogdet(P)[1]
    for t, (ty, d) in enumerate(zip(et.tolist(), dt.tolist())):
        if ty != NONE:
            if d not in fq:
                fq[d] = (Ff(d), Qf(d))
            F, Q = fq[d]
            x = np.dot(F, x)
            P = ref_kf.predict_covariance(P, F, Q)
            opened = False
            ld_pred = None
            if ty == GPS or ty == IMU:
                if finite:
                    sgn, ld_pred = np.linalg.slogdet(P)
                    q = sgn * ld_pred
                    gate[t] = q
                    margin = min(margin, abs(q - thr))
                    opened = q > thr
                else:
                    opened = always
            if opened:
                if ty == GPS:
                    x, P = ref_kf.update(x, P, Hg, Rg, [float(v) for v in pay[t, :g]])
                else:
                    x, P = ref_kf.update(x, P, Hi, Ri, pseudo(x, ['t', *pay[t].tolist()], d))
                updated[t] = 1
                ld_post = np.linalg.slogdet(P)[1]
            else:
                # the covariance the event leaves is P_pred: its slogdet, once
                ld_post = ld_pred if ld_pred is not None else np.linalg.slogdet(P)[1]
        traj[t] = x[:w]
        logdet[t] = ld_post
        if cov:
            covs[t] = P
    return GatedRun(traj, logdet, updated, x, P, float(margin), gate, covs)
