"""The reference's 15-state GPS+IMU drivers on the engine (KF_MODEL_REF15).

Same names, arguments and return layouts as the reference's methods on KF_SensorFusion, with
the event list (``indexed_sensor_data``, built by combine_sensor_data, kf_workers.py:375-385:
``[(idx, 'GPS'|'IMU', t, payload), ...]``) passed explicitly:

    run_kalman_filter_full                               kf_workers.py:623-728
    run_adaptive_threshold_kalman_filter                 kf_workers.py:959-1058
    evaluate_combo_chunk (evaluate_combo_chunk_worker)   kf_workers.py:22-97
    run_brute_force_kalman_filter_no_sampling_min_usage  kf_workers.py:1218-1392
    run_kalman_filter_scheduled                          kf_workers.py:826-957
    run_kalman_filter (states + per-step covariances)    kf_workers.py:738-824
    run_no_update_kalman_filter                          kf_workers.py:1060-1160
    scheduler_gain / scheduler_cov_trace (Scheduler)     kf_workers.py:112-185
    sampling_sweep (the driver behind sampling_sweep/kf_plot_{10..120}.png)
    search_schedules (run_brute_force_kalman_filter)     KF_SensorFusion.ipynb, the class cell

Host code here only selects events and differences their time stamps in fp64 with the
reference's rules (first-GPS start, negative-dt skips); every predict/update/logdet runs in the
HIP kernels (kf_run_events, kf_eval_combos).  Covariances cross the boundary as 15x15 NumPy
arrays (the reference's format) and are stored block-packed on the GPU: they must be
block-diagonal over the axis chains (pos,vel,acc) and (att,rate), which every covariance the
reference itself produces is, exactly (see csrc/kf_ref15.hip).
"""
from __future__ import annotations

import itertools
import math

import numpy as np
import torch

from . import _lib
from .engine import BatchedKF, SCORE_ROWS, consts_table, innovation_nll

GPS, IMU, PREDICT, NONE = _lib.KF_EVENT_GPS, _lib.KF_EVENT_IMU, _lib.KF_EVENT_PREDICT, _lib.KF_EVENT_NONE

def _block_rows(pva, aw):
    rows = []
    for blk in pva:
        rows += [(blk[a], blk[b]) for a in range(3) for b in range(a, 3)]
    for blk in aw:
        rows += [(blk[a], blk[b]) for a in range(2) for b in range(a, 2)]
    return rows


# block-packed row r -> (i, j) of the dense covariance, per model (csrc/kf_ref_model.h, include/kf.h)
_LAYOUT = {
    # n: (rows, model name) — REF15 chains (pos, vel, acc)_i = (i, 6+i, 12+i), (att, rate)_i = (3+i, 9+i)
    15: (_block_rows([(0, 6, 12), (1, 7, 13), (2, 8, 14)], [(3, 9), (4, 10), (5, 11)]), 'ref15'),
    # REF8 (hw5_2.py:219-231): (x, vx, ax), (y, vy, ay), (theta, theta_dot)
    8: (_block_rows([(0, 3, 6), (1, 4, 7)], [(2, 5)]), 'ref8'),
}
_BY_ROWS = {len(r): n for n, (r, _) in _LAYOUT.items()}
_MASK = {}
for _n, (_rows, _) in _LAYOUT.items():
    _MASK[_n] = np.zeros((_n, _n), bool)
    for _i, _j in _rows:
        _MASK[_n][_i, _j] = _MASK[_n][_j, _i] = True
_ROWS = _LAYOUT[15][0]

# reference P0 (kf_workers.py:651)
P0 = np.diag([10000.0] * 3 + [1000.0] * 3 + [1000.0] * 3 + [1000.0] * 3 + [10000.0] * 3)

# H of the models (kf_workers.py:551-579, hw5_2.py:258-278): the engine's update selects these rows
_H = {15: (np.eye(15)[:3], np.eye(15)), 8: (np.eye(8)[:2], np.eye(8))}


class ModelConsts:
    """Diagonal noise constants of a reference model (include/kf.h kf_params.ref_*): Q rates,
    R_imu, R_gps and P0 per state, in the model's state order.  The reference hard-codes them in
    its getters (kf_workers.py:519-614, P0 :651; hw5_2.py:233-304, P0 :317-326) and lets a
    caller replace the getters through its class_args dict (kf_workers.py:1242-1251); any
    diagonal choice keeps the covariance block-diagonal over the axis chains, which the engine
    stores.  ``ModelConsts('ref15')`` is the reference's."""

    def __init__(self, model='ref15', q=None, r_imu=None, r_gps=None, p0=None):
        from .engine import default_params
        if model not in ('ref15', 'ref8'):
            raise ValueError(f'ModelConsts: {model!r} is not a reference model')
        self.model = model
        self.n = 15 if model == 'ref15' else 8
        d = default_params(model)
        n, g = self.n, 3 if model == 'ref15' else 2

        def vec(v, ref, k, name):
            a = np.array(ref[:k] if v is None else v, dtype=np.float64).reshape(-1)
            if a.shape != (k,):
                raise ValueError(f'ModelConsts: {name} needs {k} values, got {a.shape}')
            return a
        self.q = vec(q, d.ref_q, n, 'q')
        self.r_imu = vec(r_imu, d.ref_r_imu, n, 'r_imu')
        self.r_gps = vec(r_gps, d.ref_r_gps, g, 'r_gps')
        self.p0 = vec(p0, d.ref_p0, n, 'p0')

    @property
    def P0(self):
        return np.diag(self.p0)

    def Q(self, dt):
        return np.diag(self.q * dt)

    @property
    def R_gps(self):
        return np.diag(self.r_gps)

    @property
    def R_imu(self):
        return np.diag(self.r_imu)

    def is_reference(self):
        return self == ModelConsts(self.model)

    def __eq__(self, other):
        return isinstance(other, ModelConsts) and self.model == other.model and all(
            np.array_equal(getattr(self, k), getattr(other, k)) for k in ('q', 'r_imu', 'r_gps', 'p0'))

    def params(self):
        """kf_params for BatchedKF(model, ..., params=...), or None for the reference's."""
        if self.is_reference():
            return None
        p = _lib.kf_params()
        for name, v in (('ref_q', self.q), ('ref_r_imu', self.r_imu), ('ref_r_gps', self.r_gps),
                        ('ref_p0', self.p0)):
            arr = getattr(p, name)
            for i, x in enumerate(v):
                arr[i] = float(x)
        return p

    def oracle(self):
        """The same constants as oracle/ref_kf.py's K argument (tests)."""
        return dict(q=self.q, r_imu=self.r_imu, r_gps=self.r_gps, p0=self.p0)

    @classmethod
    def from_matrices(cls, model='ref15', F=None, Q=None, H_gps=None, H_imu=None, R_gps=None, R_imu=None, P0=None):
        """Constants from the reference's getters or a caller's replacements (the class_args
        callables, kf_workers.py:1242-1251): F(dt), Q(dt) callables, H / R matrices, P0.  Any
        argument may be None (the reference's).  The engine runs the reference's F and H (a
        kinematic chain per axis) with Q = diag(q dt) and diagonal R, P0: anything else — a
        different F or H, a Q not of that form, an R or P0 with an off-diagonal entry — raises
        ValueError, before any GPU work."""
        c = cls(model)
        n = c.n
        if F is not None:
            from .kf_workers import _F
            from .hw5_2 import _F8
            ref_f = _F if n == 15 else _F8
            for dt in (0.5, 0.0123, 2.0):
                if not np.array_equal(np.asarray(F(dt), np.float64), ref_f(dt)):
                    raise ValueError('ModelConsts: the state transition is not the reference model\'s F(dt) '
                                     '(the engine\'s kernels run its kinematic chains)')
        for name, Hm, ref in (('H_gps', H_gps, _H[n][0]), ('H_imu', H_imu, _H[n][1])):
            if Hm is not None and not (np.shape(Hm) == ref.shape and np.array_equal(np.asarray(Hm, np.float64), ref)):
                raise ValueError(f'ModelConsts: {name} is not the reference model\'s observation matrix')

        def diag_of(M, k, name):
            M = np.asarray(M, np.float64)
            if M.shape != (k, k):
                raise ValueError(f'ModelConsts: {name} must be {k}x{k}, got {M.shape}')
            if np.any(M - np.diag(np.diag(M))):
                raise ValueError(f'ModelConsts: {name} has off-diagonal entries; the engine takes diagonal '
                                 f'noise and initial covariances (block-diagonal P over the axis chains)')
            return np.diag(M).copy()
        if Q is not None:
            q = diag_of(Q(1.0), n, 'Q(1)')
            for dt in (0.5, 0.0123, 2.0):
                if not np.allclose(diag_of(Q(dt), n, f'Q({dt})'), q * dt, rtol=1e-12, atol=0.0):
                    raise ValueError('ModelConsts: Q(dt) is not diag(q * dt), the reference\'s form '
                                     '(kf_workers.py:519-544)')
            c.q = q
        if R_gps is not None:
            c.r_gps = diag_of(R_gps, 3 if n == 15 else 2, 'R_gps')
        if R_imu is not None:
            c.r_imu = diag_of(R_imu, n, 'R_imu')
        if P0 is not None:
            c.p0 = diag_of(P0, n, 'P0')
        if np.any(c.q < 0) or np.any(c.r_gps <= 0) or np.any(c.r_imu <= 0) or np.any(c.p0 <= 0):
            raise ValueError('ModelConsts: Q rates must be >= 0 and R, P0 variances > 0')
        return c


def _params(consts):
    return consts.params() if consts is not None else None


def _p0(consts):
    return consts.P0 if consts is not None else P0


def to_blocks(P):
    """n x n (or [..., n, n]) covariance of REF15 (n = 15) or REF8 (n = 8) -> block-packed
    [..., 27 | 15]; raises ValueError if it couples different axis chains (the engine stores only
    the chain blocks)."""
    P = np.asarray(P, dtype=np.float64)
    n = P.shape[-1]
    if n not in _LAYOUT or P.shape[-2] != n:
        raise ValueError(f'expected a [..., 15, 15] or [..., 8, 8] covariance, got {P.shape}')
    off = np.abs(P[..., ~_MASK[n]])
    if off.size and off.max() > 0.0:
        raise ValueError(f'covariance couples different axis chains (max |off-block| = {off.max():g}); '
                         f'KF_MODEL_{_LAYOUT[n][1].upper()} stores the (pos,vel,acc)/(att,rate) blocks only')
    return np.stack([P[..., i, j] for i, j in _LAYOUT[n][0]], axis=-1)


def from_blocks(b):
    """block-packed [..., 27 | 15] -> 15x15 | 8x8 symmetric."""
    b = np.asarray(b, dtype=np.float64)
    n = _BY_ROWS[b.shape[-1]]
    P = np.zeros(b.shape[:-1] + (n, n))
    for r, (i, j) in enumerate(_LAYOUT[n][0]):
        P[..., i, j] = b[..., r]
        P[..., j, i] = b[..., r]
    return P


def event_payload(stype, sdata):
    """The 9 payload values of one reference event (kf_workers.py:331, 367; hw5_2.py:54 stores
    no altitude, which its 8-state model never reads)."""
    if stype == 'GPS':
        return [sdata['easting'], sdata['northing'], sdata.get('altitude', 0.0), 0, 0, 0, 0, 0, 0]
    return [float(v) for v in sdata[1:10]]


def _run_streams(streams, x0, P0b, dtype='f64', device=0, threshold=None, model='ref15', cov=False, consts=None,
                 kf=None, thresholds=None):
    """Run one event list per filter in ONE kf_run_events launch.

    streams: list (per filter) of [(type, dt, payload9)]; each stream is preceded by a NONE
    event so row 0 of the outputs holds the initial state and logdet.  x0 [B, n] and P0b
    [B, rows] are the initial states.  Returns traj [T, W, B], logdet [T, B], updated [T, B],
    x [n, B], P blocks [rows, B], status [B] (and cov [T, rows, B] with cov=True) as NumPy
    arrays.  consts: a ModelConsts (None = the reference's constants).  kf: a handle of this
    model, batch, dtype and constants to run on (kept open), instead of a new one.  thresholds
    [B]: a gate per filter (kf_run_events_gates) instead of the one ``threshold``."""
    B = len(streams)
    T = 1 + max((len(s) for s in streams), default=0)
    etype = np.full((T, B), NONE, np.uint8)
    dt = np.zeros((T, B))
    pay = np.zeros((T, 9, B))
    for f, s in enumerate(streams):
        for t, (ty, d, p) in enumerate(s, start=1):
            etype[t, f] = ty
            dt[t, f] = d
            pay[t, :, f] = p
    own = kf is None
    if own:
        kf = BatchedKF(model, B, dtype, device=device, params=_params(consts))
    npd = np.float64 if dtype == 'f64' else np.float32
    kf.set_state(np.ascontiguousarray(np.asarray(x0, np.float64).T.astype(npd)),
                 np.ascontiguousarray(np.asarray(P0b, np.float64).T.astype(npd)))
    if thresholds is not None:
        tr, ld, up, cv = kf.run_events_gates(etype, dt, pay.astype(npd), np.asarray(thresholds, np.float64),
                                             updated=True, cov=cov)
    else:
        tr, ld, up, cv = kf.run_events(etype, dt, pay.astype(npd), updated=True, threshold=threshold, cov=cov)
    x, Pb = kf.state()
    st = kf.status()
    torch.cuda.synchronize(kf.device)
    out = (tr.double().cpu().numpy(), ld.double().cpu().numpy(), up.cpu().numpy(), x.double().cpu().numpy(),
           Pb.double().cpu().numpy(), st.cpu().numpy())
    if cov:
        out += (cv.double().cpu().numpy(),)
    if own:
        kf.close()
    return out


def _window(events, start_idx, end_idx):
    if start_idx is None or start_idx < 0:
        start_idx = 0
    if end_idx is None or end_idx > len(events):
        end_idx = len(events)
    return start_idx, end_idx


def _driver_stream(window, prev, rule, predict_only=False):
    """The (type, dt, payload) stream a list driver builds from the events ``window`` after a
    state at time ``prev``, with its dt < 0 rule: _lib.KF_DT_FULL (run_kalman_filter_full,
    kf_workers.py:683-685) skips the event and moves the previous time to it, KF_DT_MONOTONE
    (the adaptive and no-update drivers, :1013-1015, :1113-1116) skips it and leaves the previous
    time alone.  ``predict_only``: every kept event as a KF_EVENT_PREDICT with a zero payload
    (run_no_update_kalman_filter).  Returns (stream, times of the kept events, their positions
    in the window, previous time after the window)."""
    stream, times, kept = [], [], []
    for j, (_, stype, t, sdata) in enumerate(window):
        dt = t - prev
        if dt < 0:
            if rule == _lib.KF_DT_FULL:
                prev = t
            continue
        if predict_only:
            stream.append((PREDICT, dt, [0.0] * 9))
        else:
            stream.append((GPS if stype == 'GPS' else IMU, dt, event_payload(stype, sdata)))
        times.append(t)
        kept.append(j)
        prev = t
    return stream, times, kept, prev


def _cold_start(events, start_idx, stop):
    """First GPS fix in events[start_idx:stop]: (x0, t0, absolute index) or None
    (kf_workers.py:655-666)."""
    for i, (_, stype, t, sdata) in enumerate(events[start_idx:stop]):
        if stype == 'GPS':
            x = np.zeros(15)
            x[0], x[1], x[2] = sdata['easting'], sdata['northing'], sdata['altitude']
            return x, t, start_idx + i
    return None


def run_kalman_filter_full(events, start_idx=None, end_idx=None, initial_pt=None, initial_state=None,
                           print_output=False, dtype='f64', device=0, consts=None):
    """kf_workers.py:623-728 on the GPU: returns (states, logdets, P, prev_time) in the
    reference's layout (states = [(t, x, y, z, roll, pitch, yaw), ...]).  ``events`` is the
    reference's event list or a kfmi.ingest.EventStream (then the whole window runs from HBM:
    run_full_stream, with the lists built from its arrays)."""
    from .ingest import EventStream
    if isinstance(events, EventStream):
        r = run_full_stream(events, start_idx, end_idx, initial_pt, initial_state, dtype, consts=consts)
        if r is None:
            return [], [], []
        t, traj, ld, P, prev = r
        states = [(float(t[i]), *traj[i]) for i in range(len(t))]
        if print_output:
            print(f'Full Kalman Filter (GPU): processed {len(t) - 1} measurements')
        return states, [float(v) for v in ld], P, prev
    if not events:
        return [], [], []
    start_idx, end_idx = _window(events, start_idx, end_idx)
    x0 = np.zeros(15)
    if initial_pt is not None and initial_state is not None:
        P = np.asarray(initial_pt, np.float64)
        x0[0:6] = initial_state[1:7]
        prev = initial_state[0]
        start_off = start_idx
    else:
        P = _p0(consts)
        cs = _cold_start(events, start_idx, end_idx + 1)
        if cs is None:
            return [], [], []
        x0, prev, start_off = cs
    stream, times, _, prev = _driver_stream(events[start_off:end_idx], prev, _lib.KF_DT_FULL)
    tr, ld, _, x, Pb, st = _run_streams([stream], x0[None], to_blocks(P)[None], dtype, device, consts=consts)
    states = [(initial_state[0] if (initial_pt is not None and initial_state is not None) else
               events[start_off][2], *tr[0, :, 0])]
    states += [(t, *tr[i + 1, :, 0]) for i, t in enumerate(times)]
    logdets = [float(v) for v in ld[:len(times) + 1, 0]]
    if print_output:
        print(f'Full Kalman Filter (GPU): processed {len(times)} measurements from index {start_off} to {end_idx}')
    return states, logdets, from_blocks(Pb[:, 0]), prev


def run_full_stream(stream, start_idx=None, end_idx=None, initial_pt=None, initial_state=None, dtype='f64',
                    cov=False, parallel=True, parallel_min_events=1 << 16, consts=None):
    """run_kalman_filter_full (kf_workers.py:623-728) over an EventStream window, entirely on
    the device: cold-start fix search, per-event dt with the driver's dt < 0 rule
    (kf_events_dt, KF_DT_FULL) and one single-filter kf_run_events launch — or, for windows of
    at least ``parallel_min_events`` events, kf_run_stream (chunks of the window as filters of
    one launch, checked on the device, with the single filter as its fallback).  Returns NumPy
    (t [R], traj [R, 6], logdet [R], P 15x15, prev_time) with R = 1 + processed events (plus
    the block-packed per-record covariances [R, 27] with cov=True), or None when a cold window
    holds no fix."""
    from .ingest import events_dt
    n = len(stream)
    start_idx = 0 if start_idx is None or start_idx < 0 else int(start_idx)
    end_idx = n if end_idx is None or end_idx > n else int(end_idx)
    dev = stream.t.device
    x0 = np.zeros(15)
    if initial_pt is not None and initial_state is not None:
        P = np.asarray(initial_pt, np.float64)
        x0[0:6] = initial_state[1:7]
        prev0 = float(initial_state[0])
        start_off = start_idx
        t_first = prev0
    else:
        P = _p0(consts)
        win = stream.etype[start_idx:min(end_idx + 1, n)]  # the reference searches [start, end] (:655)
        hit = torch.nonzero(win == GPS)
        if hit.numel() == 0:
            return None
        start_off = start_idx + int(hit[0, 0])
        p = stream.payload[start_off].cpu().numpy()
        x0[0:3] = p[0:3]
        prev0 = float(stream.t[start_off])
        t_first = prev0
    T = max(end_idx - start_off, 0)
    kf = BatchedKF('ref15', 1, dtype, device=dev.index or 0, params=_params(consts))
    npd = np.float64 if dtype == 'f64' else np.float32
    kf.set_state(x0[:, None].astype(npd), to_blocks(P)[:, None].astype(npd))
    t = stream.t[start_off:start_off + T]
    dt, et = events_dt(t, prev0, _lib.KF_DT_FULL, stream.etype[start_off:start_off + T])
    pay = stream.payload[start_off:start_off + T]
    if dtype != 'f64':
        pay = pay.float()
    # a NONE event first records the initial state and logdet (states[0], logdets[0])
    et = torch.cat([torch.full((1,), NONE, dtype=torch.uint8, device=dev), et])
    dt = torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), dt])
    pay = torch.cat([torch.zeros(1, 9, dtype=pay.dtype, device=dev), pay])
    if parallel and T + 1 >= parallel_min_events:
        tr, ld, _, cv = kf.run_stream(et, dt, pay, cov=cov)
    else:
        # parallel=False: the single filter even where kf_run_events would route it over time
        tr, ld, _, cv = kf.run_events(et[:, None], dt[:, None], pay[:, :, None], cov=cov, sequential=not parallel)
    x, Pb = kf.state()
    keep = et != NONE
    keep[0] = True
    t_all = torch.cat([torch.full((1,), t_first, dtype=torch.float64, device=dev), t])
    prev = float(t[-1]) if T else prev0
    out = (t_all[keep].cpu().numpy(), tr[keep, :, 0].double().cpu().numpy(), ld[keep, 0].double().cpu().numpy(),
           from_blocks(Pb[:, 0].double().cpu().numpy()), prev)
    if cov:
        out += (cv[keep, :, 0].double().cpu().numpy(),)
    kf.close()
    return out


# --------------------------------------------------------------------------------------------
# One filter over a long stream, parallel over time (run_kalman_filter_full's own use: one
# filter over a whole drive log, kf_workers.py:623-728)
# --------------------------------------------------------------------------------------------

# the checks of the last run_stream_parallel call (diagnostics)
parallel_check = {}


def run_stream_parallel(et, dt, pay, x0, P0b, chunk=None, warmup=None, dtype='f64', cov=False, options=None,
                        consts=None):
    """One filter over a long event stream, parallel over time (kf_run_stream): et [T] uint8,
    dt [T] float64 (the driver's dt rule already applied), pay [T, 9] on the device; x0 [15], P0b
    [27] block-packed initial state.  Returns (traj [T, 6], logdet [T], x [15], P blocks [27],
    cov [T, 27] or None) on the device.  The chunked records stand only if the device checks
    pass (warm-up covariances meet their predecessors' end covariances, chunk end states meet
    the next starts, no chunk filter failed); otherwise the library's sequential fallback has
    rewritten them.  ``parallel_check`` holds the verdict and the measured gaps.  ``options``:
    BatchedKF options of the handle (e.g. stream_final='on')."""
    dev = et.device
    npd = torch.float64 if dtype == 'f64' else torch.float32
    kf = BatchedKF('ref15', 1, dtype, device=dev.index or 0, options=options, params=_params(consts))
    try:
        kf.set_state(torch.as_tensor(np.asarray(x0, np.float64).reshape(15, 1), dtype=npd, device=dev),
                     torch.as_tensor(np.asarray(P0b, np.float64).reshape(27, 1), dtype=npd, device=dev))
        tr, ld, _, cv = kf.run_stream(et, dt, pay.to(npd), cov=cov, chunk=chunk or 0,
                                      warmup=-1 if warmup is None else warmup)
        x, P = kf.state()
        parallel_check.clear()
        parallel_check.update(kf.stream_check())
        return tr[:, :, 0], ld[:, 0], x[:, 0], P[:, 0], (cv[:, :, 0] if cov else None)
    finally:
        kf.close()


def _device_stream(events):
    """The kfmi.ingest.EventStream behind ``events`` (the stream itself, or an event list over
    one: kfmi.kf_workers.EventList after combine_sensor_data), or None for a plain list."""
    from .ingest import EventStream
    if isinstance(events, EventStream):
        return events
    s = getattr(events, 's', None)
    return s if isinstance(s, EventStream) else None


def run_monotone_stream(stream, start_idx=None, end_idx=None, initial_pt=None, initial_state=None, dtype='f64',
                        consts=None, threshold=None, predict_only=False):
    """The adaptive-threshold (``threshold``, kf_workers.py:959-1058) and no-update
    (``predict_only``, :1060-1160) drivers over an EventStream window, on the device: the cold
    start's first fix in [start, end) (:990-1000), the drivers' dt rule — a dt < 0 event is skipped
    without advancing the previous time (kf_events_dt KF_DT_MONOTONE) — and one single-filter
    kf_run_events launch (the gate on logdet(P_pred) needs the filter's own history, so it runs in
    time order).  The Python loop over the event list it replaces built a tuple and three array
    entries per event (0.49 s for the 82,570 events up to the visualizing run's start).  Returns
    NumPy (t [R], traj [R, 6], logdet [R], P 15x15, previous_time, measurement_times) with R = 1 +
    processed events, or None when a cold window holds no fix."""
    from .ingest import events_dt
    n = len(stream)
    start_idx = 0 if start_idx is None or start_idx < 0 else int(start_idx)
    end_idx = n if end_idx is None or end_idx > n else int(end_idx)
    dev = stream.t.device
    x0 = np.zeros(15)
    mtimes = []
    if initial_pt is not None and initial_state is not None:
        P = np.asarray(initial_pt, np.float64)
        x0[0:6] = initial_state[1:7]
        prev0 = float(initial_state[0])
        start_off = start_idx
    else:
        P = _p0(consts)
        hit = torch.nonzero(stream.etype[start_idx:end_idx] == GPS)
        if hit.numel() == 0:
            return None
        start_off = start_idx + int(hit[0, 0])
        x0[0:3] = stream.payload[start_off, 0:3].double().cpu().numpy()
        prev0 = float(stream.t[start_off])
        mtimes.append(prev0)
    T = max(end_idx - start_off, 0)
    t = stream.t[start_off:start_off + T]
    dt, et = events_dt(t, prev0, _lib.KF_DT_MONOTONE, stream.etype[start_off:start_off + T])
    if predict_only:
        et = torch.where(et != NONE, torch.full_like(et, PREDICT), et)
        pay = torch.zeros(T, 9, dtype=torch.float64, device=dev)
    else:
        pay = stream.payload[start_off:start_off + T].double()
    if dtype != 'f64':
        pay = pay.float()
    # a NONE event first records the initial state and logdet (states[0], logdets[0])
    et = torch.cat([torch.full((1,), NONE, dtype=torch.uint8, device=dev), et])
    dt = torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), dt])
    pay = torch.cat([torch.zeros(1, 9, dtype=pay.dtype, device=dev), pay])
    kf = BatchedKF('ref15', 1, dtype, device=dev.index or 0, params=_params(consts))
    try:
        npd = np.float64 if dtype == 'f64' else np.float32
        kf.set_state(x0[:, None].astype(npd), to_blocks(P)[:, None].astype(npd))
        tr, ld, up, _ = kf.run_events(et[:, None], dt[:, None], pay[:, :, None], updated=True,
                                      threshold=None if threshold is None else float(threshold))
        x, Pb = kf.state()
        keep = et != NONE
        keep[0] = True
        t_all = torch.cat([torch.full((1,), prev0, dtype=torch.float64, device=dev), t.double()])
        upd = up[:, 0].bool() & keep
        upd[0] = False
        tk = t_all[keep]
        prev = float(tk[-1]) if tk.numel() > 1 else prev0
        out = (tk.cpu().numpy(), tr[keep, :, 0].double().cpu().numpy(), ld[keep, 0].double().cpu().numpy(),
               from_blocks(Pb[:, 0].double().cpu().numpy()), prev, mtimes + t_all[upd].cpu().tolist())
    finally:
        kf.close()
    return out


def _stream_states(t, traj):
    """[(t, x, y, z, roll, pitch, yaw), ...] from run_*_stream's arrays."""
    return list(zip(t.tolist(), *traj.T.tolist()))


def run_adaptive_threshold_kalman_filter(events, start_idx=None, end_idx=None, R_threshold=None,
                                         initial_pt=None, initial_state=None, print_output=False,
                                         dtype='f64', device=0, consts=None):
    """kf_workers.py:959-1058 on the GPU: the update is applied only when logdet(P_pred) >
    R_threshold.  Returns (states, logdets, P, previous_time, measurement_times).  Over an
    ingested stream (or an event list over one) the window never leaves the device
    (run_monotone_stream)."""
    if R_threshold is None:
        R_threshold = -float('inf')
    ds = _device_stream(events)
    if ds is not None:
        r = run_monotone_stream(ds, start_idx, end_idx, initial_pt, initial_state, dtype, consts,
                                threshold=float(R_threshold))
        if r is None:
            return None
        t, traj, ld, P, prev, mtimes = r
        if print_output:
            print(f'Adaptive Kalman Filter (GPU): processed {len(t) - 1} events')
        return _stream_states(t, traj), ld.tolist(), P, prev, mtimes
    start_idx, end_idx = _window(events, start_idx, end_idx)
    x0 = np.zeros(15)
    mtimes = []
    if initial_pt is not None and initial_state is not None:
        P = np.asarray(initial_pt, np.float64)
        x0[0:6] = initial_state[1:7]
        prev = initial_state[0]
        start_off = start_idx
    else:
        P = _p0(consts)
        cs = _cold_start(events, start_idx, end_idx)
        if cs is None:
            return None
        x0, prev, start_off = cs
        mtimes.append(prev)
    t_first = prev
    # kf_workers.py:1013-1015 assigns an unused name, so a skipped event does NOT advance previous_time
    stream, times, _, prev = _driver_stream(events[start_off:end_idx], prev, _lib.KF_DT_MONOTONE)
    tr, ld, up, x, Pb, st = _run_streams([stream], x0[None], to_blocks(P)[None], dtype, device,
                                         threshold=float(R_threshold), consts=consts)
    states = [(t_first, *tr[0, :, 0])] + [(t, *tr[i + 1, :, 0]) for i, t in enumerate(times)]
    logdets = [float(v) for v in ld[:len(times) + 1, 0]]
    mtimes += [t for i, t in enumerate(times) if up[i + 1, 0]]
    if print_output:
        print(f'Adaptive Kalman Filter (GPU): processed {len(times)} events from index {start_off} to {end_idx}')
    return states, logdets, from_blocks(Pb[:, 0]), prev, mtimes


class AdaptiveSweep:
    """run_adaptive_threshold_kalman_filter (kf_workers.py:959-1058) over ONE window under every
    threshold of ``thresholds`` at once (kf_run_sweep: one launch, 8 thresholds per wave), as the
    experiment loop draws them (:2298-2317).  ``events``: an ingested stream (or an event list
    over one), whose window never leaves the device, or a plain event list.  The drivers' rules
    are run_monotone_stream's and the list path's: the cold start is the first fix in the
    window, a dt < 0 event is skipped without advancing the previous time (here a NONE event, so
    array entry 1 + j is event start + j), and a leading NONE event records the initial state.
    The sweep's arrays stay on the device.

    ``thresholds`` / ``n_updates``: NumPy [B].  ``result(i)``: the 5-tuple the driver returns
    for thresholds[i] (needs records=True).  ``warm_start(i, end_idx)``: (states[-1], P,
    previous_time) of the driver over [start_idx, end_idx), from the checkpoint at or before
    end_idx (every ``checkpoint_every`` array entries) and a one-filter sweep over the fewer than
    checkpoint_every events after it.  ``warm_starts(index, end_idxs)``: the list of
    warm_start(index[w], end_idxs[w]), every tail in one launch (kf_run_tails).

    ``smooth=True`` (f64 only; 'full' keeps the smoothed covariances too) adds the fixed-interval
    smoother: the forward launch runs with checkpoint_every = 1, so its checkpoint arrays are the
    filtered record (336 B per entry and filter; KFError(KF_ENOMEM) before anything runs if the
    records do not fit the device's free memory) and warm_start reads its row directly, then one
    kf_smooth_sweep runs over it.  ``smoothed(i)``: (states, logdets) shaped like result(i)'s,
    the estimate of every entry given the whole window.  result(i) and warm_start are the
    smooth=False object's.  The smoothed positions with the entries' times are a ``track`` as
    they are:
        states, _ = AdaptiveSweep(events, [-np.inf], smooth=True).smoothed(0)
        track = (np.array([s[0] for s in states]), np.array([s[1:4] for s in states]))
        ParameterSweep(events, sets, scores=True, track=track).best('pos_rmse')

    ``em=True`` (needs smooth) makes the backward launch kf_smooth_sweep_em: the forward launch also
    records ``updated`` (even with records=False), and ``.em`` is the EM statistics for the
    diagonals of Q, R_imu and R_gps, a NumPy [36, B] table (engine.ref_em_rows('ref15'); the leading
    NONE entry makes "event 0 is not counted" lossless here).  ``.em_update(imu_rows='measured')``:
    the list of B ModelConsts after one M-step (engine.ref_em_update), each keeping its set's P0.
    fit_noise iterates it."""

    def __init__(self, events, thresholds, start_idx=None, end_idx=None, initial_pt=None, initial_state=None,
                 dtype='f64', device=0, consts=None, records=True, checkpoint_every=4096, scores=False, track=None,
                 smooth=False, em=False, _run=True):
        from .ingest import events_dt
        self.em = None
        if em and not smooth:
            raise ValueError('em=True needs smooth=True (the statistics are the smoother\'s)')
        self.thresholds = np.array(thresholds, dtype=np.float64).reshape(-1)
        self.dtype, self.consts, self.records = dtype, consts, bool(records)
        self.scored, self.scores = bool(scores), None
        self.every = int(checkpoint_every)
        self.smooth = smooth
        if smooth:
            if smooth is not True and smooth != 'full':
                raise ValueError(f'smooth: True, False or \'full\', got {smooth!r}')
            if dtype != 'f64':
                raise _lib.KFError(_lib.KF_EINVAL, f'smooth=True needs dtype=\'f64\', got {dtype!r} (the smoother '
                                                   f'is f64 only)')
            self.every = 1  # the filtered record is the checkpoint array: a row per entry
        self.n_updates = np.zeros(len(self.thresholds), np.int64)
        self.empty = True  # a cold window without a fix: the driver returns None
        self._kf1, self._kft = None, {}  # warm_start's one-filter handle; warm_starts' handles by batch size
        B = len(self.thresholds)
        ds = _device_stream(events)
        n = len(ds) if ds is not None else len(events)
        start_idx = 0 if start_idx is None or start_idx < 0 else int(start_idx)
        end_idx = n if end_idx is None or end_idx > n else int(end_idx)
        self.start_idx, self.end_idx = start_idx, end_idx
        warm = initial_pt is not None and initial_state is not None
        x0 = np.zeros(15)
        if warm:
            P = np.asarray(initial_pt, np.float64)
            x0[0:6] = initial_state[1:7]
            prev0 = float(initial_state[0])
            start_off = start_idx
        else:
            P = _p0(consts)
            if ds is not None:
                hit = torch.nonzero(ds.etype[start_idx:end_idx] == GPS)
                if hit.numel() == 0:
                    return
                start_off = start_idx + int(hit[0, 0])
                x0[0:3] = ds.payload[start_off, 0:3].double().cpu().numpy()
                prev0 = float(ds.t[start_off])
            else:
                cs = _cold_start(events, start_idx, end_idx)
                if cs is None:
                    return
                x0, prev0, start_off = cs
        self.empty = B == 0
        self.cold, self.prev0, self.start_off = not warm, prev0, start_off
        T = max(end_idx - start_off, 0)
        self.dev = ds.t.device if ds is not None else torch.device('cuda', device)
        dev = self.dev
        tdt = torch.float64 if dtype == 'f64' else torch.float32
        if ds is not None:
            t = ds.t[start_off:start_off + T]
            dt, et = events_dt(t, prev0, _lib.KF_DT_MONOTONE, ds.etype[start_off:start_off + T])
            pay = ds.payload[start_off:start_off + T].to(tdt)
            t_host = t.double().cpu().numpy()
            keep = et.cpu().numpy() != NONE
        else:
            t_host = np.zeros(T)
            keep = np.zeros(T, bool)
            et_h = np.full(T, NONE, np.uint8)
            dt_h = np.zeros(T)
            pay_h = np.zeros((T, 9))
            prev = prev0
            for j, (_, stype, tj, sdata) in enumerate(events[start_off:end_idx]):
                t_host[j] = tj
                d = tj - prev
                if d < 0:  # kf_workers.py:1013-1015: skipped, previous_time NOT advanced
                    continue
                keep[j] = True
                et_h[j] = GPS if stype == 'GPS' else IMU
                dt_h[j] = d
                pay_h[j] = event_payload(stype, sdata)
                prev = tj
            et = torch.from_numpy(et_h).to(dev)
            dt = torch.from_numpy(dt_h).to(dev)
            pay = torch.from_numpy(pay_h).to(dev).to(tdt)
        # a NONE event first records the initial state and logdet (states[0], logdets[0])
        self._et = torch.cat([torch.full((1,), NONE, dtype=torch.uint8, device=dev), et])
        self._dt = torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), dt])
        self._pay = torch.cat([torch.zeros(1, 9, dtype=tdt, device=dev), pay])
        self._t = np.concatenate([[prev0], t_host])
        self._keep = np.concatenate([[True], keep])
        # time of the last processed entry at or before each entry (the driver's previous_time)
        last = np.maximum.accumulate(np.where(self._keep, np.arange(T + 1), 0))
        self._prev = self._t[last]
        self._x0 = torch.as_tensor(x0[:, None], dtype=tdt, device=dev)
        self._P0 = torch.as_tensor(to_blocks(P)[:, None], dtype=tdt, device=dev)
        # ParameterSweep: a constant set per filter, [R, B] on the device, and on a cold start each
        # set's own P0 as that filter's column
        sets = getattr(self, '_sets', None)
        self._table = None
        if sets is not None:
            self._table = torch.from_numpy(consts_table('ref15', sets)).to(dev)
            if not warm:
                self._P0 = torch.as_tensor(np.stack([to_blocks(c.P0) for c in sets], 1), dtype=tdt, device=dev)
        self._kf1 = None
        if self.empty:
            return
        if self.scored:
            # the scored launch takes a table: this sweep's one constant set in every column
            if self._table is None:
                one = consts if consts is not None else ModelConsts('ref15')
                self._table = torch.from_numpy(consts_table('ref15', [one] * B)).to(dev)
            # the track at the entries' times (entry 0 is states[0], at the start time); a skipped
            # dt < 0 entry is no state of the driver's: no reference there
            if track is None and getattr(events, 'h', None) is None and ds is None:
                # a plain event list's own fixes, at the events' own times
                fixes = [(t, sd) for _, stype, t, sd in events if stype == 'GPS']
                track = (np.array([t for t, _ in fixes], np.float64),
                         np.array([[sd['easting'], sd['northing'], sd['altitude']] for _, sd in fixes], np.float64))
            tt, tp = _track_of(events, track)
            rows = track_positions(tt, tp, self._t)
            rows[~self._keep] = np.nan
            self._track = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
        if not _run:  # fit_noise: the window's arrays only
            return
        if smooth:
            # the filtered record (15 + 27 rows) and the smoothed records kept, 8 B each per entry and filter
            _smooth_memory_check(dev, T + 1, B, 15 + 27 + 6 + 1 + (27 if smooth == 'full' else 0))
        need_up = self.records or bool(em)
        kf = BatchedKF('ref15', B, dtype, device=dev.index or 0, params=_params(consts))
        try:
            kf.set_state(self._x0.expand(15, B).contiguous(), self._P0.expand(27, B).contiguous())
            if self.scored:
                r = kf.run_sweep_scores(self._et, self._dt, self._pay, self._table, torch.from_numpy(self.thresholds),
                                        track=self._track, traj=self.records, logdet=self.records,
                                        updated=need_up, checkpoint_every=self.every)
                self._traj, self._ld, self._up, nu, self._cx, self._cP = (r.traj, r.logdet, r.updated, r.n_updated,
                                                                          r.ckpt_x, r.ckpt_P)
                self.scores = _scores_dict(r.scores.cpu().numpy())
            else:
                (self._traj, self._ld, self._up, nu, self._cx, self._cP) = kf.run_sweep(
                    self._et, self._dt, self._pay, torch.from_numpy(self.thresholds), traj=self.records,
                    logdet=self.records, updated=need_up, checkpoint_every=self.every, consts=self._table)
            self._x, self._Pb = kf.state()
            self._status = kf.status()
            self.n_updates = nu.cpu().numpy().astype(np.int64)
            if smooth and em:
                sm = kf.smooth_sweep_em(self._et, self._dt, self._pay, self._up, self._cx, self._cP,
                                        consts=self._table, x=False, P=smooth == 'full', traj=True, logdet=True)
                self.em = sm.em.cpu().numpy()
            elif smooth:
                sm = kf.smooth_sweep(self._et, self._dt, self._cx, self._cP, consts=self._table, x=False,
                                     P=smooth == 'full', traj=True, logdet=True)
            if smooth:
                self._sm_traj, self._sm_ld, self._sm_P, self._sm_status = sm.traj, sm.logdet, sm.P, sm.status
        finally:
            kf.close()

    def em_update(self, imu_rows='measured'):
        """One M-step on ``.em`` (needs em=True): the list of B ModelConsts, filter i's constants
        after engine.ref_em_update with its own P0 kept.  ``imu_rows``: 'measured' | 'all' | 'none'."""
        from .engine import ref_em_update
        if self.em is None:
            raise ValueError('em_update needs em=True and a window that ran')
        sets = getattr(self, '_sets', None) or [self.consts if self.consts is not None else ModelConsts('ref15')] * \
            len(self.thresholds)
        new = ref_em_update(self.em, consts_table('ref15', sets), 'ref15', imu_rows)
        return [ModelConsts('ref15', q=new[:15, f], r_imu=new[15:30, f], r_gps=new[30:, f], p0=c.p0)
                for f, c in enumerate(sets)]

    def smoothed(self, i):
        """(states, logdets) of the fixed-interval smoother over thresholds[i]'s run (needs
        smooth=True): shaped like the first two items of result(i) and over the same kept entries,
        every state the estimate given the WHOLE window (kf_smooth_sweep over the filtered record),
        logdets the log det of the smoothed covariances.  The leading entry is the smoothed initial
        state; the last equals result(i)'s.  None where result(i) is None.  smooth='full' also keeps
        the smoothed covariances, block-packed [entries, 27, B] on the device, as ``_sm_P``."""
        if not self.smooth:
            raise ValueError('AdaptiveSweep.smoothed needs smooth=True')
        if self.empty:
            return None
        keep = torch.from_numpy(self._keep).to(self.dev)
        traj = self._sm_traj[:, :, i][keep].cpu().numpy()
        ld = self._sm_ld[:, i][keep].cpu().numpy()
        return _stream_states(self._t[self._keep], traj), ld.tolist()

    def close(self):
        if getattr(self, '_kf1', None) is not None:
            self._kf1.close()
            self._kf1 = None
        for kf in getattr(self, '_kft', {}).values():
            kf.close()
        self._kft = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def best(self, by='gps_nll'):
        """Index of the filter with the smallest finite ``scores[by]`` (needs scores=True)."""
        if self.scores is None:
            raise ValueError('best needs scores=True and a window that ran')
        v = np.asarray(self.scores[by], np.float64)
        if not np.isfinite(v).any():
            raise ValueError(f'best: no finite {by}')
        return int(np.argmin(np.where(np.isfinite(v), v, np.inf)))

    def result(self, i):
        """(states, logdets, P, previous_time, measurement_times) of
        run_adaptive_threshold_kalman_filter(..., R_threshold=thresholds[i]) over the window, or
        None where it returns None."""
        if not self.records:
            raise ValueError('AdaptiveSweep.result needs records=True')
        if self.empty:
            return None
        keep = torch.from_numpy(self._keep).to(self.dev)
        traj = self._traj[:, :, i][keep].double().cpu().numpy()
        ld = self._ld[:, i][keep].double().cpu().numpy()
        up = self._up[:, i].cpu().numpy().astype(bool) & self._keep
        up[0] = False
        mtimes = ([self.prev0] if self.cold else []) + self._t[up].tolist()
        P = from_blocks(self._Pb[:, i].double().cpu().numpy())
        return _stream_states(self._t[self._keep], traj), ld.tolist(), P, float(self._prev[-1]), mtimes

    def warm_start(self, i, end_idx):
        """(state, P, previous_time): states[-1] (a 7-tuple) and the 15x15 P that
        run_adaptive_threshold_kalman_filter(start_idx, end_idx, R_threshold=thresholds[i])
        returns, or None where it returns None (a cold window whose first fix is not before
        end_idx).  The checkpoint at or before end_idx, then a one-filter sweep over the tail
        (none for an empty tail); previous_time comes from the host's times and types, which do
        not depend on the threshold."""
        if self.empty:
            return None
        end_idx = self.end_idx if end_idx is None or end_idx > self.end_idx else int(end_idx)
        if self.cold and self.start_off >= end_idx:
            return None
        n = 1 + max(end_idx - self.start_off, 0)  # array entries of the prefix (the leading NONE included)
        c = n // self.every - 1 if self.every > 0 else -1
        if c >= 0:
            x, Pb, lo = self._cx[c][:, i:i + 1], self._cP[c][:, i:i + 1], (c + 1) * self.every
        else:
            x, Pb, lo = self._x0, self._P0[:, i:i + 1] if self._P0.shape[1] > 1 else self._P0, 0
        if n > lo:
            if self._kf1 is None:
                self._kf1 = BatchedKF('ref15', 1, self.dtype, device=self.dev.index or 0, params=_params(self.consts))
            kf = self._kf1
            kf.set_state(x.contiguous(), Pb.contiguous())
            kf.run_sweep(self._et[lo:n], self._dt[lo:n], self._pay[lo:n], self.thresholds[i:i + 1], traj=False,
                         logdet=False, counts=False,
                         consts=self._table[:, i:i + 1].contiguous() if self._table is not None else None)
            x, Pb = kf.state()
        xs = x[:6, 0].double().cpu().numpy()
        prev = float(self._prev[n - 1])
        return (prev, *xs.tolist()), from_blocks(Pb[:, 0].double().cpu().numpy()), prev

    def warm_starts(self, index, end_idxs):
        """[warm_start(index[w], end_idxs[w]) for every w], the same tuples and Nones, computed
        at once: every tail past its checkpoint in ONE run_tails launch straight from the
        sweep's checkpoint arrays (row -1: the sweep's own start state), one device-to-host copy
        and vectorised host code.  The tails are sorted by length before the launch, so the
        eight tails of a wave are of similar length (a wave runs to its longest), and the
        results un-permuted.  One handle per batch size is kept until close()."""
        index = np.asarray(index, dtype=np.int64).reshape(-1)
        W = len(index)
        if len(end_idxs) != W:
            raise ValueError(f'warm_starts: {W} thresholds for {len(end_idxs)} end points')
        out = [None] * W
        if self.empty or W == 0:
            return out
        if W and (index.min() < 0 or index.max() >= len(self.thresholds)):
            raise IndexError(f'warm_starts: threshold index outside [0, {len(self.thresholds)})')
        ends = np.array([self.end_idx if e is None or e > self.end_idx else int(e) for e in end_idxs], dtype=np.int64)
        valid = np.nonzero(ends > self.start_off)[0] if self.cold else np.arange(W)
        if len(valid) == 0:
            return out
        n = 1 + np.maximum(ends[valid] - self.start_off, 0)  # array entries of each prefix
        row = n // self.every - 1 if self.every > 0 else np.full(len(valid), -1, np.int64)
        lo = np.where(row >= 0, (row + 1) * self.every, 0)
        order = np.argsort(n - lo, kind='stable')
        sel = valid[order]
        B = len(sel)
        kf = self._kft.get(B)
        if kf is None:
            kf = self._kft[B] = BatchedKF('ref15', B, self.dtype, device=self.dev.index or 0,
                                          params=_params(self.consts))
        if (row < 0).any():
            kf.set_state(self._x0.expand(15, B).contiguous(), self._P0.expand(27, B).contiguous())
        kf.run_tails(self._et, self._dt, self._pay, lo[order], n[order], torch.from_numpy(self.thresholds[index[sel]]),
                     src_x=self._cx if self.every > 0 else None, src_P=self._cP if self.every > 0 else None,
                     src_row=row[order], src_col=index[sel])
        x, Pb = kf.state()
        host = torch.cat([x[:6], Pb]).double().cpu().numpy()  # [6 + 27, B]
        xs = host[:6].T.tolist()
        Ps = from_blocks(np.ascontiguousarray(host[6:].T))
        prev = self._prev[n[order] - 1].tolist()
        for j, w in enumerate(sel.tolist()):
            out[w] = ((prev[j], *xs[j]), Ps[j], prev[j])
        return out


def _smooth_memory_check(dev, entries, B, rows):
    """KFError(KF_ENOMEM) before anything runs if ``rows`` float64 rows per entry and filter do not
    fit the device's free memory (the smoothed sweeps' records)."""
    need = entries * rows * B * 8
    free = torch.cuda.mem_get_info(dev)[0]
    if need > free:
        raise _lib.KFError(_lib.KF_ENOMEM, f'smooth: the filtered and smoothed records of {entries} entries x '
                                           f'{B} filters need {need} B, the device has {free} B free')


def _scores_dict(table):
    """run_sweep_scores' [8, B] table as the sweeps' ``scores``: the counts, sums and innovation
    negative log-likelihoods per sensor, pos_n and pos_rmse = sqrt(pos_sse / pos_n)."""
    d = {k: table[r].copy() for k, r in SCORE_ROWS.items() if k != 'pos_sse'}
    for sensor in ('gps', 'imu'):
        d[f'{sensor}_nll'] = innovation_nll(table, 'ref15', sensor)
    n = table[SCORE_ROWS['pos_n']]
    d['pos_rmse'] = np.sqrt(np.where(n > 0, table[SCORE_ROWS['pos_sse']], np.nan) / np.where(n > 0, n, 1.0))
    return d


def run_smoothed_kalman_filter(events, start_idx=None, end_idx=None, R_threshold=None, consts=None, initial_pt=None,
                               initial_state=None, device=0):
    """run_adaptive_threshold_kalman_filter (R_threshold None: the ungated filter) followed by the
    fixed-interval smoother over its run, f64: an AdaptiveSweep(smooth=True) of the one threshold.
    Returns result(0) + smoothed(0): (states, logdets, P, previous_time, measurement_times,
    smoothed_states, smoothed_logdets), or None where the driver returns None.  The reference has
    no smoother; the smoothed states are the estimate of every entry given the whole window."""
    thr = -float('inf') if R_threshold is None else float(R_threshold)
    sw = AdaptiveSweep(events, [thr], start_idx, end_idx, initial_pt, initial_state, 'f64', device, consts, smooth=True)
    try:
        r = sw.result(0)
        return None if r is None else r + sw.smoothed(0)
    finally:
        sw.close()


def run_adaptive_threshold_sweep(events, thresholds, **kw):
    """The AdaptiveSweep of ``events`` under ``thresholds`` (its keyword arguments)."""
    return AdaptiveSweep(events, thresholds, **kw)


class ParameterSweep(AdaptiveSweep):
    """run_adaptive_threshold_kalman_filter over ONE window under every constant set of
    ``consts_list`` (ModelConsts('ref15', ...): the getters a caller of the reference replaces
    through class_args, kf_workers.py:1242-1251) at once: one kf_run_sweep_params launch, filter i
    under consts_list[i] and thresholds[i] (None: no gate, every event updates), instead of one
    handle and one run per set.  The window, the drivers' rules and the arrays are
    AdaptiveSweep's.  A cold start takes each set's own P0 (a column of the start state); a warm
    start (initial_pt, initial_state) is shared by every filter.

    ``result(i)``: the 5-tuple run_adaptive_threshold_kalman_filter(..., R_threshold=thresholds[i],
    consts=consts_list[i]) returns.  ``warm_start(i, end_idx)``: its prefix's (states[-1], P,
    previous_time), the tail past the checkpoint run as a one-filter parameter sweep with set i's
    column, so it rounds as the sweep did.  ``warm_starts`` is the list of those (kf_run_tails
    has no per-filter constants: one launch per tail).

    ``scores=True`` makes the one launch kf_run_sweep_scores (AdaptiveSweep takes it too, with its
    one constant set in every column), so the grid is ranked without records (``records=False``
    loses nothing of the ranking): ``.scores`` is a dict of NumPy [B] arrays gps_n, gps_nis,
    gps_logdet_s, gps_nll, the same four for imu, pos_n and pos_rmse, the position error against
    ``track`` (anything _track_of takes; None: the stream's own fixes) interpolated at the entries'
    times with track_positions as calculate_accuracy_metrics does (kf_workers.py:1162-1216); the
    leading NONE entry is scored (it is states[0]), a skipped dt < 0 entry is not.  ``.best(by)``:
    the index of the smallest finite scores[by]."""

    def __init__(self, events, consts_list, thresholds=None, start_idx=None, end_idx=None, initial_pt=None,
                 initial_state=None, dtype='f64', device=0, records=True, checkpoint_every=4096, track=None,
                 scores=False, smooth=False, em=False, _run=True):
        self._sets = list(consts_list)
        if thresholds is None:
            thresholds = np.full(len(self._sets), -np.inf)
        if len(np.reshape(thresholds, -1)) != len(self._sets):
            raise _lib.KFError(_lib.KF_EINVAL, f'ParameterSweep: {len(np.reshape(thresholds, -1))} thresholds for '
                                               f'{len(self._sets)} constant sets')
        for c in self._sets:
            if not isinstance(c, ModelConsts) or c.model != 'ref15':
                raise ValueError('ParameterSweep: consts_list holds ModelConsts(\'ref15\', ...)')
        super().__init__(events, thresholds, start_idx, end_idx, initial_pt, initial_state, dtype, device, None,
                         records, checkpoint_every, scores, track, smooth=smooth, em=em, _run=_run)
        self.consts_list = self._sets

    def warm_starts(self, index, end_idxs):
        if len(index) != len(end_idxs):
            raise ValueError(f'warm_starts: {len(index)} constant sets for {len(end_idxs)} end points')
        return [self.warm_start(int(i), e) for i, e in zip(index, end_idxs)]


def fit_noise(events, consts_list=None, thresholds=None, iters=10, imu_rows='measured', **window):
    """EM for the diagonals of Q, R_imu and R_gps of the 15-state model over ONE log: the B starting
    sets of ``consts_list`` (ModelConsts('ref15', ...); None: the reference's alone) each run their
    own EM, filter i gated by thresholds[i] (None: no gate).  ``window``: ParameterSweep's start_idx,
    end_idx, initial_pt, initial_state, device.  Every iteration is one scored forward sweep
    (kf_run_sweep_scores with ckpt_every = 1 and ``updated``), one kf_smooth_sweep_em in place over
    its record, and engine.ref_em_update(imu_rows=...); the tables stay on the device.  The start
    state and each set's P0 are kept (x0 / P0 are not estimated).

    Returns engine.NoiseFit(consts, history, nll, status): the B fitted ModelConsts, history
    [iters + 1, 33, B] (the table every iteration started from, then the result), nll [iters + 1,
    B] (the GPS + IMU innovation negative log-likelihood of every forward sweep, so before each
    update, plus one more sweep that scores the last table) and status [B] (the last backward
    pass'; a filter that failed keeps NaN constants from there on).

    Unlike the constant-velocity loop (BatchedKF.fit_noise) this is not textbook EM on fixed data:
    the IMU pseudo-measurement's position and velocity rows are built from the predicted state, so
    the "data" move with the constants, and under a finite threshold the gate decides which updates
    exist at all, so the likelihood's terms change from one iteration to the next.  The NLL need
    not fall monotonically under a finite threshold or with imu_rows='all'; read ``nll`` before
    trusting a fit."""
    from .engine import NoiseFit, innovation_nll, ref_em_update
    sets = [ModelConsts('ref15')] if consts_list is None else list(consts_list)
    if iters < 0:
        raise ValueError(f'fit_noise: iters = {iters} < 0')
    for k in ('dtype', 'records', 'scores', 'smooth', 'em', 'checkpoint_every', 'track'):
        if k in window:
            raise ValueError(f'fit_noise: {k} is not a window argument (start_idx, end_idx, initial_pt, '
                             f'initial_state, device)')
    sw = ParameterSweep(events, sets, thresholds, dtype='f64', records=False, _run=False, **window)
    B = len(sets)
    tab = torch.from_numpy(consts_table('ref15', sets))
    if sw.empty:  # a cold window without a fix: nothing to fit
        return NoiseFit(sets, tab.numpy()[None], np.zeros((1, B)), np.zeros(B, np.int32))
    dev = sw.dev
    T = int(sw._et.shape[0])
    _smooth_memory_check(dev, T, B, 15 + 27)
    tab = tab.to(dev)
    thr = torch.from_numpy(sw.thresholds)
    x0, P0 = sw._x0.expand(15, B).contiguous(), sw._P0.expand(27, B).contiguous()
    history, nll = [tab], []
    status = torch.zeros(B, dtype=torch.int32, device=dev)

    def forward(kf, tab, record):
        kf.set_state(x0, P0)
        r = kf.run_sweep_scores(sw._et, sw._dt, sw._pay, tab, thr, updated=record, checkpoint_every=1 if record else 0)
        nll.append(innovation_nll(r.scores, 'ref15', 'gps') + innovation_nll(r.scores, 'ref15', 'imu'))
        return r

    with BatchedKF('ref15', B, 'f64', device=dev.index or 0) as kf:
        for _ in range(iters):
            r = forward(kf, tab, True)
            sm = kf.smooth_sweep_em(sw._et, sw._dt, sw._pay, r.updated, r.ckpt_x, r.ckpt_P, consts=tab, x=True, P=True,
                                    inplace=True)
            status = sm.status
            tab = ref_em_update(sm.em, tab, 'ref15', imu_rows)
            history.append(tab)
            del r, sm
        forward(kf, tab, False)
    hist = torch.stack(history).cpu().numpy()
    fitted = [ModelConsts('ref15', q=hist[-1, :15, f], r_imu=hist[-1, 15:30, f], r_gps=hist[-1, 30:, f], p0=c.p0)
              for f, c in enumerate(sets)]
    return NoiseFit(fitted, hist, torch.stack(nll).cpu().numpy(), status.cpu().numpy())


def run_parameter_sweep(events, consts_list, thresholds=None, **kw):
    """The ParameterSweep of ``events`` under ``consts_list`` (its keyword arguments)."""
    return ParameterSweep(events, consts_list, thresholds, **kw)


def run_kalman_filter(events, start_idx, end_idx, dtype='f64', device=0, consts=None):
    """kf_workers.py:738-824 on the GPU: x0 = 0, the reference's P0, the window's events from
    its first GPS fix on (that fix at dt = 0), no dt < 0 guard.  Returns (states,
    covariances) — states[0] = (0, 0, 0, 0, 0, 0, 0) and one 15x15 covariance per record, the
    per-step covariances coming from kf_run_events' cov stream."""
    stream, times = [], []
    prev = None
    for (_, stype, t, sdata) in events[start_idx:end_idx]:
        if stype == 'GPS' and prev is None:
            prev = t
        if prev is None:
            continue
        stream.append((GPS if stype == 'GPS' else IMU, t - prev, event_payload(stype, sdata)))
        times.append(t)
        prev = t
    tr, _, _, _, _, _, cv = _run_streams([stream], np.zeros((1, 15)), to_blocks(_p0(consts))[None], dtype, device,
                                         cov=True, consts=consts)
    states = [(0, *tr[0, :, 0])] + [(t, *tr[i + 1, :, 0]) for i, t in enumerate(times)]
    covs = list(from_blocks(cv[:len(times) + 1, :, 0]))
    return states, covs


def run_no_update_kalman_filter(events, start_idx=None, end_idx=None, R_threshold=None, initial_pt=None,
                                initial_state=None, print_output=False, dtype='f64', device=0, consts=None):
    """kf_workers.py:1060-1160 on the GPU: the window as KF_EVENT_PREDICT events (every update
    of the reference's loop is commented out), logdet after each.  A dt < 0 event is skipped
    without advancing the previous time (:1113-1116).  Returns (states, logdets, P,
    previous_time, measurement_times), or None when no GPS fix starts a cold window.  Over an
    ingested stream the window never leaves the device (run_monotone_stream)."""
    ds = _device_stream(events)
    if ds is not None:
        r = run_monotone_stream(ds, start_idx, end_idx, initial_pt, initial_state, dtype, consts, predict_only=True)
        if r is None:
            return None
        t, traj, ld, P, prev, mtimes = r
        if print_output:
            print(f'No-update Kalman Filter (GPU): {len(t) - 1} predictions')
        return _stream_states(t, traj), ld.tolist(), P, prev, mtimes
    start_idx, end_idx = _window(events, start_idx, end_idx)
    x0 = np.zeros(15)
    mtimes = []
    if initial_pt is not None and initial_state is not None:
        P = np.asarray(initial_pt, np.float64)
        x0[0:6] = initial_state[1:7]
        prev = initial_state[0]
        start_off = start_idx
    else:
        P = _p0(consts)
        cs = _cold_start(events, start_idx, end_idx)
        if cs is None:
            return None
        x0, prev, start_off = cs
        mtimes.append(prev)
    t_first = prev
    stream, times, _, prev = _driver_stream(events[start_off:end_idx], prev, _lib.KF_DT_MONOTONE, predict_only=True)
    tr, ld, _, _, Pb, _ = _run_streams([stream], x0[None], to_blocks(P)[None], dtype, device, consts=consts)
    states = [(t_first, *tr[0, :, 0])] + [(t, *tr[i + 1, :, 0]) for i, t in enumerate(times)]
    logdets = [float(v) for v in ld[:len(times) + 1, 0]]
    if print_output:
        print(f'No-update Kalman Filter (GPU): {len(times)} predictions from index {start_off} to {end_idx}')
    return states, logdets, from_blocks(Pb[:, 0]), prev, mtimes


def _combo_stream(combo, prev_time, target_end):
    """Event stream of one combination with the worker's rules (kf_workers.py:36-82)."""
    s, times = [], []
    cur = prev_time
    for (_, stype, t, sdata) in combo:
        dt = t - cur
        if dt < 0:
            continue
        s.append((GPS if stype == 'GPS' else IMU, dt, event_payload(stype, sdata)))
        times.append(t)
        cur = t
    if cur < target_end - 1e-8:
        s.append((PREDICT, target_end - cur, [0.0] * 9))
        times.append(target_end)
    return s, times


def evaluate_combo_chunk(chunk, xt, Pt, prev_time, target_end_time, dtype='f64', device=0, consts=None, kf=None):
    """evaluate_combo_chunk_worker (kf_workers.py:22-97) for a whole chunk in ONE launch, one
    filter per combination.  Returns [(0, traj, combo, x_final, None, log_det, k), ...].  kf: a
    'ref15' handle of len(chunk) filters with these constants to run on (_run_streams)."""
    if not chunk:
        return []
    built = [_combo_stream(c, prev_time, target_end_time) for c in chunk]
    B = len(chunk)
    tr, ld, _, x, Pb, st = _run_streams([b[0] for b in built], np.broadcast_to(np.asarray(xt, np.float64), (B, 15)),
                                        np.broadcast_to(to_blocks(Pt), (B, 27)), dtype, device, consts=consts, kf=kf)
    results = []
    for f, (combo, (s, times)) in enumerate(zip(chunk, built)):
        if st[f] != 0:  # the worker skips a combination that raised (kf_workers.py:88-91)
            continue
        n = len(times)
        traj = [(prev_time, *tr[0, :, f])] + [(t, *tr[i + 1, :, f]) for i, t in enumerate(times)]
        results.append((0, traj, combo, x[:, f].copy(), None, [float(v) for v in ld[:n + 1, f]], len(combo)))
    return results


def unrank_combination(n, k, r):
    """The r-th k-subset of range(n) in itertools.combinations order."""
    out, a = [], 0
    for j in range(k):
        while True:
            c = math.comb(n - a - 1, k - j - 1)
            if r < c:
                break
            r -= c
            a += 1
        out.append(a)
        a += 1
    return out


def brute_force_setup(events, start_idx=0, end_idx=None, initial_pt=None, initial_state=None, consts=None):
    """The search's inputs as kf_workers.py:1262-1310 sets them up: (candidates, x0, P0,
    prev_time, target_end, events [n, 11], init [42]), or None when there is no candidate: a
    cold window without a starting fix (:1303-1305), or an empty warm-start window, where the
    reference's size loop (:1325) never runs and it returns None (:1391-1392)."""
    if start_idx is None or start_idx < 0:
        start_idx = 0
    if end_idx is None or end_idx > len(events):
        end_idx = len(events)
    xt = np.zeros(15)
    if initial_pt is not None and initial_state is not None:
        Pt = np.asarray(initial_pt, np.float64)
        xt[0:6] = initial_state[1:7]
        prev_time = initial_state[0]
        cand = list(events[start_idx:end_idx])
    else:
        Pt = _p0(consts)
        cand, prev_time, started = [], None, False
        for (idx, stype, t, sdata) in events[start_idx:end_idx + 1]:  # the reference's +1 slice
            if not started and stype == 'GPS':
                xt[0], xt[1], xt[2] = sdata['easting'], sdata['northing'], sdata['altitude']
                started, prev_time = True, t
            if started:
                cand.append((idx, stype, t, sdata))
    if not cand:
        return None
    target_end = events[end_idx - 1][2]
    n = len(cand)
    if n > 64:
        raise ValueError(f'{n} candidate events: the GPU search supports at most 64 (2^64 subsets)')
    ev = np.zeros((n, 11))
    for i, (_, stype, t, sdata) in enumerate(cand):
        ev[i, 0] = t
        ev[i, 1] = GPS if stype == 'GPS' else IMU
        ev[i, 2:] = event_payload(stype, sdata)
    return cand, xt, Pt, prev_time, target_end, ev, np.concatenate([xt, to_blocks(Pt)])


def first_valid_rank(kf, ev, init, prev_time, target_end, k, lo, hi, threshold):
    """Smallest combination rank r in [lo, hi) of the k-subsets whose max log-determinant is
    below threshold (the reference's acceptance test, kf_workers.py:1353), or None; kf_eval_combos
    launches of kf.batch lanes."""
    width = kf.batch
    for off in range(lo, hi, width):
        cnt = min(width, hi - off)
        mx, _, _ = kf.eval_combos(ev, init, prev_time, target_end, k, combo_offset=off, logdets=False)
        ok = mx[:cnt] < threshold
        if bool(ok.any()):
            return off + int(torch.argmax(ok.to(torch.int8)).item())
    return None


def brute_force_result(cand, k, r, xt, Pt, prev_time, target_end, dtype='f64', device=0, indices=None, consts=None,
                       kf=None):
    """The reference's result dict (kf_workers.py:1358-1367) for combination rank r of size k
    (or the candidate ``indices`` of the subset); kf: a one-filter handle to run it on (the
    search's)."""
    idx = unrank_combination(len(cand), k, r) if indices is None else indices
    combo = tuple(cand[i] for i in idx)
    metric, traj, combo, x_bf, P_bf, log_det, used = evaluate_combo_chunk([combo], xt, Pt, prev_time, target_end,
                                                                          dtype, device, consts, kf=kf)[0]
    return {'selected_sensors': combo, 'final_state': x_bf, 'final_covariance': P_bf, 'trajectory': traj,
            'accuracy_metric': metric, 'log_determinants': log_det, 'num_measurements_used': used}


def search_level_bytes(nodes, dtype, sym=False):
    """Device bytes of one kf_search_combos level buffer (node blocks of 64, kf_internal.h; an
    axis-symmetric search's nodes hold 10 rows instead of 28, KF_OPT_AXIS_SYM; then the running
    max's exponent, the time and the mask: 20 B)."""
    w = 8 if dtype == 'f64' else 4
    return (nodes + 63) // 64 * 64 * ((10 if sym else 28) * w + 20)


SEARCH_HEAD_STEPS = 400000  # kf_capi.cpp kSearchHeadSteps
SEARCH_END_STEPS = 200000   # kf_capi.cpp kSearchEndSteps


def search_head_size(n, k_max=None):
    """The sizes 1 .. K kf_search_combos runs in its one-launch head (kf_capi.cpp: the largest K
    <= n - 2, below k_max, whose subsets' event steps from the root sum_k k C(n, k) stay within
    kSearchHeadSteps; 0 = no head, for n < 5 or K < 2).  Bookkeeping for the bench's bytes."""
    k_max = n if k_max is None else k_max
    if n < 5:
        return 0
    K, steps = 0, 0
    for k in range(1, min(n - 2, k_max - 1) + 1):
        steps += k * math.comb(n, k)
        if steps > SEARCH_HEAD_STEPS:
            break
        K = k
    return K if K >= 2 else 0


def search_end_size(n, k_max=None, head=True):
    """The first size k_end0 of kf_search_combos' end launch (kf_capi.cpp: sizes k_end0 .. k_max
    in one launch from level k_end0 - 1's stored nodes), k_max + 1 for none: the smallest k0 with
    sum_{k >= k0} (k - k0 + 1) C(n, k) within kSearchEndSteps, 2 <= k0 <= min(k_max - 1, n - 2),
    above the head's sizes, n - k0 + 1 <= 6.  Bookkeeping for the bench's bytes."""
    k_max = n if k_max is None else k_max
    K = search_head_size(n, k_max) if head else 0
    k_first = K + 1 if K else 1
    end = k_max + 1
    k0 = min(k_max - 1, n - 2)
    while k0 >= 2 and k0 > k_first and n - k0 + 1 <= 6:
        if sum((k - k0 + 1) * math.comb(n, k) for k in range(k0, k_max + 1)) > SEARCH_END_STEPS:
            break
        end = k0
        k0 -= 1
    return end


SEARCH_CM_PARENTS = 200000  # kf_capi.cpp kSearchChildMajorParents: levels with more parents run parent-major
SEARCH_PAIR_PARENTS = 1 << 22  # kf_capi.cpp kSearchPairParents: KF_OPT_SEARCH_PAIR = 0 pairs levels with as many


def _pair_policy(pair):
    """(least parents of a parent-major pair, child-major pairs for the rest?) of a
    KF_OPT_SEARCH_PAIR value, or None for no pairs (kf_capi.cpp)."""
    pair = {'auto': 0, 'off': 1, 'all': 2, 'cm': 3, True: 0, False: 1}.get(pair, pair)
    if pair == 1:
        return None
    pm_min = {0: SEARCH_PAIR_PARENTS, 2: 0, 3: None}.get(pair, int(pair))
    return pm_min, pair == 3


def search_plan(n, k_max=None, sym=False, pair='auto'):
    """kf_search_combos' launches over n free candidates, exhaustive (kf_capi.cpp): the head
    (sizes 1 .. K, if any), then per level k with stored parents a level launch or — axis-
    symmetric, level k + 1 below the end launch's sizes (KF_OPT_SEARCH_PAIR = pair) — one pair
    launch for levels k and k + 1: parent-major ('pair') for a parent-major level (more than
    SEARCH_CM_PARENTS parents) of at least the policy's parent count (SEARCH_PAIR_PARENTS by
    default), child-major ('pair_cm') otherwise; then the end launch (if any).  Returns
    (launches [(kind, k)], stored levels: the levels whose nodes a launch writes and the next one
    reads, once each)."""
    k_max = n if k_max is None else k_max
    K = search_head_size(n, k_max)
    end = search_end_size(n, k_max)
    pol = _pair_policy(pair) if sym else None
    launches, stored = [], []
    if K:
        launches.append(('head', K))
        stored.append(K)
    k = K + 1 if K else 1
    while k <= k_max:
        if k == end:
            launches.append(('end', k))
            break
        par = 1 if k == 1 else math.comb(n - 2, k - 1)
        if par and pol is not None and k >= 2 and k + 1 <= k_max and k + 1 < end:
            pm_pair = par > SEARCH_CM_PARENTS and pol[0] is not None and par >= pol[0]
            if pm_pair or pol[1]:
                launches.append(('pair' if pm_pair else 'pair_cm', k))
                if k + 1 < k_max:
                    stored.append(k + 1)
                k += 2
                continue
        if par:
            launches.append(('level', k))
            if k < k_max:
                stored.append(k)
        k += 1
    return launches, stored


def search_launches(n, k_max=None, sym=False, pair='auto'):
    """Kernel launches of one kf_search_combos over n free candidates (search_plan)."""
    return len(search_plan(n, k_max, sym, pair)[0])


def search_stored_levels(n, k_max=None, sym=False, pair='auto'):
    """The levels whose nodes one kf_search_combos writes once and reads once as parents
    (search_plan): the head's last size, each level launch's below k_max, each pair launch's
    second level; the end launch stores none."""
    return search_plan(n, k_max, sym, pair)[1]


def search_levels(n, dtype='f64', mem_bytes=32 << 30, sym=False):
    """Largest k_max for which kf_search_combos' level buffers (two of the widest stored level:
    the C(n - 2, k) subsets of size k < k_max whose largest candidate is <= n - 3) fit in
    ``mem_bytes`` and every level stays below 2^28 stored parents (n = free candidates; sym:
    the axis-symmetric search's 10-row nodes, kf_search_plan says which the handle runs)."""
    k_max, widest = 0, 0
    for k in range(1, n + 1):
        if k > 1:
            par = math.comb(n - 2, k - 1)
            if par >= 1 << 28:
                break
            widest = max(widest, par)
        if 2 * search_level_bytes(widest, dtype, sym) + 4096 > mem_bytes:
            break
        k_max = k
    return k_max


def search_class_width(n, dtype='f64', mem_bytes=32 << 30, sym=False):
    """The fewest leading candidates w whose fixed intersections split the search of n
    candidates into 2^w classes that kf_search_combos runs whole: a class has n - w free
    candidates, and every size of it fits ``mem_bytes`` and the 2^28-parent cap
    (search_levels(n - w) = n - w).  n = 40, f64, 32 GiB: 8 axis-symmetric (the widest stored
    level C(30, 15) nodes, 2 x 15.5 GB), 10 with every chain."""
    for w in range(n):
        if search_levels(n - w, dtype, mem_bytes, sym) >= n - w:
            return w
    return max(n - 1, 0)


NO_SIZE = None


def bitrev64(v):
    return int(f'{v & ((1 << 64) - 1):064b}'[::-1], 2)


def class_order(w):
    """The classes of candidates 0 .. w - 1, fewest fixed members first (the classes that can hold
    the smallest sizes; a search that is not exhaustive skips the rest once they cannot win)."""
    return sorted(range(1 << w), key=lambda c: (bin(c).count('1'), c))


def prefix_classes(n, k_max, dtype='f64', mem_bytes=32 << 30, sym=False, limit=None):
    """Classes for the sizes up to ``k_max`` of a search whose levels do not fit one call, when
    the fixed-pattern classes that fit every size (search_class_width) would be too many (n = 64:
    2^32).  A class is a prefix P, its members fixed and its free candidates those after max(P):
    kf_search_combos(n_fixed = max(P) + 1, fixed_mask = P), the subsets P + S, S within
    max(P) + 1 .. n - 1.  From the whole search (P empty), a class whose free sizes up to
    k_max - |P| do not fit one call (search_levels) is split by its next member f into the
    classes P + {f}, f = max(P) + 1 .. n - 1, which hold every subset of the class but P itself
    (the last, P + {n - 1}, as the class of P with the one free candidate n - 1).  Returns
    ([(n_fixed, fixed_mask)], fewest fixed members first, and the largest |P| of a split class —
    that subset is in no class: its size must have been searched already), or None past
    ``limit`` classes.  n = 64, 32 GiB: 64 classes for sizes up to 8, 532 up to 9, 2623 up to 10."""
    import functools
    levels = functools.lru_cache(None)(lambda m: search_levels(m, dtype, mem_bytes, sym))
    out, split = [], [-1]

    def rec(a, mask, p):
        if limit is not None and len(out) > limit:
            return
        if a == n:  # P + {n - 1}: the class of P over the one free candidate n - 1
            out.append((n - 1, mask & ~(1 << (n - 1))))
            return
        if levels(n - a) >= min(k_max - p, n - a):
            out.append((a, mask))
            return
        split[0] = max(split[0], p)
        for f in range(a, n):
            rec(f + 1, mask | (1 << f), p + 1)
    rec(0, 0, 0)
    if limit is not None and len(out) > limit:
        return None
    out.sort(key=lambda x: (bin(x[1]).count('1'), x[0], x[1]))
    return out, split[0]


def search_bands(n, k_done, dtype='f64', mem_bytes=32 << 30, sym=False, max_classes=None):
    """The size bands of a search too large for one call whose sizes 1 .. k_done accepted
    nothing: yields (K, prefix classes of the sizes up to K) for K = k_done + 1, k_done + 2, ...
    while those are fewer than ``max_classes`` (the fixed-pattern classes that search every
    size, which then finish the search: 256 at n = 40) and every subset a split leaves out has a
    size already searched (<= k_done).  Each band searches its sizes again below K; a band holds
    ~(n - K) / K times the subsets of the one before, so the repeats cost a fraction of the last."""
    for K in range(k_done + 1, n + 1):
        got = prefix_classes(n, K, dtype, mem_bytes, sym, limit=max_classes)
        if got is None:
            return
        classes, split = got
        if (max_classes is not None and len(classes) >= max_classes) or split > k_done:
            return
        yield K, classes


SEARCH_FIRST_BYTES = 1 << 30  # the first one-call pass's level buffers (one_call_search)


def one_call_search(kf, ev, init, prev_time, target_end, threshold, k_search, dtype='f64', mem_bytes=32 << 30,
                    sym=False):
    """The sizes 1 .. k_search in one kf_search_combos call each pass, stopping at the first
    accepted size: first the sizes whose level buffers fit SEARCH_FIRST_BYTES, then, if none was
    accepted, all k_search (which searches the first ones again).  A handle's level buffers are
    sized by the call's k_max and freed with the handle, and at n = 40 the sizes up to 10 take
    2 x 16 GB that a box took up to ~0.7 s to map and free per window; the reference's windows
    accept within the first pass's sizes (7 at n = 40, 1 GiB).  Returns (k, indices) or (0, None)."""
    n = int(np.asarray(ev).shape[0])
    k_first = min(k_search, search_levels(n, dtype, min(mem_bytes, SEARCH_FIRST_BYTES), sym))
    k, idx = 0, None
    for k_max in sorted({k_first, k_search} - {0}):
        k, idx, _, _ = kf.search_combos(ev, init, prev_time, target_end, threshold, k_max=k_max)
        if k:
            break
    return k, idx


def search_past(search_class, n, k_done, w, dtype='f64', mem_bytes=32 << 30, sym=False):
    """The reference's pick (class_search's (k, key)) in a search of n candidates whose sizes
    1 .. k_done accepted nothing and whose levels do not fit one call: the next sizes by bands of
    prefix classes (search_bands) while those are fewer than the 2^w classes that fit every size
    (search_class_width; n = 40: 40 classes for size 11, 151 up to 12, then the 256), then every
    size by the latter.  ``search_class(n_fixed, fixed_mask, k_max)`` as class_search's."""
    for K, classes in search_bands(n, k_done, dtype, mem_bytes, sym, 1 << w):
        k, key = class_search(search_class, n, 0, classes, False, K)
        if k is not NO_SIZE:
            return k, key
    return class_search(search_class, n, w, class_order(w))


def class_search(search_class, n, w, classes, exhaustive=False, k_max=None):
    """Runs ``search_class(n_fixed, c, k_max) -> (k, indices or None)`` for each class in turn and
    keeps the reference's pick among them (kf_workers.py:1325-1356): the smallest accepted size
    and, at it, the first subset in itertools.combinations order, i.e. the largest bit-reversed
    mask.  A class is a bit pattern c (the subsets whose intersection with candidates 0 .. w - 1
    is c, n_fixed = w) or a pair (n_fixed, c) (prefix_classes).  Returns (k, key) or
    (NO_SIZE, 0).  Not exhaustive, a class searches only the sizes that can still win: up to
    the best size so far (skipped when its fixed members alone exceed it; one size above when
    they make exactly it, the least k_max kf_search_combos takes).  ``k_max`` caps the sizes
    searched (the reference's loop over sizes 1 .. n, :1325, cut short)."""
    k_r, key_r = NO_SIZE, 0
    cap = n if k_max is None else int(k_max)
    for item in classes:
        nf, c = item if isinstance(item, tuple) else (w, item)
        k_base = bin(c).count('1')
        lim = cap
        if not exhaustive and k_r is not NO_SIZE:
            lim = min(lim, k_r)
        if k_base > lim:
            continue
        k, idx = search_class(nf, c, min(n, max(lim, k_base + 1)))
        if k and idx is not None and k <= cap:
            key = bitrev64(sum(1 << i for i in idx))
            if k_r is NO_SIZE or k < k_r or (k == k_r and key > key_r):
                k_r, key_r = k, key
    return k_r, key_r


def search_combos_classed(kf, ev, init, prev_time, target_end, threshold, w, exhaustive=False, subset_max=False,
                          classes=None, k_max=None):
    """kf.search_combos over sizes 1 .. k_max (default n) of the n candidates as 2^w class
    searches run one after another on this handle's GPU (``class_search``; w from
    ``search_class_width`` when the whole search does not fit one call).  Returns
    search_combos' (k_found, winner indices or None, accepted count per size [n + 1],
    subset_max [2^n] or None): the same winner and counts as one call over those sizes of every
    subset (not exhaustive: counts past k_found are 0)."""
    n = int(np.asarray(ev).shape[0])
    acc = np.zeros(n + 1, dtype=np.uint64)
    sm = None
    if subset_max:
        sm = kf.empty(1 << n)
        sm.fill_(float('nan'))

    def search_class(nf, c, k_max):
        k, idx, a, _ = kf.search_combos(ev, init, prev_time, target_end, threshold, k_max=k_max,
                                        exhaustive=exhaustive, subset_max=sm if sm is not None else False,
                                        n_fixed=nf, fixed_mask=c)
        acc[:len(a)] += a
        return k, idx
    k, key = class_search(search_class, n, w, class_order(w) if classes is None else classes, exhaustive, k_max)
    if k_max is not None:
        acc[int(k_max) + 1:] = 0   # a class whose fixed members make k_max searched one size more
    if k is NO_SIZE:
        return 0, None, acc, sm
    if not exhaustive:
        acc[k + 1:] = 0
    mask = bitrev64(key)
    return k, tuple(i for i in range(n) if (mask >> i) & 1), acc, sm


def run_brute_force_kalman_filter_no_sampling_min_usage(events, start_idx=0, end_idx=None, R_threshold=None,
                                                       initial_pt=None, initial_state=None,
                                                       max_combos_in_memory=1 << 22, dtype='f64', device=0,
                                                       search_mem_bytes=32 << 30, consts=None):
    """kf_workers.py:1218-1392 on the GPU: for k = 1..n, evaluate every k-subset of the candidate
    events and return the first subset, in itertools.combinations order, whose max
    log-determinant is below R_threshold — the reference's result dict — or None.  The subsets
    run as the shared-prefix search (kf_search_combos: one event step per subset): the sizes
    whose level buffers fit ``search_mem_bytes`` in one call (k_search), then, if none of those
    was accepted, class searches one after another (search_past): bands of the next sizes by
    prefix classes while they are the fewer calls, then every size as the 2^w fixed-pattern
    classes (n = 40, the reference's visualizing window, kf_workers_visualizing.py:2293, 2340:
    size 11 in 40 prefix classes, sizes up to 12 in 151, then 256 classes of 32 free
    candidates; n = 64: sizes up to 8 in 64 classes, 9 in 532, 10 in 2623).  ``max_combos_in_memory`` is the reference's argument; the
    search needs no per-subset batch.  One filter per subset stays available as
    ``first_valid_rank`` (kf_eval_combos).  Multi-GPU: kfmi.dist.brute_force_search."""
    if R_threshold is None:
        raise ValueError('R_threshold must be specified for brute force KF.')
    st = brute_force_setup(events, start_idx, end_idx, initial_pt, initial_state, consts)
    if st is None:
        return None
    cand, xt, Pt, prev_time, target_end, ev, init = st
    n = len(cand)
    kf = BatchedKF('ref15', 1, dtype, device=device, params=_params(consts))
    try:
        sym = kf.search_plan(init, n, k_max=1)['sym']
        k_search = search_levels(n, dtype, search_mem_bytes, sym)
        k, idx = one_call_search(kf, ev, init, prev_time, target_end, R_threshold, k_search, dtype,
                                 search_mem_bytes, sym)
        if not k and k_search < n:
            def search_class(nf, c, k_max):
                kk, ii, _, _ = kf.search_combos(ev, init, prev_time, target_end, R_threshold, k_max=k_max,
                                                n_fixed=nf, fixed_mask=c)
                return kk, ii
            w = search_class_width(n, dtype, search_mem_bytes, sym)
            kr, key = search_past(search_class, n, k_search, w, dtype, search_mem_bytes, sym)
            if kr is not NO_SIZE:
                mask = bitrev64(key)
                k, idx = kr, tuple(i for i in range(n) if (mask >> i) & 1)
        if not k:
            return None
        return brute_force_result(cand, k, None, xt, Pt, prev_time, target_end, dtype, device, indices=idx,
                                  consts=consts, kf=kf)
    finally:
        kf.close()


# --------------------------------------------------------------------------------------------
# The per-window schedule search scored by RMSE (KF_SensorFusion.ipynb's
# run_brute_force_kalman_filter and calculate_accuracy_metrics)
# --------------------------------------------------------------------------------------------

# the notebook's cold-start covariance (KF_SensorFusion.ipynb: run_brute_force_kalman_filter's Pt)
SCHEDULE_P0 = np.diag([1000.0] * 3 + [100.0] * 9 + [1000.0] * 3)
SCHEDULE_MAX_NODES = 1 << 26  # kf_internal.h kScheduleMaxNodes: the widest stored level of one call


def schedule_queues(events, start_idx=0, end_idx=None, frequency=None):
    """The notebook's windowing of events[start_idx:end_idx] into sampling windows of 1/frequency
    seconds: start at the first fix; an event closer than 1/f to the previous trigger is queued;
    the first event past the window (the trigger) closes the queue and is itself dropped, unless
    the queue was empty, when it is queued alone; the trailing partial queue is discarded.
    ``events``: the reference's event list or a kf_workers.EventList.  Returns the list of
    queues, each a list of event tuples."""
    if frequency is None or not frequency > 0:
        raise ValueError('frequency must be > 0')
    if end_idx is None:
        end_idx = len(events)
    period = 1 / frequency
    queues, queue = [], []
    started, previous = False, None
    for ev in events[start_idx:end_idx]:
        _, stype, t, _ = ev
        if not started and stype == 'GPS':
            started, previous = True, t
        if not started:
            continue
        if t - previous < period:
            queue.append(ev)
            continue
        if not queue:
            queue.append(ev)
        queues.append(queue)
        queue = []
        previous = t
    return queues


def track_positions(track_t, track_p, tq):
    """Positions of the track (times [G] strictly increasing, positions [G, 3]) at the times tq,
    linearly interpolated, and extrapolated from the end segments, in fp64, with
    scipy.interpolate.interp1d(kind='linear', fill_value='extrapolate')'s own formula."""
    t = np.asarray(track_t, np.float64)
    p = np.asarray(track_p, np.float64)
    tq = np.atleast_1d(np.asarray(tq, np.float64))
    if t.ndim != 1 or t.size < 2 or p.shape != (t.size, 3):
        raise ValueError('the track needs times [G] and positions [G, 3] with G >= 2')
    if not np.all(np.diff(t) > 0):
        raise ValueError('the track\'s times must be strictly increasing')
    hi = np.clip(np.searchsorted(t, tq, side='left'), 1, t.size - 1)
    lo = hi - 1
    slope = (p[hi] - p[lo]) / (t[hi] - t[lo])[:, None]
    return slope * (tq - t[lo])[:, None] + p[lo]


def _track_of(events, track):
    """(times, positions) of a metric track: a (times, positions) pair, a utm_data list of fix
    dicts, or None for the event list's own fixes."""
    if track is None:
        h = getattr(events, 'h', None)
        if h is not None:  # an EventList: its stream's host arrays
            g = np.asarray(h['etype']) == GPS
            return np.asarray(h['t'], np.float64)[g], np.asarray(h['payload'], np.float64)[g][:, 0:3]
        track = [sd for _, stype, _, sd in events if stype == 'GPS']
    if isinstance(track, tuple) and len(track) == 2:
        return np.asarray(track[0], np.float64), np.asarray(track[1], np.float64)
    tt = np.array([sd['time'] for sd in track], np.float64)
    pp = np.array([[sd['easting'], sd['northing'], sd['altitude']] for sd in track], np.float64).reshape(len(tt), 3)
    return tt, pp


def schedule_arrays(queues, track_t, track_p):
    """The queues as kf_search_schedules' host arrays: (q_len [W] int32, events [C, 11],
    ref_pos [C, 3])."""
    flat = [ev for q in queues for ev in q]
    ev = np.zeros((len(flat), 11))
    for i, (_, stype, t, sdata) in enumerate(flat):
        ev[i, 0] = t
        ev[i, 1] = GPS if stype == 'GPS' else IMU
        ev[i, 2:] = event_payload(stype, sdata)
    ref = track_positions(track_t, track_p, ev[:, 0]) if len(flat) else np.zeros((0, 3))
    return np.array([len(q) for q in queues], np.int32), ev, ref


def search_schedules(events, start_idx=0, end_idx=None, frequency=None, initial_pt=None, initial_state=None,
                     track=None, consts=None, mem_bytes=32 << 30, max_schedules=1 << 36, metrics=False, device=0):
    """The notebook's run_brute_force_kalman_filter on the GPU: every schedule of one pick per
    sampling window (schedule_queues) as its own filter, scored by the position RMSE of its
    trajectory against ``track`` (track_positions; None = the event list's own fixes), the first
    schedule in itertools.product order with the strictly smallest score kept.  Without a warm
    start (initial_pt, initial_state = a driver's P and states[-1]) x0 = 0, P0 = SCHEDULE_P0 and
    the first pick's dt is 0, as in the notebook.  The search runs as kf_search_schedules, with
    the smallest number of fixed leading windows whose plan fits ``mem_bytes``, the classes one
    after another and (metric, global rank) reduced here; the winner is then run through
    kf_run_events for its trajectory.  Raises ValueError when the space exceeds ``max_schedules``
    (the notebook warns and never finishes).  Returns a dict: the notebook's selected_sensors,
    final_state, final_covariance, trajectory [(t, x, y, z, roll, pitch, yaw)], accuracy_metric
    (None x 4 and inf with no complete window or no finite metric), and rank, digits, n_valid,
    n_schedules, n_fixed, q_len, metrics (a device tensor of every metric in product order with
    ``metrics``, else None)."""
    queues = schedule_queues(events, start_idx, end_idx, frequency)
    out = {'selected_sensors': None, 'final_state': None, 'final_covariance': None, 'trajectory': None,
           'accuracy_metric': float('inf'), 'rank': None, 'digits': None, 'n_valid': 0, 'n_schedules': 0,
           'n_fixed': 0, 'q_len': [len(q) for q in queues], 'metrics': None}
    if not queues:
        return out
    log_n = sum(math.log10(len(q)) for q in queues)
    if log_n > math.log10(max_schedules):
        raise ValueError(f'the windows hold about 1e{log_n:.1f} schedules (log10 = {log_n:.2f}), more than '
                         f'max_schedules = {max_schedules}; shorten the slice or lower the frequency')
    q_len, ev, ref = schedule_arrays(queues, *_track_of(events, track))
    W = len(queues)
    n_total = math.prod(int(q) for q in q_len)
    x0 = np.zeros(15)
    if initial_pt is not None and initial_state is not None:
        P = np.asarray(initial_pt, np.float64)
        x0[0:6] = initial_state[1:7]
        prev = float(initial_state[0])
    else:
        P, prev = SCHEDULE_P0, float('nan')
    P0b = to_blocks(P)
    init = np.concatenate([x0, P0b])
    kf = BatchedKF('ref15', 1, 'f64', device=device, params=_params(consts))
    try:
        for n_fixed in range(W + 1):
            plan = kf.schedule_plan(q_len, n_fixed)
            if (plan['n_free'] is not None and plan['widest'] <= SCHEDULE_MAX_NODES
                    and plan['workspace_bytes'] <= mem_bytes):
                break
        else:
            raise ValueError(f'no split of the {W} windows fits mem_bytes = {mem_bytes}')
        n_free = plan['n_free']
        mt = torch.empty(n_total, dtype=torch.float64, device=kf.device) if metrics else None
        best = (float('inf'), None, None)
        n_valid = 0
        for c, fixed in enumerate(itertools.product(*(range(int(q)) for q in q_len[:n_fixed]))):
            sl = mt[c * n_free:(c + 1) * n_free] if mt is not None else False
            rank, digits, metric, nv, _ = kf.search_schedules(ev, q_len, ref, init, prev, fixed=fixed, metrics=sl)
            n_valid += nv
            if rank is not None and metric < best[0]:  # classes in rank order: a tie keeps the earlier
                best = (metric, c * n_free + rank, digits)
        out.update(n_valid=n_valid, n_schedules=n_total, n_fixed=n_fixed, metrics=mt)
        if best[1] is None:
            return out
        metric, rank, digits = best
        picks = [queues[w][d] for w, d in enumerate(digits)]
        stream, last = [], prev
        for _, stype, t, sdata in picks:
            stream.append((GPS if stype == 'GPS' else IMU, 0.0 if last != last else t - last,
                           event_payload(stype, sdata)))
            last = t
        tr, _, _, x, Pb, _ = _run_streams([stream], x0[None], P0b[None], 'f64', device, consts=consts, kf=kf)
    finally:
        kf.close()
    out.update(selected_sensors=tuple(picks), final_state=x[:, 0].copy(), final_covariance=from_blocks(Pb[:, 0]),
               trajectory=[(p[2], *tr[i + 1, :, 0]) for i, p in enumerate(picks)], accuracy_metric=metric,
               rank=rank, digits=digits)
    return out


# --------------------------------------------------------------------------------------------
# The experiment loop's windows as one batch (kf_workers.py:2320-2345)
# --------------------------------------------------------------------------------------------

def _window_rule(tt, ee, pp, valid, prev_times, rule):
    """window_arrays on gathered entries: tt / ee [L, B] and pp [L, B, 9] are the stream's times,
    types and payloads at the windows' entries, valid [L, B] marks the entries inside each
    window (a prefix of every column)."""
    prev0 = np.asarray(prev_times, np.float64)[None, :]
    before = np.concatenate([prev0, tt[:-1]], axis=0)  # the previous entry's time (prev_time for the first)
    if rule == _lib.KF_DT_MONOTONE:
        before = np.maximum.accumulate(before, axis=0)  # skipped events do not move the previous time
    elif rule != _lib.KF_DT_FULL:
        raise ValueError('rule must be KF_DT_FULL or KF_DT_MONOTONE')
    d = tt - before
    et = np.where(valid, np.where(d < 0, NONE, ee), NONE).astype(np.uint8)
    dt = np.where(valid, d, 0.0)
    pay = np.where(valid[:, :, None], pp, 0.0)
    return et, dt, np.ascontiguousarray(pay.transpose(0, 2, 1))


def _window_index(start_idxs, lengths):
    """(entry indices [L, B] clipped into their windows, valid [L, B]) of B windows, L the longest."""
    starts = np.asarray(start_idxs, np.int64).reshape(-1)
    lens = np.asarray(lengths, np.int64).reshape(-1)
    L = int(lens.max()) if lens.size else 0
    j = np.arange(L, dtype=np.int64)[:, None]
    valid = j < lens[None, :]
    return np.where(valid, starts[None, :] + j, starts[None, :]), valid


def window_arrays(t, etype, payload, start_idxs, lengths, prev_times, rule):
    """The [L][B] event arrays of B windows of one merged stream, one window per filter, as the
    per-window drivers build them: window w holds entries start_idxs[w] .. start_idxs[w] +
    lengths[w] - 1 of the stream (t [N] float64, etype [N] uint8, payload [N, 9]; host arrays)
    after a state at time prev_times[w], and L = max(lengths).  ``rule`` is kf_events_dt's:
    _lib.KF_DT_FULL (run_kalman_filter_full: dt against the previous entry's time, skipped or
    not) or _lib.KF_DT_MONOTONE (the adaptive and no-update drivers: against the latest time so
    far); an entry with dt < 0 becomes KF_EVENT_NONE and keeps its dt and payload, as
    kf_events_dt leaves them.  Entries past a window's length are KF_EVENT_NONE with zero dt and
    payload.  Returns (etype [L, B] uint8, dt [L, B] float64, payload [L, 9, B] float64)."""
    t = np.asarray(t, np.float64)
    idx, valid = _window_index(start_idxs, lengths)
    if valid.any() and (idx.min() < 0 or idx.max() >= len(t)):
        raise ValueError('a window reaches outside the stream')
    return _window_rule(t[idx], np.asarray(etype)[idx], np.asarray(payload, np.float64)[idx], valid, prev_times, rule)


class WindowBatch:
    """run_window_batch's results: a sequence over the windows whose entry w is built on access,
    a dict of what the experiment loop takes from its four calls on that window
    (kf_workers.py:2320-2345), in the single drivers' layouts:
      'full'        run_kalman_filter_full's (states, logdets, P, prev_time)
      'adaptive'    run_adaptive_threshold_kalman_filter's (states, logdets, P, previous_time,
                    measurement_times) at 'threshold'
      'no_update'   run_no_update_kalman_filter's 5-tuple
      'brute_force' run_brute_force_kalman_filter_no_sampling_min_usage's result dict or None
      'threshold'   the window's R_threshold (its ratio times the full filter's lowest log-det)
    ``k_found`` [W], ``winners`` (index tuples or None) and ``thresholds`` [W] are NumPy / lists
    for the whole batch; ``fallback`` lists the windows that went through the one-window search."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __len__(self):
        return len(self.thresholds)

    def _filter(self, col, t_all, keep, rule_prev):
        states = [(float(t_all[i]), *self._traj[i, :, col].tolist()) for i in np.nonzero(keep)[0]]
        return states, self._ld[keep, col].tolist(), from_blocks(self._Pb[:, col]), rule_prev

    def __getitem__(self, w):
        W = len(self)
        if isinstance(w, slice):
            return [self[i] for i in range(*w.indices(W))]
        if w < 0:
            w += W
        if not 0 <= w < W:
            raise IndexError(w)
        L = int(self._lens[w])
        prev0 = float(self._prev0[w])
        t_all = np.concatenate([[prev0], self._tt[:L, w]])
        # masks over all L_max + 1 record rows: the entries past this window's length are NONE
        kfull, km = self._keep_full[:, w].copy(), self._keep_mono[:, w].copy()
        kfull[0] = km[0] = True  # the leading NONE entry records the initial state
        full = self._filter(w, t_all, kfull, float(t_all[-1]) if L else prev0)
        tk = t_all[km[:L + 1]]
        prev_m = float(tk[-1]) if len(tk) > 1 else prev0
        upd = (self._up[:, W + w].astype(bool) & km)[:L + 1]
        upd[0] = False
        adaptive = self._filter(W + w, t_all, km, prev_m) + (t_all[upd].tolist(),)
        no_update = self._filter(2 * W + w, t_all, km, prev_m) + ([],)
        return {'full': full, 'adaptive': adaptive, 'no_update': no_update, 'brute_force': self._brute(w),
                'threshold': float(self.thresholds[w])}

    def _brute(self, w):
        if w in self._fallback_results:
            return self._fallback_results[w]
        idx = self.winners[w]
        if idx is None:
            return None
        f = self._win_col[w]
        if self._win_status[f] != 0:
            return None
        s = int(self._starts[w])
        combo = tuple(self._events[s + i] for i in idx)
        times = self._win_times[f]
        traj = [(float(self._prev0[w]), *self._win_traj[0, :, f].tolist())]
        traj += [(t, *self._win_traj[i + 1, :, f].tolist()) for i, t in enumerate(times)]
        return {'selected_sensors': combo, 'final_state': self._win_x[:, f].copy(), 'final_covariance': None,
                'trajectory': traj, 'accuracy_metric': 0,
                'log_determinants': [float(v) for v in self._win_ld[:len(times) + 1, f]],
                'num_measurements_used': len(combo)}


def run_window_batch(events, start_idxs, end_idxs, initial_pts, initial_states, ratios=None, thresholds=None, k_max=4,
                     dtype='f64', device=0, consts=None):
    """The experiment loop's window phase (kf_workers.py:2320-2345) for W windows at once: each
    window [start_idxs[w], end_idxs[w]) of ``events`` (an ingested stream, an event list over one,
    or a plain event list) from its warm start initial_pts[w] (15x15) / initial_states[w]
    (states[-1] of the warm-up: x[0:6] = state[1:7], the other nine states zero, previous time =
    state[0]; :643-646, :978-981).  In order:
      1. the W full filters (run_kalman_filter_full) in one kf_run_events_gates launch;
      2. each window's threshold: ratios[w] times its full filter's lowest log-det (:2325), or
         thresholds[w] as given;
      3. the W adaptive and W no-update filters in one launch on a handle of 2 W filters (gates
         thresholds[w], and -inf over KF_EVENT_PREDICT events);
      4. every window's search over the sizes 1 .. k_max in one kf_search_windows call;
      5. the winners' own filters (the subset's events, then the predict to the window's end) as
         one more ragged batch, for the result dict's log_determinants, final_state, trajectory;
      6. a window without an accepted subset up to k_max goes through
         run_brute_force_kalman_filter_no_sampling_min_usage, one window per call as before.
    Returns a WindowBatch."""
    if (ratios is None) == (thresholds is None):
        raise ValueError('give either ratios or thresholds')
    starts = np.asarray(start_idxs, np.int64).reshape(-1)
    ends = np.asarray(end_idxs, np.int64).reshape(-1)
    W = len(starts)
    ds = _device_stream(events)
    n_all = len(ds) if ds is not None else len(events)
    ends = np.minimum(ends, n_all)
    lens = ends - starts
    if W == 0 or len(ends) != W or len(initial_pts) != W or len(initial_states) != W:
        raise ValueError('start_idxs, end_idxs, initial_pts and initial_states must list the same W >= 1 windows')
    if lens.min() < 1 or starts.min() < 0:
        raise ValueError('every window needs at least one event inside the stream')
    if lens.max() > 64:
        raise ValueError(f'{int(lens.max())} candidate events: the GPU search supports at most 64')
    idx, valid = _window_index(starts, lens)
    L = idx.shape[0]
    if ds is not None:  # the stream's host copy (cached by the stream): the windows' entries by index
        h = ds.host()
        tt, ee, pp = h['t'][idx].astype(np.float64), h['etype'][idx], h['payload'][idx].astype(np.float64)
        device = ds.t.device.index or 0
    else:
        tt, ee, pp = np.zeros((L, W)), np.zeros((L, W), np.uint8), np.zeros((L, W, 9))
        for w in range(W):
            for j, (_, stype, t, sdata) in enumerate(events[int(starts[w]):int(ends[w])]):
                tt[j, w], ee[j, w], pp[j, w] = t, GPS if stype == 'GPS' else IMU, event_payload(stype, sdata)
    x0 = np.zeros((W, 15))
    x0[:, 0:6] = np.asarray([s[1:7] for s in initial_states], np.float64)
    prev0 = np.asarray([s[0] for s in initial_states], np.float64)
    P0b = np.stack([to_blocks(np.asarray(P, np.float64)) for P in initial_pts])
    et_f, dt_f, pay_f = _window_rule(tt, ee, pp, valid, prev0, _lib.KF_DT_FULL)
    et_m, dt_m, pay_m = _window_rule(tt, ee, pp, valid, prev0, _lib.KF_DT_MONOTONE)

    def lead(et, dt, pay):  # a NONE event first records the initial state and logdet
        return (np.concatenate([np.full((1,) + et.shape[1:], NONE, np.uint8), et]),
                np.concatenate([np.zeros((1,) + dt.shape[1:]), dt]),
                np.concatenate([np.zeros((1,) + pay.shape[1:]), pay]))
    # the records' columns: [0, W) full, [W, 2W) adaptive, [2W, 3W) no-update.  The full filters
    # run first, on a handle of W filters (the thresholds come from their log-dets); the adaptive
    # and no-update filters then share one launch on a handle of 2 W
    et_p = np.where(et_m != NONE, PREDICT, NONE).astype(np.uint8)
    et1, dt1, pay1 = lead(et_f, dt_f, pay_f)
    et2, dt2, pay2 = lead(np.concatenate([et_m, et_p], 1), np.concatenate([dt_m, dt_m], 1),
                          np.concatenate([pay_m, np.zeros_like(pay_m)], 2))
    npd = np.float64 if dtype == 'f64' else np.float32
    inf = float('inf')
    kf1 = BatchedKF('ref15', W, dtype, device=device, params=_params(consts))
    kf = BatchedKF('ref15', 2 * W, dtype, device=device, params=_params(consts))
    try:
        xs, Ps = np.ascontiguousarray(x0.T.astype(npd)), np.ascontiguousarray(P0b.T.astype(npd))
        kf1.set_state(xs, Ps)
        tr1, ld1, up1, _ = kf1.run_events_gates(et1, dt1, pay1.astype(npd), np.full(W, -inf), updated=True)
        keep_full = et1 != NONE
        if thresholds is None:
            rec = keep_full.copy()
            rec[0] = True  # logdets[0], the initial covariance's, is in the driver's list too
            low = np.where(rec, ld1.double().cpu().numpy(), np.inf).min(axis=0)
            thr = np.asarray(ratios, np.float64).reshape(-1) * low
        else:
            thr = np.asarray(thresholds, np.float64).reshape(-1).copy()
        if thr.shape != (W,):
            raise ValueError('ratios / thresholds must hold one value per window')
        kf.set_state(np.tile(xs, (1, 2)), np.tile(Ps, (1, 2)))
        tr2, ld2, up2, _ = kf.run_events_gates(et2, dt2, pay2.astype(npd), np.concatenate([thr, np.full(W, -inf)]),
                                               updated=True)
        st = torch.cat([kf1.status(), kf.status()])
        traj = torch.cat([tr1, tr2], 2).double().cpu().numpy()
        ld = torch.cat([ld1, ld2], 1).double().cpu().numpy()
        up = torch.cat([up1, up2], 1).cpu().numpy()
        Pb_h = torch.cat([kf1.state()[1], kf.state()[1]], 1).double().cpu().numpy()
        # 4. the searches
        ev = np.zeros((W, L, 11))
        ev[:, :, 0] = tt.T
        ev[:, :, 1] = ee.T
        ev[:, :, 2:] = pp.transpose(1, 0, 2)
        init = np.concatenate([x0, P0b], 1)
        target_end = tt[lens - 1, np.arange(W)]
        k_found, masks, acc = kf.search_windows(ev, init, prev0, target_end, thr, int(k_max), n_events=lens)
    finally:
        kf1.close()
        kf.close()
    winners = [tuple(i for i in range(int(lens[w])) if (int(masks[w]) >> i) & 1) if k_found[w] else None
               for w in range(W)]
    # 5. the winners' own filters, one ragged batch (the combination worker's rules, kf_workers.py:36-82)
    cols, streams, times_l = {}, [], []
    for w in range(W):
        if winners[w] is None:
            continue
        s, times, cur = [], [], prev0[w]
        for i in winners[w]:
            d = tt[i, w] - cur
            if d < 0:
                continue
            s.append((int(ee[i, w]), d, pp[i, w]))
            times.append(float(tt[i, w]))
            cur = tt[i, w]
        if cur < target_end[w] - 1e-8:
            s.append((PREDICT, target_end[w] - cur, np.zeros(9)))
            times.append(float(target_end[w]))
        cols[w] = len(streams)
        streams.append(s)
        times_l.append(times)
    win = dict(_win_col=cols, _win_times=times_l, _win_traj=None, _win_ld=None, _win_x=None, _win_status=None)
    if streams:
        sel = np.asarray(list(cols))
        wtr, wld, _, wx, _, wst = _run_streams(streams, x0[sel], P0b[sel], dtype, device, consts=consts,
                                               thresholds=np.full(len(streams), -inf))
        win.update(_win_traj=wtr, _win_ld=wld, _win_x=wx, _win_status=wst)
    # 6. windows without an accepted subset up to k_max: the one-window search, as before
    fallback = {}
    for w in np.nonzero(np.asarray(k_found) == 0)[0]:
        fallback[int(w)] = run_brute_force_kalman_filter_no_sampling_min_usage(
            events, int(starts[w]), int(ends[w]), float(thr[w]), initial_pts[w], initial_states[w], dtype=dtype,
            device=device, consts=consts)
    return WindowBatch(thresholds=thr, k_found=np.asarray(k_found), winners=winners, n_accepted=acc,
                       fallback=sorted(fallback), status=st.cpu().numpy(), _fallback_results=fallback, _events=events,
                       _starts=starts, _lens=lens, _prev0=prev0, _tt=tt, _traj=traj, _ld=ld, _up=up, _Pb=Pb_h,
                       _keep_full=keep_full, _keep_mono=et2[:, :W] != NONE, **win)


# --------------------------------------------------------------------------------------------
# Sensor scheduling (kf_workers.py:99-213, 826-957)
# --------------------------------------------------------------------------------------------

def scheduler_gain(covariances, types=('GPS', 'IMU'), full=False, dtype='f64', device=0, consts=None):
    """Scheduler.gain (kf_workers.py:174-185) for a batch: covariances [B, 15, 15] (block-diagonal)
    -> [B, len(types)] traces of the posterior covariance after a candidate of each type
    (full=False: the reference's cov_matrix(S=[1]); full=True: every row of the sensor),
    computed in one kf_score_candidates launch."""
    Ps = np.asarray(covariances, np.float64)
    if Ps.ndim == 2:
        Ps = Ps[None]
    B = Ps.shape[0]
    kf = BatchedKF('ref15', B, dtype, device=device, params=_params(consts))
    npd = np.float64 if dtype == 'f64' else np.float32
    kf.set_state(np.zeros((15, B), npd), np.ascontiguousarray(to_blocks(Ps).T.astype(npd)))
    g = kf.score_candidates([GPS if s == 'GPS' else IMU for s in types], full=full)
    out = g.double().cpu().numpy().T
    kf.close()
    return out


def _host_stream(events):
    """The host arrays behind an event list that views an ingested stream (kfmi.kf_workers
    .EventList over kf_ingest's output), or None for a plain list of tuples."""
    h = getattr(events, 'h', None)
    return h if isinstance(h, dict) and {'t', 'etype', 'payload'} <= set(h) else None


def _scheduled_window_events(events, start_idx, end_idx, initial_pt, initial_state, consts=None):
    """Start state and candidate events exactly as run_kalman_filter_scheduled sets them up
    (kf_workers.py:828-877).  Returns (x0, P, prev_time, candidates) or None; candidates is the
    list of event tuples, or for an event list over an ingested stream the (lo, hi) index range
    of the candidates in its arrays (no per-event Python)."""
    if start_idx is None or start_idx < 0:
        start_idx = 0
    if end_idx is None or end_idx > len(events):
        end_idx = len(events)
    x0 = np.zeros(15)
    h = _host_stream(events)
    if initial_state is not None:
        P = np.asarray(initial_pt, np.float64)
        x0[0:6] = initial_state[1:7]
        start_off, prev = start_idx, initial_state[0]
    elif h is not None:
        P = _p0(consts)
        fixes = np.nonzero(h['etype'][start_idx:end_idx] == GPS)[0]
        if not len(fixes):
            return None
        start_off = start_idx + int(fixes[0])
        x0[0:3] = h['payload'][start_off, 0:3]
        prev = float(h['t'][start_off])
    else:
        P = _p0(consts)
        cs = _cold_start(events, start_idx, end_idx)
        if cs is None:
            return None
        x0, prev, start_off = cs
    if end_idx == -1:
        end_idx = len(events)
    if h is not None:
        return x0, P, prev, (start_off + 1, max(start_off + 1, end_idx))
    return x0, P, prev, list(events[start_off + 1:end_idx])


def _stream_arrays(cands, B=1, events=None):
    """Candidate events as one filter's streams repeated over B columns: t [T, B], etype [T, B],
    payload [T, 9, B] (T >= 1: an empty window is one padding event).  cands: event tuples, or
    an index range into the ingested arrays of ``events`` (_scheduled_window_events)."""
    if isinstance(cands, tuple):
        h = _host_stream(events)
        lo, hi = cands
        T = hi - lo
        t = np.zeros((max(T, 1), B))
        et = np.full((max(T, 1), B), NONE, np.uint8)
        pay = np.zeros((max(T, 1), 9, B))
        t[:T] = h['t'][lo:hi, None]
        et[:T] = h['etype'][lo:hi, None]
        pay[:T] = h['payload'][lo:hi, :, None]
        return t, et, pay, T
    T = len(cands)
    t = np.zeros((max(T, 1), B))
    et = np.full((max(T, 1), B), NONE, np.uint8)
    pay = np.zeros((max(T, 1), 9, B))
    for i, (_, stype, ti, sdata) in enumerate(cands):
        t[i, :] = ti
        et[i, :] = GPS if stype == 'GPS' else IMU
        pay[i, :, :] = np.asarray(event_payload(stype, sdata))[:, None]
    return t, et, pay, T


def legacy_words(n):
    """The next n raw 32-bit outputs of NumPy's global legacy generator (np.random's
    MT19937), without advancing it: what kf_run_scheduled_random draws np.random.choice from."""
    rs = np.random.RandomState()
    rs.set_state(np.random.get_state())
    return rs.randint(0, 1 << 32, size=n, dtype=np.uint32)


def run_kalman_filter_scheduled(events, start_idx=None, end_idx=None, initial_pt=None, initial_state=None,
                                selection_method=None, processing_frequency=None, print_output=False,
                                dtype='f64', device=0, consts=None, parallel=True):
    """kf_workers.py:826-957 on the GPU.  'greedy': windowing, Scheduler scoring and the filter
    all run in kf_run_scheduled; 'random': the same in kf_run_scheduled_random, each pick
    np.random.choice over the queue drawn on the device from the global NumPy generator's outputs
    in the reference's order (the generator advances by the outputs drawn).  Returns (states,
    logdets, P).  parallel=False: the random arm's picked events run as the single filter even
    where kf_run_events would take the time-parallel route (a long log; tests)."""
    if selection_method not in ('random', 'greedy'):
        print("Invalid selection_method. Choose either 'random' or 'greedy'.")
        return None
    w = _scheduled_window_events(events, start_idx, end_idx, initial_pt, initial_state, consts)
    if w is None:
        return None, None
    x0, P, prev0, cands = w
    f = float(processing_frequency)
    if selection_method == 'greedy':
        kf = BatchedKF('ref15', 1, dtype, device=device, params=_params(consts))
        npd = np.float64 if dtype == 'f64' else np.float32
        kf.set_state(x0[:, None].astype(npd), to_blocks(P)[:, None].astype(npd))
        t, et, pay, _ = _stream_arrays(cands, events=events)
        tr, ld, stt, ns = kf.run_scheduled(t, et, pay.astype(npd), np.array([prev0]), f)
        # the handle's initial logdet comes from a zero-event pass of the same kernels
        ld0 = _run_streams([[]], x0[None], to_blocks(P)[None], dtype, device, consts=consts)[1][0, 0]
        n = int(ns[0])
        tr, ld, stt = tr.double().cpu().numpy(), ld.double().cpu().numpy(), stt.cpu().numpy()
        xf, Pb = kf.state()
        Pf = from_blocks(Pb[:, 0].double().cpu().numpy())
        kf.close()
        states = [(prev0, *x0[:6])] + [(stt[i, 0], *tr[i, :, 0]) for i in range(n)]
        logdets = [float(ld0)] + [float(v) for v in ld[:n, 0]]
    else:
        # random_schedule (kf_workers.py:188-193): each window's np.random.choice is drawn on the
        # device from the global generator's next outputs, in the reference's order (the windows
        # follow the picks); the global generator then advances by the outputs the run took
        # the picks (windows + draws, kf_sched_random_picks: no filter state needed), then the
        # picked events through the event engine, which runs one long filter parallel over time
        kf = BatchedKF('ref15', 1, dtype, device=device, params=_params(consts))
        npd = np.float64 if dtype == 'f64' else np.float32
        t, et, pay, n_cand = _stream_arrays(cands, events=events)
        dev = kf.device
        td, etd = torch.as_tensor(t, device=dev), torch.as_tensor(et, device=dev)
        n_words = 2 * n_cand + 64
        while True:
            pick, stt, ns, used = kf.sched_random_picks(td, etd, np.array([prev0]), f,
                                                        legacy_words(n_words)[:, None])
            taken = int(used[0])
            if taken >= 0:
                break
            n_words *= 4  # the column ran out (rejections beyond 2 outputs per window): draw again
        np.random.randint(0, 1 << 32, size=taken, dtype=np.uint32)
        n = int(ns[0])
        sel = pick[:n, 0].long()
        st_d = stt[:n, 0]
        prev_d = torch.cat([torch.tensor([prev0], dtype=torch.float64, device=dev), st_d[:-1]])
        # a leading padding event: row 0 of the records holds the start state and its log-det
        ev_t = torch.cat([torch.tensor([NONE], dtype=torch.uint8, device=dev), etd[sel, 0]])
        ev_dt = torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), st_d - prev_d])
        paydev = torch.as_tensor(pay[:, :, 0].astype(npd), device=dev)
        ev_p = torch.cat([torch.zeros(1, 9, dtype=paydev.dtype, device=dev), paydev[sel]])
        kf.set_state(x0[:, None].astype(npd), to_blocks(P)[:, None].astype(npd))
        tr, ld, _, _ = kf.run_events(ev_t[:, None], ev_dt[:, None], ev_p[:, :, None].contiguous(),
                                     sequential=not parallel)
        tr, ld, stt = tr.double().cpu().numpy(), ld.double().cpu().numpy(), st_d.cpu().numpy()
        _, Pb = kf.state()
        Pf = from_blocks(Pb[:, 0].double().cpu().numpy())
        kf.close()
        states = [(prev0, *x0[:6])] + [(stt[i], *tr[i + 1, :, 0]) for i in range(n)]
        logdets = [float(v) for v in ld[:n + 1, 0]]
    if print_output:
        print(f'{selection_method.capitalize()} Scheduled Kalman Filter (GPU): processed {len(states) - 1} measurements')
    return states, logdets, Pf


def sampling_sweep(events, frequencies, start_idx=None, end_idx=None, initial_pt=None, initial_state=None,
                   dtype='f64', device=0, consts=None):
    """The greedy scheduled filter at every processing frequency in ONE kf_run_scheduled launch
    (one filter per frequency) — the experiment behind the reference's
    sampling_sweep/kf_plot_{10..120}.png.  Returns {f: (states, logdets, P)}."""
    w = _scheduled_window_events(events, start_idx, end_idx, initial_pt, initial_state, consts)
    if w is None:
        return {}
    x0, P, prev0, cands = w
    freqs = np.asarray(frequencies, np.float64)
    B = len(freqs)
    npd = np.float64 if dtype == 'f64' else np.float32
    kf = BatchedKF('ref15', B, dtype, device=device, params=_params(consts))
    kf.set_state(np.repeat(x0[:, None], B, 1).astype(npd), np.repeat(to_blocks(P)[:, None], B, 1).astype(npd))
    t, et, pay, _ = _stream_arrays(cands, B, events=events)
    tr, ld, stt, ns = kf.run_scheduled(t, et, pay.astype(npd), np.full(B, prev0), freqs)
    ld0 = _run_streams([[]], x0[None], to_blocks(P)[None], dtype, device, consts=consts)[1][0, 0]
    tr, ld, stt, ns = tr.double().cpu().numpy(), ld.double().cpu().numpy(), stt.cpu().numpy(), ns.cpu().numpy()
    _, Pb = kf.state()
    Pb = Pb.double().cpu().numpy()
    kf.close()
    out = {}
    for b, f in enumerate(frequencies):
        n = int(ns[b])
        states = [(prev0, *x0[:6])] + [(stt[i, b], *tr[i, :, b]) for i in range(n)]
        out[f] = (states, [float(ld0)] + [float(v) for v in ld[:n, b]], from_blocks(Pb[:, b]))
    return out
