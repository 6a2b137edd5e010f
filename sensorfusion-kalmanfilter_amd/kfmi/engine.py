"""BatchedKF — the Python face of libkfmi.so: B independent Kalman filters on one MI355X.

The per-step call shape follows the reference's fusion loop (kf_workers.py:688-717):
``predict(dt, u)`` then ``update(z)`` per event, or the fused ``run(...)`` over T steps
(the hot path, one kernel launch).  Device buffers are torch tensors (torch is only the
allocator / stream provider here); all arithmetic happens in the HIP kernels.
"""
from __future__ import annotations

import collections
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import KFError, check

MODELS = {
    # name: (model id, n, m, c, covariance rows)
    'cv2': (_lib.KF_MODEL_CV2, 4, 2, 2, 10),    # 4-state/2-meas, hw5_2.py:219-304 restricted to [x,y,vx,vy]
    'cv3': (_lib.KF_MODEL_CV3, 6, 3, 3, 21),    # 6-state/3-meas, kf_workers.py:493-614 restricted to pos/vel
    'ref15': (_lib.KF_MODEL_REF15, 15, 3, 0, 27),  # the reference's 15-state model; P block-packed
    'ref8': (_lib.KF_MODEL_REF8, 8, 2, 0, 15),     # hw5_2.py's 8-state model; P block-packed
}
REF_MODELS = ('ref15', 'ref8')
TRAJ_WIDTH = {'ref15': 6, 'ref8': 3}  # kf_workers.py:714 (x, y, z, roll, pitch, yaw); hw5_2.py:369 (x, y, theta)
DTYPES = {'f32': (_lib.KF_F32, torch.float32, np.float32), 'f64': (_lib.KF_F64, torch.float64, np.float64)}


# kf_set_option (include/kf.h): option name -> (id, value names); 0 = the library's choice
OPTIONS = {
    'predict': (_lib.KF_OPT_PREDICT, {'auto': 0, 'deferred': 0, 'eager': 1}),
    'cv_kernel': (_lib.KF_OPT_CV_KERNEL, {'auto': 0, 'general': 1, 'block2': 2, 'block4': 4, 'block8': 8}),
    'blocks_per_cu': (_lib.KF_OPT_BLOCKS_PER_CU, {'auto': 0}),
    'events_kernel': (_lib.KF_OPT_EVENTS_KERNEL, {'auto': 0, 'lane': 1, 'chain': 2, 'lds': 3, 'gated': 4}),
    'stream': (_lib.KF_OPT_STREAM, {'auto': 0, 'off': 1}),
    'stream_chunks': (_lib.KF_OPT_STREAM_CHUNKS, {'auto': 0}),
    'stream_final': (_lib.KF_OPT_STREAM_FINAL, {'auto': 0, 'off': 0, 'on': 1}),
    'start_threads': (_lib.KF_OPT_START_THREADS, {'auto': 0}),
    'search_kernel': (_lib.KF_OPT_SEARCH_KERNEL, {'auto': 0, 'cm': 1, 'pm': 2}),
    'search_pm': (_lib.KF_OPT_SEARCH_PM, {'auto': 0, 'lds': 0, 'regs': 1}),
    'search_head': (_lib.KF_OPT_SEARCH_HEAD, {'auto': 0, 'on': 0, 'off': 1}),
    'search_end': (_lib.KF_OPT_SEARCH_END, {'auto': 0, 'on': 0, 'off': 1}),
    'search_pair': (_lib.KF_OPT_SEARCH_PAIR, {'auto': 0, 'off': 1, 'all': 2, 'cm': 3}),
    'axis_sym': (_lib.KF_OPT_AXIS_SYM, {'auto': 0, 'on': 0, 'off': 1}),
    'sched_kernel': (_lib.KF_OPT_SCHED_KERNEL, {'auto': 0, 'regs': 1, 'fused': 2, 'two_pass': 3, 'one_launch': 4}),
    'sched_group': (_lib.KF_OPT_SCHED_GROUP, {'auto': 0, 'wave': 1, 'block': 4}),
    'sched_order': (_lib.KF_OPT_SCHED_ORDER, {'auto': 0, 'heaviest_first': 0, 'batch': 1}),
    'sched_rec_time': (_lib.KF_OPT_SCHED_REC_TIME, {'auto': 0, 'off': 0, 'on': 1}),
}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def default_params(model):
    p = _lib.kf_params()
    check(_lib.lib().kf_default_params(MODELS[model][0], ctypes.byref(p)))
    return p


def consts_rows(model):
    """Rows R of run_sweep's ``consts`` table for a reference model (kf_consts_rows): q per state,
    then r_imu per state, then r_gps per axis; 33 for 'ref15', 18 for 'ref8'."""
    n = ctypes.c_int(0)
    check(_lib.lib().kf_consts_rows(MODELS[model][0], ctypes.byref(n)))
    return n.value


def consts_table(model, sets):
    """The [R, B] float64 table of B constant sets (kfmi.ref15.ModelConsts of ``model``): column f
    is sets[f]'s q, r_imu, r_gps.  Their P0 is not part of it (set_state carries it)."""
    for c in sets:
        if getattr(c, 'model', None) != model:
            raise KFError(_lib.KF_EINVAL, f'consts: a constant set of model {getattr(c, "model", None)!r} for a '
                                          f'{model} handle')
    tab = np.empty((consts_rows(model), len(sets)), np.float64)
    for f, c in enumerate(sets):
        tab[:, f] = np.concatenate([c.q, c.r_imu, c.r_gps])
    return tab


# rows of run_sweep_scores' [8, B] table (kf.h's KF_SCORE_*)
SCORE_ROWS = {'gps_n': _lib.KF_SCORE_GPS_N, 'gps_nis': _lib.KF_SCORE_GPS_NIS,
              'gps_logdet_s': _lib.KF_SCORE_GPS_LOGDET_S, 'imu_n': _lib.KF_SCORE_IMU_N,
              'imu_nis': _lib.KF_SCORE_IMU_NIS, 'imu_logdet_s': _lib.KF_SCORE_IMU_LOGDET_S,
              'pos_n': _lib.KF_SCORE_POS_N, 'pos_sse': _lib.KF_SCORE_POS_SSE}
assert len(SCORE_ROWS) == _lib.KF_SCORE_ROWS

SweepScores = collections.namedtuple('SweepScores', 'scores n_updated traj logdet updated ckpt_x ckpt_P')
SmoothedSweep = collections.namedtuple('SmoothedSweep', 'x P traj logdet status')
SmoothedSweepEm = collections.namedtuple('SmoothedSweepEm', 'x P traj logdet status em')
SmoothedRun = collections.namedtuple('SmoothedRun', 'x P logdet status')
RunSmoothed = collections.namedtuple('RunSmoothed', 'traj cov logdet smoothed')
ScoredRun = collections.namedtuple('ScoredRun', 'scores traj cov logdet')
SmoothedEm = collections.namedtuple('SmoothedEm', 'x P logdet status init_x init_P em')
NoiseFit = collections.namedtuple('NoiseFit', 'consts history nll status')

# rows of smooth_run_em's [4 + d, B] table (kf.h's KF_EM_*; 'r' is the first of d rows)
EM_ROWS = {'n_trans': _lib.KF_EM_N_TRANS, 'q_pos': _lib.KF_EM_Q_POS, 'q_vel': _lib.KF_EM_Q_VEL,
           'n_fix': _lib.KF_EM_N_FIX, 'r': _lib.KF_EM_R}


def cv_consts_table(model, sets):
    """The [2 + d, B] float64 table of B constant sets for a 'cv2' / 'cv3' handle (run_scores,
    smooth_run's ``consts``): column f is sets[f] = (q_pos, q_vel, r) or a dict with those keys, r
    the d diagonal entries of R (a scalar: the same on every axis).  P0 is not part of it."""
    if model not in ('cv2', 'cv3'):
        raise KFError(_lib.KF_EINVAL, f'cv_consts_table: model {model!r} is not cv2 / cv3')
    d = MODELS[model][2]
    tab = np.empty((_lib.KF_CV_CONST_ROWS(d), len(sets)), np.float64)
    for f, c in enumerate(sets):
        try:
            q_pos, q_vel, r = (c['q_pos'], c['q_vel'], c['r']) if isinstance(c, dict) else c
            r = np.broadcast_to(np.asarray(r, np.float64), (d,)) if np.ndim(r) == 0 else np.asarray(r, np.float64)
            q_pos, q_vel = float(q_pos), float(q_vel)
        except (KeyError, TypeError, ValueError) as e:
            raise KFError(_lib.KF_EINVAL, f'cv_consts_table: set {f}: (q_pos, q_vel, r[{d}]) expected: {e}') from e
        if r.shape != (d,):
            raise KFError(_lib.KF_EINVAL, f'cv_consts_table: set {f}: r has shape {r.shape}, expected ({d},)')
        tab[_lib.KF_CV_CONST_Q_POS, f] = q_pos
        tab[_lib.KF_CV_CONST_Q_VEL, f] = q_vel
        tab[_lib.KF_CV_CONST_R:, f] = r
    return tab


def cv_em_update(em, consts, model):
    """EM's M-step on smooth_run_em's statistics, per filter, in torch where the tables live: from
    em [4 + d, B] and the table consts [2 + d, B] it was gathered under, the new table with
    q_pos = Q_POS / (d N_TRANS), q_vel = Q_VEL / (d N_TRANS) and r_i = R_i / N_FIX.  A zero count
    keeps the old value (no transition of a positive dt: both q; no applied fix: every r).  Tensors
    (any device) or arrays; the result is of consts' kind.  A failed filter's NaN rows pass through."""
    if model not in ('cv2', 'cv3'):
        raise KFError(_lib.KF_EINVAL, f'cv_em_update: model {model!r} is not cv2 / cv3')
    d = MODELS[model][2]
    as_array = not torch.is_tensor(consts)
    c = torch.as_tensor(consts, dtype=torch.float64)
    e = torch.as_tensor(em, dtype=torch.float64).to(c.device)
    rows_e, rows_c = _lib.KF_EM_ROWS(d), _lib.KF_CV_CONST_ROWS(d)
    if e.ndim != 2 or c.ndim != 2 or e.shape[0] != rows_e or c.shape[0] != rows_c or e.shape[1] != c.shape[1]:
        raise KFError(_lib.KF_EINVAL, f'cv_em_update: em {tuple(e.shape)} / consts {tuple(c.shape)}, expected '
                                      f'({_lib.KF_EM_ROWS(d)}, B) / ({_lib.KF_CV_CONST_ROWS(d)}, B)')
    n_tr, n_fix = e[_lib.KF_EM_N_TRANS], e[_lib.KF_EM_N_FIX]
    out = torch.empty_like(c)
    for row, src in ((_lib.KF_CV_CONST_Q_POS, _lib.KF_EM_Q_POS), (_lib.KF_CV_CONST_Q_VEL, _lib.KF_EM_Q_VEL)):
        out[row] = torch.where(n_tr > 0, e[src] / (d * n_tr), c[row])
    out[_lib.KF_CV_CONST_R:] = torch.where(n_fix > 0, e[_lib.KF_EM_R:] / n_fix, c[_lib.KF_CV_CONST_R:])
    return out.numpy() if as_array else out


def em_rows(model):
    """Rows of smooth_sweep_em's table for a reference model (kf_em_rows): 36 for 'ref15', 21 for
    'ref8'."""
    n = ctypes.c_int(0)
    check(_lib.lib().kf_em_rows(MODELS[model][0], ctypes.byref(n)))
    return n.value


def ref_em_rows(model):
    """Where smooth_sweep_em's blocks start for 'ref15' / 'ref8' (kf.h's KF_REF_EM_*): a dict of
    n_trans, q, n_imu, r_imu, n_gps, r_gps ('q', 'r_imu', 'r_gps': the first of n, n, m rows) and
    rows, the table's height."""
    if model not in REF_MODELS:
        raise KFError(_lib.KF_EINVAL, f'ref_em_rows: model {model!r} is not ref15 / ref8')
    n, m = MODELS[model][1], MODELS[model][2]
    return {'n_trans': _lib.KF_REF_EM_N_TRANS, 'q': _lib.KF_REF_EM_Q, 'n_imu': _lib.KF_REF_EM_N_IMU(n),
            'r_imu': _lib.KF_REF_EM_R_IMU(n), 'n_gps': _lib.KF_REF_EM_N_GPS(n), 'r_gps': _lib.KF_REF_EM_R_GPS(n),
            'rows': _lib.KF_REF_EM_ROWS(n, m)}


# the states whose IMU pseudo-measurement row is the sensor's own value (attitude, rate,
# acceleration); the position and velocity rows are built from the predicted state
IMU_MEASURED = {'ref15': (3, 4, 5, 9, 10, 11, 12, 13, 14), 'ref8': (2, 5, 6, 7)}


def ref_em_update(em, consts, model, imu_rows='measured'):
    """EM's M-step on smooth_sweep_em's statistics, per filter, in torch where the tables live: from
    em [ROWS, B] and the table consts [R, B] (run_sweep's, the one it was gathered under), the new
    table with q_i = Q_i / N_TRANS, r_imu,i = R_IMU_i / N_IMU and r_gps,i = R_GPS_i / N_GPS.  A zero
    count keeps the old values of its block, and a q row whose old value is 0 stays 0 (the model's
    way of saying the state has no process noise).  ``imu_rows``: 'measured' (the default) updates
    only the R_imu rows whose z is sensor data (attitude, rate, acceleration: IMU_MEASURED) and keeps
    the position and velocity rows, whose z the forward run built from its own predicted state;
    'all' updates every row; 'none' leaves R_imu alone.  Tensors (any device) or arrays; the result
    is of consts' kind.  A failed filter's NaN rows pass through."""
    if model not in REF_MODELS:
        raise KFError(_lib.KF_EINVAL, f'ref_em_update: model {model!r} is not ref15 / ref8')
    if imu_rows not in ('measured', 'all', 'none'):
        raise KFError(_lib.KF_EINVAL, f"ref_em_update: imu_rows {imu_rows!r} is not 'measured', 'all' or 'none'")
    n, m = MODELS[model][1], MODELS[model][2]
    r = ref_em_rows(model)
    as_array = not torch.is_tensor(consts)
    c = torch.as_tensor(consts, dtype=torch.float64)
    e = torch.as_tensor(em, dtype=torch.float64).to(c.device)
    if e.ndim != 2 or c.ndim != 2 or e.shape[0] != r['rows'] or c.shape[0] != 2 * n + m or e.shape[1] != c.shape[1]:
        raise KFError(_lib.KF_EINVAL, f'ref_em_update: em {tuple(e.shape)} / consts {tuple(c.shape)}, expected '
                                      f'({r["rows"]}, B) / ({2 * n + m}, B)')
    n_tr, n_imu, n_gps = e[r['n_trans']], e[r['n_imu']], e[r['n_gps']]
    out = c.clone()
    q_old = c[:n]
    out[:n] = torch.where((n_tr > 0) & (q_old != 0), e[r['q']:r['q'] + n] / n_tr, q_old)
    if imu_rows != 'none':
        rows = list(range(n)) if imu_rows == 'all' else list(IMU_MEASURED[model])
        idx = torch.as_tensor(rows, device=c.device)
        out[n + idx] = torch.where(n_imu > 0, e[r['r_imu'] + idx] / n_imu, c[n + idx])
    out[2 * n:] = torch.where(n_gps > 0, e[r['r_gps']:r['r_gps'] + m] / n_gps, c[2 * n:])
    return out.numpy() if as_array else out


def innovation_nll(scores, model, sensor):
    """The Gaussian innovation negative log-likelihood per filter from run_sweep_scores' table
    ([8, B], a tensor or an array): -sum over the sensor's applied updates of log N(y; 0, S) =
    0.5 (NIS + logdet_S + n m log 2 pi), m the measurement's length (GPS 3 | 2, IMU 15 | 8 for
    'ref15' | 'ref8').  ``sensor``: 'gps' | 'imu'.  run_scores' table of a 'cv2' / 'cv3' handle:
    'gps' only, m = d."""
    if model in ('cv2', 'cv3') and sensor == 'gps':
        m = MODELS[model][2]
    elif model not in REF_MODELS or sensor not in ('gps', 'imu'):
        raise ValueError(f'innovation_nll: model {model!r}, sensor {sensor!r}')
    else:
        m = {'ref15': (3, 15), 'ref8': (2, 8)}[model][sensor == 'imu']
    n, nis, ld = (scores[SCORE_ROWS[f'{sensor}_{k}']] for k in ('n', 'nis', 'logdet_s'))
    return 0.5 * (nis + ld + n * (m * math.log(2.0 * math.pi)))


def device_count():
    n = ctypes.c_int(0)
    check(_lib.lib().kf_device_count(ctypes.byref(n)))
    return n.value


class BatchedKF:
    """``batch`` independent filters of ``model`` ('cv2' | 'cv3') in ``dtype`` ('f32' | 'f64').

    State layout in HBM (SoA, filter index fastest): x [n, B], P [n(n+1)/2, B] (upper
    triangle packed row-major), status [B] int32.
    """

    def __init__(self, model='cv3', batch=1, dtype='f64', device=0, params=None, options=None):
        if model not in MODELS:
            raise ValueError(f'unknown model {model!r}; choose from {sorted(MODELS)}')
        if dtype not in DTYPES:
            raise ValueError(f'unknown dtype {dtype!r}; choose from {sorted(DTYPES)}')
        self.model = model
        self.dtype = dtype
        self.batch = int(batch)
        if self.batch < 0:
            raise ValueError('batch must be >= 0')
        self.device = torch.device('cuda', device)
        _, self.n, self.m, self.c, self.ntri = MODELS[model]
        self.torch_dtype = DTYPES[dtype][1]
        L = _lib.lib()
        check(L.kf_init(device))
        torch.cuda.set_device(self.device)
        # reference models: params carries the caller's diagonal constants (kf_params.ref_*,
        # e.g. kfmi.ref15.ModelConsts(...).params()), None = the reference's
        self.params = params if params is not None else (None if model in REF_MODELS else default_params(model))
        h = ctypes.c_void_p()
        check(L.kf_alloc(ctypes.byref(h), MODELS[model][0], self.batch, DTYPES[dtype][0],
                         ctypes.byref(self.params) if self.params is not None else None))
        self._h = h
        for k, v in (options or {}).items():
            self.set_option(k, v)

    # -- lifecycle ---------------------------------------------------------------------
    def close(self):
        if getattr(self, '_h', None):
            _lib.lib().kf_free(self._h)
            self._h = None

    def release_retired(self):
        """Free the workspaces earlier graph captures used and larger eager calls replaced
        (kf_release_retired); only once every graph captured from this handle is destroyed.
        Returns the bytes freed."""
        out = ctypes.c_int64(0)
        check(_lib.lib().kf_release_retired(self.handle, ctypes.byref(out)))
        return out.value

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        if not self._h:
            raise KFError(_lib.KF_EINVAL, 'BatchedKF is closed')
        return self._h

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # -- options (kf_set_option): per handle, nothing is read from the environment --------
    def set_option(self, name, value):
        """Select a kernel variant for this handle (A/B runs, tests); ``name`` is one of
        OPTIONS, ``value`` an int or one of that option's names (``'auto'`` = 0 everywhere)."""
        opt, names = OPTIONS[name]
        v = names[value] if isinstance(value, str) else int(value)
        check(_lib.lib().kf_set_option(self.handle, opt, v))
        return self

    def get_option(self, name):
        out = ctypes.c_int64(0)
        check(_lib.lib().kf_get_option(self.handle, OPTIONS[name][0], ctypes.byref(out)))
        return out.value

    # -- buffers -------------------------------------------------------------------------
    def empty(self, *shape, dtype=None):
        return torch.empty(shape, dtype=dtype or self.torch_dtype, device=self.device)

    def _dev(self, a, shape, name, dtype=None):
        """Validate (or move) an input stream to a contiguous device tensor of `shape`."""
        dt = dtype or self.torch_dtype
        if isinstance(a, np.ndarray):
            a = torch.from_numpy(np.ascontiguousarray(a))
        if not torch.is_tensor(a):
            raise TypeError(f'{name}: expected a torch tensor or numpy array, got {type(a)}')
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f'{name}: shape {tuple(a.shape)} != expected {tuple(shape)}')
        if a.dtype != dt:
            raise TypeError(f'{name}: dtype {a.dtype} != expected {dt}')
        if a.device != self.device:
            a = a.to(self.device)
        return a.contiguous()

    # -- state ---------------------------------------------------------------------------
    def reset(self, x0=None):
        """x = x0 ([n, B]; None = zeros), P = P0, status = OK (kf_workers.py:651-666)."""
        x0d = self._dev(x0, (self.n, self.batch), 'x0') if x0 is not None else None
        check(_lib.lib().kf_reset(self.handle, _ptr(x0d), self._stream()))

    def set_state(self, x, P):
        xd = self._dev(x, (self.n, self.batch), 'x')
        Pd = self._dev(P, (self.ntri, self.batch), 'P')
        check(_lib.lib().kf_set_state(self.handle, _ptr(xd), _ptr(Pd), 1, self._stream()))

    def state(self):
        """(x [n, B], P_packed [n(n+1)/2, B]) as new device tensors."""
        x = self.empty(self.n, self.batch)
        P = self.empty(self.ntri, self.batch)
        check(_lib.lib().kf_get_state(self.handle, _ptr(x), _ptr(P), 1, self._stream()))
        return x, P

    def status(self):
        s = torch.empty(self.batch, dtype=torch.int32, device=self.device)
        check(_lib.lib().kf_get_status(self.handle, _ptr(s), 1, self._stream()))
        return s

    # -- per-step call shape (kf_workers.py:688-717) ----------------------------------------
    def predict(self, dt, u=None, dt_per_filter=None, logdet=False):
        """x = F(dt) x + G(dt) u, P = F P F^T + Q(dt).  Returns logdet(P_pred) [B] if asked.
        Reference models: one KF_EVENT_PREDICT event per filter (kf_run_events, T = 1)."""
        if self.model in REF_MODELS:
            if u is not None:
                raise ValueError(f'{self.model}: no control input (the IMU enters as a measurement)')
            dts = (dt_per_filter if dt_per_filter is not None else
                   np.full(self.batch, float(dt if dt is not None else 0.0)))
            return self._event(_lib.KF_EVENT_PREDICT, dts, None, None, logdet)
        ud = self._dev(u, (self.c, self.batch), 'u') if u is not None else None
        dtf = (self._dev(dt_per_filter, (self.batch,), 'dt_per_filter', torch.float64)
               if dt_per_filter is not None else None)
        ld = self.empty(self.batch) if logdet else None
        check(_lib.lib().kf_predict(self.handle, float(dt if dt is not None else 0.0), _ptr(dtf),
                                    _ptr(ud), _ptr(ld), self._stream()))
        return ld

    def update(self, z, mask=None, logdet=True, sensor='gps'):
        """GPS update with z [m, B]; mask [B] (0 = skip).  Returns logdet(P) [B] if asked.
        Reference models: a GPS fix event at dt = 0 (the predict is then exactly the identity);
        the IMU pseudo-measurement is built from the predicted state and the event's dt
        (kf_workers.py:698-706), so it is an event: ``step('imu', dt, payload)``."""
        if self.model in REF_MODELS:
            if sensor != 'gps':
                raise ValueError("the IMU update needs the event's dt: use step('imu', dt, payload)")
            zz = z.cpu().numpy() if torch.is_tensor(z) else np.asarray(z)
            if zz.shape != (self.m, self.batch):
                raise ValueError(f'z: shape {zz.shape} != expected {(self.m, self.batch)}')
            pay = np.zeros((9, self.batch))
            pay[:self.m] = zz
            return self._event(_lib.KF_EVENT_GPS, np.zeros(self.batch), pay, mask, logdet)
        zd = self._dev(z, (self.m, self.batch), 'z')
        md = self._dev(mask, (self.batch,), 'mask', torch.uint8) if mask is not None else None
        ld = self.empty(self.batch) if logdet else None
        check(_lib.lib().kf_update(self.handle, _ptr(zd), _ptr(md), _ptr(ld), self._stream()))
        return ld

    def step(self, sensor, dt, payload, mask=None, logdet=True):
        """Reference models: one event of the reference loop for every filter (kf_workers.py:
        688-717): predict over dt (scalar or [B]), then the GPS fix (payload [3, B]: easting,
        northing, altitude) or the IMU pseudo-measurement (payload [9, B]: roll, pitch, yaw,
        wx, wy, wz, ax, ay, az).  mask [B]: 0 = no event for that filter.  Returns logdet [B]."""
        if self.model not in REF_MODELS:
            raise ValueError('step() is the event call of the reference models (ref15 / ref8)')
        et = {'gps': _lib.KF_EVENT_GPS, 'imu': _lib.KF_EVENT_IMU}.get(sensor)
        if et is None:
            raise ValueError(f"sensor must be 'gps' or 'imu', not {sensor!r}")
        pp = payload.cpu().numpy() if torch.is_tensor(payload) else np.asarray(payload)
        rows = 3 if sensor == 'gps' else 9
        if pp.shape != (rows, self.batch):
            raise ValueError(f'payload: shape {pp.shape} != expected {(rows, self.batch)}')
        pay = np.zeros((9, self.batch))
        pay[:rows] = pp
        dts = np.array(np.broadcast_to(np.asarray(dt, dtype=np.float64), (self.batch,)))
        return self._event(et, dts, pay, mask, logdet)

    def logdet(self):
        """log det P of every filter's current covariance [B] (no state change)."""
        if self.model in REF_MODELS:
            return self._event(_lib.KF_EVENT_NONE, np.zeros(self.batch), None, None, True)
        return self.predict(0.0, logdet=True)  # F(0) = I, Q(0) = 0: P is left exactly as it is

    def _event(self, etype, dts, payload, mask, logdet):
        et = np.full((1, self.batch), etype, np.uint8)
        if mask is not None:
            m = mask.cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)
            et[0, m.reshape(-1) == 0] = _lib.KF_EVENT_NONE
        npd = DTYPES[self.dtype][2]
        pay = np.zeros((1, 9, self.batch), npd) if payload is None else np.asarray(payload, npd)[None]
        _, ld, _, _ = self.run_events(et, np.asarray(dts, np.float64).reshape(1, self.batch), pay, traj=False,
                                      logdet=logdet)
        return ld[0] if logdet else None

    # -- fused hot path -----------------------------------------------------------------
    def run(self, u, z, dt=None, dt_steps=None, update_every=1, mask=None, traj=True, logdet=True,
            out=None):
        """T fused predict(+update) steps in one launch.

        u [T, c, B]; z [T // update_every, m, B]; dt scalar or dt_steps [T] (float64);
        mask [T // update_every, B] uint8 or None.  Returns (traj [T, n, B], logdet [T, B]);
        pass ``out=(traj, logdet)`` to reuse buffers (either may be None to skip it)."""
        T = int(u.shape[0])
        U = T // update_every
        ud = self._dev(u, (T, self.c, self.batch), 'u')
        zd = self._dev(z, (U, self.m, self.batch), 'z') if U > 0 else None
        md = self._dev(mask, (U, self.batch), 'mask', torch.uint8) if mask is not None else None
        dts = self._dev(dt_steps, (T,), 'dt_steps', torch.float64) if dt_steps is not None else None
        if dts is None and dt is None:
            raise ValueError('run: give dt (scalar) or dt_steps [T]')
        if out is not None:
            tr, ld = out
            if tr is not None:
                tr = self._dev(tr, (T, self.n, self.batch), 'traj')
            if ld is not None:
                ld = self._dev(ld, (T, self.batch), 'logdet')
        else:
            tr = self.empty(T, self.n, self.batch) if traj else None
            ld = self.empty(T, self.batch) if logdet else None
        check(_lib.lib().kf_run(self.handle, T, float(dt or 0.0), _ptr(dts), _ptr(ud), _ptr(zd),
                                _ptr(md), int(update_every), _ptr(tr), _ptr(ld), self._stream()))
        return tr, ld

    def _need_cv(self, what):
        if self.model in REF_MODELS:
            raise KFError(_lib.KF_EINVAL, f'{what}: needs a cv2 or cv3 handle')

    def run_rec(self, u, z, dt=None, dt_steps=None, update_every=1, mask=None, traj=True, cov=True, logdet=True):
        """``run`` that also records the filtered covariance (kf_run_rec): the forward half of a
        smoothed track.  u [T, c, B] or None (zero control; then z, dt_steps or mask give T:
        T = len(dt_steps), else update_every * len(z)); the other arguments as in ``run``.
        Returns (traj [T, n, B], cov [T, 3 d, B], logdet [T, B]), None where not asked for; rows
        3 i .. 3 i + 2 of cov[t] are axis i's (pp, pv, vv) after step t.  State, status, traj and
        logdet are ``run``'s bit for bit.  KFError(KF_EINVAL) unless the handle's P is
        block-diagonal over the axes and R is diagonal."""
        self._need_cv('run_rec')
        if u is not None:
            T = int(u.shape[0])
        elif dt_steps is not None:
            T = int(dt_steps.shape[0])
        else:
            T = int(z.shape[0]) * int(update_every)
        U = T // update_every
        ud = self._dev(u, (T, self.c, self.batch), 'u') if u is not None else None
        zd = self._dev(z, (U, self.m, self.batch), 'z') if U > 0 else None
        md = self._dev(mask, (U, self.batch), 'mask', torch.uint8) if mask is not None else None
        dts = self._dev(dt_steps, (T,), 'dt_steps', torch.float64) if dt_steps is not None else None
        if dts is None and dt is None:
            raise ValueError('run_rec: give dt (scalar) or dt_steps [T]')
        tr = self.empty(T, self.n, self.batch) if traj else None
        cv = self.empty(T, 3 * self.c, self.batch) if cov else None
        ld = self.empty(T, self.batch) if logdet else None
        check(_lib.lib().kf_run_rec(self.handle, T, float(dt or 0.0), _ptr(dts), _ptr(ud), _ptr(zd), _ptr(md),
                                    int(update_every), _ptr(tr), _ptr(cv), _ptr(ld), self._stream()))
        return tr, cv, ld

    def run_scores(self, u, z, consts=None, track=None, dt=None, dt_steps=None, update_every=1, mask=None,
                   scores=True, traj=False, cov=False, logdet=False):
        """``run_rec`` under per-filter constants, scored in the launch (kf_run_scores).  consts
        [2 + d, B] float64 (``cv_consts_table``) or None = the handle's; track [T, d, B] in the
        handle's dtype (NaN rows are not scored) or None; the other arguments as in ``run_rec``.
        Returns ScoredRun(scores [8, B] float64 in SCORE_ROWS' layout, traj, cov, logdet), None
        where not asked for.  ``innovation_nll(scores, model, 'gps')`` gives the likelihood."""
        self._need_cv('run_scores')
        if u is not None:
            T = int(u.shape[0])
        elif dt_steps is not None:
            T = int(dt_steps.shape[0])
        else:
            T = int(z.shape[0]) * int(update_every)
        U = T // update_every
        ud = self._dev(u, (T, self.c, self.batch), 'u') if u is not None else None
        zd = self._dev(z, (U, self.m, self.batch), 'z') if U > 0 else None
        md = self._dev(mask, (U, self.batch), 'mask', torch.uint8) if mask is not None else None
        dts = self._dev(dt_steps, (T,), 'dt_steps', torch.float64) if dt_steps is not None else None
        if dts is None and dt is None:
            raise ValueError('run_scores: give dt (scalar) or dt_steps [T]')
        cd = self._cv_consts(consts)
        tk = self._dev(track, (T, self.c, self.batch), 'track') if track is not None else None
        if tk is not None and not scores:
            raise KFError(_lib.KF_EINVAL, 'run_scores: a track needs scores=True')
        sc = torch.empty(_lib.KF_SCORE_ROWS, self.batch, dtype=torch.float64, device=self.device) if scores else None
        tr = self.empty(T, self.n, self.batch) if traj else None
        cv = self.empty(T, 3 * self.c, self.batch) if cov else None
        ld = self.empty(T, self.batch) if logdet else None
        check(_lib.lib().kf_run_scores(self.handle, T, float(dt or 0.0), _ptr(dts), _ptr(ud), _ptr(zd), _ptr(md),
                                       int(update_every), _ptr(cd), _ptr(tk), _ptr(sc), _ptr(tr), _ptr(cv), _ptr(ld),
                                       self._stream()))
        return ScoredRun(sc, tr, cv, ld)

    def _cv_consts(self, consts):
        if consts is None:
            return None
        return self._dev(consts, (_lib.KF_CV_CONST_ROWS(self.c), self.batch), 'consts', torch.float64)

    def smooth_run(self, filt_x, filt_P, u=None, dt=None, dt_steps=None, x=True, P=False, logdet=False, status=True,
                   inplace=False, consts=None):
        """The RTS smoother over a ``run_rec`` record (kf_smooth_run): filt_x [T, n, B] its traj,
        filt_P [T, 3 d, B] its cov (device tensors or arrays); u, dt / dt_steps the forward run's
        (u None: zero control).  An f64 cv2 / cv3 handle, whose state and status are not touched.
        Returns SmoothedRun(x [T, n, B], P [T, 3 d, B], logdet [T, B], status [B] int32), None where
        not asked for; row T - 1 is the filtered row.  ``inplace``: x and P (where asked for)
        overwrite filt_x / filt_P, which must then be contiguous device tensors.  A filter whose
        record is not positive definite (or holds a NaN) has NaN rows from there down to 0 and
        KF_ENOTSPD in ``status``.  consts [2 + d, B] (``cv_consts_table``): filter f smooths under
        column f's q_pos / q_vel (kf_smooth_run_params), as ``run_scores`` filtered it."""
        self._need_cv('smooth_run')
        if self.dtype != 'f64':
            raise KFError(_lib.KF_EINVAL, 'smooth_run: needs an f64 handle')
        T = int(filt_x.shape[0])
        if inplace and not (torch.is_tensor(filt_x) and torch.is_tensor(filt_P) and filt_x.device == self.device
                            and filt_P.device == self.device and filt_x.is_contiguous() and filt_P.is_contiguous()
                            and filt_x.dtype == self.torch_dtype and filt_P.dtype == self.torch_dtype):
            raise KFError(_lib.KF_EINVAL, 'smooth_run: inplace needs contiguous float64 device tensors filt_x / filt_P')
        fx = self._dev(filt_x, (T, self.n, self.batch), 'filt_x')
        fP = self._dev(filt_P, (T, 3 * self.c, self.batch), 'filt_P')
        ud = self._dev(u, (T, self.c, self.batch), 'u') if u is not None else None
        dts = self._dev(dt_steps, (T,), 'dt_steps', torch.float64) if dt_steps is not None else None
        if dts is None and dt is None:
            raise ValueError('smooth_run: give dt (scalar) or dt_steps [T]')
        sx = (fx if inplace else self.empty(T, self.n, self.batch)) if x else None
        sP = (fP if inplace else self.empty(T, 3 * self.c, self.batch)) if P else None
        ld = self.empty(T, self.batch) if logdet else None
        st = torch.zeros(self.batch, dtype=torch.int32, device=self.device) if status else None
        if consts is not None:
            check(_lib.lib().kf_smooth_run_params(self.handle, T, float(dt or 0.0), _ptr(dts), _ptr(ud), _ptr(fx),
                                                  _ptr(fP), _ptr(sx), _ptr(sP), _ptr(ld), _ptr(st),
                                                  _ptr(self._cv_consts(consts)), self._stream()))
        else:
            check(_lib.lib().kf_smooth_run(self.handle, T, float(dt or 0.0), _ptr(dts), _ptr(ud), _ptr(fx), _ptr(fP),
                                           _ptr(sx), _ptr(sP), _ptr(ld), _ptr(st), self._stream()))
        return SmoothedRun(sx, sP, ld, st)

    def run_smoothed(self, u, z, dt=None, dt_steps=None, update_every=1, mask=None, logdet=True, P=False,
                     smoothed_logdet=False, consts=None):
        """``run_rec`` then ``smooth_run`` out of place: RunSmoothed(traj, cov, logdet, smoothed), the
        filtered track, covariance record and log det, and ``smoothed`` = SmoothedRun(x, P, logdet,
        status).  An f64 cv2 / cv3 handle.  consts [2 + d, B]: both halves under per-filter
        constants (``run_scores`` without scores, then ``smooth_run(consts=...)``)."""
        if self.dtype != 'f64':
            raise KFError(_lib.KF_EINVAL, 'run_smoothed: needs an f64 handle')
        if consts is not None:
            cd = self._cv_consts(consts)
            _, tr, cv, ld = self.run_scores(u, z, consts=cd, dt=dt, dt_steps=dt_steps, update_every=update_every,
                                            mask=mask, scores=False, traj=True, cov=True, logdet=logdet)
            sm = self.smooth_run(tr, cv, u=u, dt=dt, dt_steps=dt_steps, P=P, logdet=smoothed_logdet, consts=cd)
            return RunSmoothed(tr, cv, ld, sm)
        tr, cv, ld = self.run_rec(u, z, dt=dt, dt_steps=dt_steps, update_every=update_every, mask=mask,
                                  logdet=logdet)
        sm = self.smooth_run(tr, cv, u=u, dt=dt, dt_steps=dt_steps, P=P, logdet=smoothed_logdet)
        return RunSmoothed(tr, cv, ld, sm)

    def _block_rows(self):
        """Rows of the tri-packed P [n (n + 1) / 2, B] that a covariance record row holds, in its order."""
        n, d = self.n, self.c
        tri = lambda i, j: i * n - i * (i - 1) // 2 + (j - i)  # noqa: E731
        return [r for i in range(d) for r in (tri(i, i), tri(i, d + i), tri(d + i, d + i))]

    def smooth_run_em(self, filt_x, filt_P, z, u=None, dt=None, dt_steps=None, update_every=1, mask=None, init=None,
                      consts=None, x=False, P=False, logdet=False, status=True, inplace=False, init_out=True, em=True):
        """``smooth_run`` that also gathers one EM iteration's statistics for q_pos, q_vel and R per
        filter (kf_smooth_run_em).  filt_x, filt_P, u, dt / dt_steps, consts, x, P, logdet, status
        and inplace as in ``smooth_run``; z [T // update_every, d, B] (or None: no R statistics),
        mask and update_every the forward run's.  init = (x [n, B], P): the state the forward run
        started from, P tri-packed [n (n + 1) / 2, B] as ``state()`` returns it (its same-axis rows are
        gathered) or block-packed [3 d, B]; given, the transition into step 0 is counted and, with
        init_out, the smoothed initial row returned.  Returns SmoothedEm(x, P, logdet, status,
        init_x [n, B], init_P [3 d, B], em [4 + d, B] float64 in EM_ROWS' layout), None where not
        asked for.  ``cv_em_update(em, consts, model)`` is the M-step."""
        self._need_cv('smooth_run_em')
        if self.dtype != 'f64':
            raise KFError(_lib.KF_EINVAL, 'smooth_run_em: needs an f64 handle')
        T = int(filt_x.shape[0])
        if inplace and not (torch.is_tensor(filt_x) and torch.is_tensor(filt_P) and filt_x.device == self.device
                            and filt_P.device == self.device and filt_x.is_contiguous() and filt_P.is_contiguous()
                            and filt_x.dtype == self.torch_dtype and filt_P.dtype == self.torch_dtype):
            raise KFError(_lib.KF_EINVAL, 'smooth_run_em: inplace needs contiguous float64 device tensors filt_x / '
                                          'filt_P')
        k = int(update_every)
        if k < 1:
            raise KFError(_lib.KF_EINVAL, f'smooth_run_em: update_every = {k} < 1')
        U = T // k
        fx = self._dev(filt_x, (T, self.n, self.batch), 'filt_x')
        fP = self._dev(filt_P, (T, 3 * self.c, self.batch), 'filt_P')
        ud = self._dev(u, (T, self.c, self.batch), 'u') if u is not None else None
        zd = self._dev(z, (U, self.m, self.batch), 'z') if (z is not None and U > 0) else None
        md = self._dev(mask, (U, self.batch), 'mask', torch.uint8) if (mask is not None and zd is not None) else None
        dts = self._dev(dt_steps, (T,), 'dt_steps', torch.float64) if dt_steps is not None else None
        if dts is None and dt is None:
            raise ValueError('smooth_run_em: give dt (scalar) or dt_steps [T]')
        ix = iP = six = siP = None
        if init is not None:
            ix = self._dev(init[0], (self.n, self.batch), 'init x')
            iP = init[1]
            if tuple(iP.shape) == (self.ntri, self.batch):
                iP = self._dev(iP, (self.ntri, self.batch), 'init P')[self._block_rows()]
            iP = self._dev(iP, (3 * self.c, self.batch), 'init P')
            if init_out:
                six, siP = self.empty(self.n, self.batch), self.empty(3 * self.c, self.batch)
        sx = (fx if inplace else self.empty(T, self.n, self.batch)) if x else None
        sP = (fP if inplace else self.empty(T, 3 * self.c, self.batch)) if P else None
        ld = self.empty(T, self.batch) if logdet else None
        st = torch.zeros(self.batch, dtype=torch.int32, device=self.device) if status else None
        et = torch.empty(_lib.KF_EM_ROWS(self.c), self.batch, dtype=torch.float64, device=self.device) if em else None
        check(_lib.lib().kf_smooth_run_em(self.handle, T, float(dt or 0.0), _ptr(dts), _ptr(ud), _ptr(zd), _ptr(md), k,
                                          _ptr(fx), _ptr(fP), _ptr(ix), _ptr(iP), _ptr(sx), _ptr(sP), _ptr(ld), _ptr(st),
                                          _ptr(six), _ptr(siP), _ptr(self._cv_consts(consts)), _ptr(et), self._stream()))
        return SmoothedEm(sx, sP, ld, st, six, siP, et)

    def fit_noise(self, u, z, x0=None, consts=None, iters=10, dt=None, dt_steps=None, update_every=1, mask=None):
        """EM for q_pos, q_vel and the diagonal of R, every filter on its own stream, on the device.
        Each of the ``iters`` iterations restores the initial state (``reset(x0)``: x0, the handle's
        P0), filters under the current table (``run_scores``), gathers the statistics with the
        initial row and no smoothed record written (``smooth_run_em``) and takes the M-step
        (``cv_em_update``); a last forward run scores the final table.  consts [2 + d, B]: the start
        (None: the handle's q_pos, q_vel and diagonal R in every filter); u, z, dt / dt_steps,
        update_every and mask as in ``run_rec``.  Returns NoiseFit(consts [2 + d, B], history
        [iters + 1, 2 + d, B] (the table each forward run used: history[0] the start, history[-1]
        the result), nll [iters + 1, B] (``innovation_nll`` of those runs) and status [B] int32 (the
        first non-zero of any run's or smoother's status)).  The handle is left after the last
        forward run.  Nothing inside the loop waits for the device."""
        self._need_cv('fit_noise')
        if self.dtype != 'f64':
            raise KFError(_lib.KF_EINVAL, 'fit_noise: needs an f64 handle')
        d = self.c
        if consts is None:
            r = [self.params.r[i * d + i] for i in range(d)]
            consts = cv_consts_table(self.model, [(self.params.q_pos, self.params.q_vel, r)] * self.batch)
        tab = self._cv_consts(consts).clone()
        x0d = self._dev(x0, (self.n, self.batch), 'x0') if x0 is not None else None
        self.reset(x0d)
        xi, Pi = self.state()
        init = (xi, Pi[self._block_rows()].contiguous())
        kw = dict(dt=dt, dt_steps=dt_steps, update_every=update_every, mask=mask)
        history, nll = [tab], []
        status = torch.zeros(self.batch, dtype=torch.int32, device=self.device)

        def note(s):
            return torch.where(status != 0, status, s)

        for _ in range(int(iters)):
            self.reset(x0d)
            sr = self.run_scores(u, z, consts=tab, traj=True, cov=True, **kw)
            status = note(self.status())
            nll.append(innovation_nll(sr.scores, self.model, 'gps'))
            sm = self.smooth_run_em(sr.traj, sr.cov, z, u=u, init=init, consts=tab, init_out=False, **kw)
            status = note(sm.status)
            tab = cv_em_update(sm.em, tab, self.model)
            history.append(tab)
        self.reset(x0d)
        sr = self.run_scores(u, z, consts=tab, **kw)
        status = note(self.status())
        nll.append(innovation_nll(sr.scores, self.model, 'gps'))
        return NoiseFit(tab, torch.stack(history), torch.stack(nll), status)

    def run_host(self, u, z, dt, update_every=1, chunks=8, traj=None, logdet=None):
        """``run`` for streams that live in host memory (numpy arrays or CPU tensors, the shapes
        of ``run``): T is cut into ``chunks`` time chunks and the H2D copy of chunk i+1, the
        launch on chunk i and the D2H copy of chunk i-1 overlap on three streams (the filter
        state carries across launches in the handle, so the result is that of one ``run``).
        traj/logdet: pinned CPU tensors to fill (allocated pinned when None).  Returns them
        after the last copy has landed.  DESIGN.md §4 gives the measured rate (1.5x serial)."""
        def host(a, shape, name):
            if isinstance(a, np.ndarray):
                a = torch.from_numpy(np.ascontiguousarray(a))
            if tuple(a.shape) != tuple(shape) or a.dtype != self.torch_dtype or a.device.type != 'cpu':
                raise ValueError(f'{name}: expected a CPU {self.torch_dtype} array of shape {tuple(shape)}')
            return a.contiguous() if a.is_pinned() else a.contiguous().pin_memory()
        T, k = int(u.shape[0]), int(update_every)
        if T % k:
            raise ValueError('run_host: T must be a multiple of update_every')
        while chunks > 1 and T % (chunks * k):
            chunks -= 1
        hu = host(u, (T, self.c, self.batch), 'u')
        hz = host(z, (T // k, self.m, self.batch), 'z')
        ht = traj if traj is not None else torch.empty(T, self.n, self.batch, dtype=self.torch_dtype).pin_memory()
        hl = logdet if logdet is not None else torch.empty(T, self.batch, dtype=self.torch_dtype).pin_memory()
        host(ht, (T, self.n, self.batch), 'traj')
        host(hl, (T, self.batch), 'logdet')
        du, dz = self.empty(T, self.c, self.batch), self.empty(T // k, self.m, self.batch)
        dtr, dld = self.empty(T, self.n, self.batch), self.empty(T, self.batch)
        sh, sc, sd = (torch.cuda.Stream(self.device) for _ in range(3))
        prev = torch.cuda.current_stream(self.device)
        sh.wait_stream(prev)
        tc = T // chunks
        for i in range(chunks):
            a, b = i * tc, (i + 1) * tc
            with torch.cuda.stream(sh):
                du[a:b].copy_(hu[a:b], non_blocking=True)
                dz[a // k:b // k].copy_(hz[a // k:b // k], non_blocking=True)
                ev_in = torch.cuda.Event()
                ev_in.record(sh)
            with torch.cuda.stream(sc):
                sc.wait_event(ev_in)
                self.run(du[a:b], dz[a // k:b // k], dt=dt, update_every=k, out=(dtr[a:b], dld[a:b]))
                ev_run = torch.cuda.Event()
                ev_run.record(sc)
            with torch.cuda.stream(sd):
                sd.wait_event(ev_run)
                ht[a:b].copy_(dtr[a:b], non_blocking=True)
                hl[a:b].copy_(dld[a:b], non_blocking=True)
        sd.synchronize()
        prev.wait_stream(sc)
        return ht, hl

    # -- reference models: per-filter event streams ----------------------------------------
    def run_events(self, etype, dt, payload, traj=True, logdet=True, updated=False, threshold=None, cov=False,
                   sequential=False):
        """KF_MODEL_REF15 / KF_MODEL_REF8: T events per filter in one launch (kf_run_events).

        etype [T, B] uint8 (KF_EVENT_*), dt [T, B] float64, payload [T, 9, B] (GPS: e, n, alt;
        IMU: roll, pitch, yaw, wx, wy, wz, ax, ay, az).  threshold: adaptive-threshold gating
        (update only if logdet(P_pred) > threshold).  sequential=True: never the time-parallel
        route kf_run_events takes by itself for one long filter (kf_run_events_seq).  Returns
        (traj [T, W, B], logdet [T, B], updated [T, B], cov [T, rows, B]) with None for outputs
        not asked for (W = 6 for ref15, 3 for ref8; cov is block-packed)."""
        if self.model not in REF_MODELS:
            raise ValueError('run_events needs a ref15 or ref8 handle')
        T = int(etype.shape[0])
        et = self._dev(etype, (T, self.batch), 'etype', torch.uint8)
        dtd = self._dev(dt, (T, self.batch), 'dt', torch.float64)
        pay = self._dev(payload, (T, 9, self.batch), 'payload')
        tr = self.empty(T, TRAJ_WIDTH[self.model], self.batch) if traj else None
        ld = self.empty(T, self.batch) if logdet else None
        up = torch.empty(T, self.batch, dtype=torch.uint8, device=self.device) if updated else None
        cv = self.empty(T, self.ntri, self.batch) if cov else None
        gate = threshold is not None
        fn = _lib.lib().kf_run_events_seq if sequential else _lib.lib().kf_run_events
        check(fn(self.handle, T, _ptr(et), _ptr(dtd), _ptr(pay), _ptr(tr), _ptr(cv), _ptr(ld), _ptr(up), int(gate),
                 float(threshold) if gate else 0.0, self._stream()))
        return tr, ld, up, cv

    def run_events_gates(self, etype, dt, payload, thresholds, traj=True, logdet=True, updated=False, cov=False):
        """run_events(sequential=True) with a gate per filter (kf_run_events_gates): filter f
        updates only where logdet(P_pred) > thresholds[f] ([B] float64; -inf always and without
        evaluating the gate, +inf or NaN never), so always-updating, gated and never-updating
        filters share one launch, each on its own [T, B] column.  Same arguments and returns as
        run_events otherwise."""
        if self.model not in REF_MODELS:
            raise ValueError('run_events_gates needs a ref15 or ref8 handle')
        T = int(etype.shape[0])
        et = self._dev(etype, (T, self.batch), 'etype', torch.uint8)
        dtd = self._dev(dt, (T, self.batch), 'dt', torch.float64)
        pay = self._dev(payload, (T, 9, self.batch), 'payload')
        thr = self._dev(thresholds, (self.batch,), 'thresholds', torch.float64)
        tr = self.empty(T, TRAJ_WIDTH[self.model], self.batch) if traj else None
        ld = self.empty(T, self.batch) if logdet else None
        up = torch.empty(T, self.batch, dtype=torch.uint8, device=self.device) if updated else None
        cv = self.empty(T, self.ntri, self.batch) if cov else None
        check(_lib.lib().kf_run_events_gates(self.handle, T, _ptr(et), _ptr(dtd), _ptr(pay), _ptr(tr), _ptr(cv),
                                             _ptr(ld), _ptr(up), _ptr(thr), self._stream()))
        return tr, ld, up, cv

    def run_stream(self, etype, dt, payload, traj=True, logdet=True, updated=False, cov=False, chunk=0,
                   warmup=-1):
        """One filter (a handle of batch 1) over a long event stream, parallel over time
        (kf_run_stream): etype [T] uint8, dt [T] float64, payload [T, 9].  Same outputs as
        run_events with B = 1 ([T, W, 1], [T, 1], ...).  chunk <= 0 / warmup < 0: the library's
        defaults.  stream_check() tells whether the chunked records stood or the sequential
        fallback rewrote them."""
        if self.model not in REF_MODELS or self.batch != 1:
            raise ValueError('run_stream needs a ref15 or ref8 handle of one filter')
        T = int(etype.shape[0])
        et = self._dev(etype.reshape(T, 1), (T, 1), 'etype', torch.uint8)
        dtd = self._dev(dt.reshape(T, 1), (T, 1), 'dt', torch.float64)
        pay = self._dev(payload.reshape(T, 9, 1), (T, 9, 1), 'payload')
        tr = self.empty(T, TRAJ_WIDTH[self.model], 1) if traj else None
        ld = self.empty(T, 1) if logdet else None
        up = torch.empty(T, 1, dtype=torch.uint8, device=self.device) if updated else None
        cv = self.empty(T, self.ntri, 1) if cov else None
        check(_lib.lib().kf_run_stream(self.handle, T, _ptr(et), _ptr(dtd), _ptr(pay), _ptr(tr), _ptr(cv), _ptr(ld),
                                       _ptr(up), int(chunk), int(warmup), self._stream()))
        return tr, ld, up, cv

    def run_sweep(self, etype, dt, payload, thresholds, traj=True, logdet=True, updated=False, counts=True,
                  checkpoint_every=0, consts=None):
        """ONE event stream under this handle's B adaptive gates in one launch (kf_run_sweep):
        etype [T] uint8, dt [T] float64, payload [T, 9]; filter f runs every event from its own
        state in the handle and updates only where logdet(P_pred) > thresholds[f] ([B] float64;
        -inf always, +inf or NaN never).  Returns (traj [T, W, B], logdet [T, B], updated [T, B],
        n_updated [B] int32, ckpt_x [C, n, B], ckpt_P [C, rows, B]) with None for outputs not
        asked for; C = T // checkpoint_every, row c the filters after event (c + 1) *
        checkpoint_every - 1 (set_state(ckpt_x[c], ckpt_P[c]) and a sweep over the events after
        it continue the run bit for bit).

        ``consts``: noise constants per filter (kf_run_sweep_params), a [R, B] float64 table (R =
        consts_rows(model): q, r_imu, r_gps per state, filter index fastest) or a list of B
        kfmi.ref15.ModelConsts; filter f then runs under column f instead of the handle's
        constants (its P0 is the caller's set_state), and ``thresholds`` may be None: every filter
        always updates.  A table of another dtype or shape and a list of another length are
        KFError(KF_EINVAL)."""
        return self._sweep(etype, dt, payload, thresholds, traj, logdet, updated, counts, checkpoint_every, consts)[:6]

    def run_sweep_scores(self, etype, dt, payload, consts, thresholds=None, track=None, traj=False, logdet=False,
                         updated=False, checkpoint_every=0):
        """run_sweep(consts=...) that also scores every filter on the device (kf_run_sweep_scores):
        the same launch, the same records, counts, checkpoints, end state and status bit for bit,
        plus ``scores``, a [8, B] float64 tensor (rows: SCORE_ROWS) of the applied updates' count,
        NIS y^T S^-1 y and log det S per sensor, and the count and sum of squared position errors
        against ``track`` ([T, 3] float64, row t the reference position at event t, NaN rows not
        scored; None: rows 6 and 7 stay 0).  ``consts`` is mandatory (a table or a list of
        ModelConsts, as in run_sweep).  A filter that failed has NaN in its float rows.  Returns
        SweepScores(scores, n_updated, traj, logdet, updated, ckpt_x, ckpt_P), None where not asked
        for."""
        if consts is None:
            raise KFError(_lib.KF_EINVAL, 'run_sweep_scores: consts is mandatory (a table with equal columns scores '
                                          'a threshold sweep under one set)')
        tr, ld, up, nu, cx, cP, sc = self._sweep(etype, dt, payload, thresholds, traj, logdet, updated, True,
                                                 checkpoint_every, consts, scored=True, track=track)
        return SweepScores(sc, nu, tr, ld, up, cx, cP)

    def _sweep(self, etype, dt, payload, thresholds, traj, logdet, updated, counts, checkpoint_every, consts,
               scored=False, track=None):
        if self.model not in REF_MODELS:
            raise ValueError('run_sweep needs a ref15 or ref8 handle')
        tab = None
        if consts is not None:
            R = consts_rows(self.model)
            if isinstance(consts, (list, tuple)):
                if len(consts) != self.batch:
                    raise KFError(_lib.KF_EINVAL, f'consts: {len(consts)} constant sets for B = {self.batch} filters')
                consts = consts_table(self.model, consts)
            if isinstance(consts, np.ndarray):
                consts = torch.from_numpy(np.ascontiguousarray(consts))
            if not torch.is_tensor(consts):
                raise TypeError(f'consts: expected a tensor, an array or a list of ModelConsts, got {type(consts)}')
            if consts.dtype != torch.float64:
                raise KFError(_lib.KF_EINVAL, f'consts: dtype {consts.dtype} != torch.float64 (the table is float64 '
                                              f'for every handle dtype; the kernel converts)')
            if tuple(consts.shape) != (R, self.batch):
                raise KFError(_lib.KF_EINVAL, f'consts: shape {tuple(consts.shape)} != expected {(R, self.batch)} '
                                              f'([R, B], R = {R} rows for {self.model})')
            tab = self._dev(consts, (R, self.batch), 'consts', torch.float64)
        elif thresholds is None:
            raise ValueError('run_sweep: thresholds may be None only with consts')
        T = int(etype.shape[0])
        every = int(checkpoint_every)
        if every < 0:
            raise ValueError('checkpoint_every must be >= 0')
        trk = None
        if track is not None:
            if isinstance(track, np.ndarray):
                track = torch.from_numpy(np.ascontiguousarray(track))
            if not torch.is_tensor(track) or track.dtype != torch.float64 or tuple(track.shape) != (T, 3):
                raise KFError(_lib.KF_EINVAL, f'track: expected a float64 [T, 3] = {(T, 3)} array, got '
                                              f'{getattr(track, "dtype", type(track))} {tuple(getattr(track, "shape", ()))}')
            trk = self._dev(track, (T, 3), 'track', torch.float64)
        et = self._dev(etype.reshape(T), (T,), 'etype', torch.uint8)
        dtd = self._dev(dt.reshape(T), (T,), 'dt', torch.float64)
        pay = self._dev(payload.reshape(T, 9), (T, 9), 'payload')
        thr = self._dev(thresholds, (self.batch,), 'thresholds', torch.float64) if thresholds is not None else None
        tr = self.empty(T, TRAJ_WIDTH[self.model], self.batch) if traj else None
        ld = self.empty(T, self.batch) if logdet else None
        up = torch.empty(T, self.batch, dtype=torch.uint8, device=self.device) if updated else None
        nu = torch.zeros(self.batch, dtype=torch.int32, device=self.device) if counts else None
        sc = torch.empty(len(SCORE_ROWS), self.batch, dtype=torch.float64, device=self.device) if scored else None
        C = T // every if every > 0 else 0
        cx = self.empty(C, self.n, self.batch) if every > 0 else None
        cP = self.empty(C, self.ntri, self.batch) if every > 0 else None
        ck = (every, _ptr(cx) if C else None, _ptr(cP) if C else None, self._stream())
        if scored:
            check(_lib.lib().kf_run_sweep_scores(self.handle, T, _ptr(et), _ptr(dtd), _ptr(pay), _ptr(thr), _ptr(tab),
                                                 _ptr(trk), _ptr(sc), _ptr(tr), _ptr(ld), _ptr(up), _ptr(nu), *ck))
        elif tab is None:
            check(_lib.lib().kf_run_sweep(self.handle, T, _ptr(et), _ptr(dtd), _ptr(pay), _ptr(thr), _ptr(tr),
                                          _ptr(ld), _ptr(up), _ptr(nu), *ck))
        else:
            check(_lib.lib().kf_run_sweep_params(self.handle, T, _ptr(et), _ptr(dtd), _ptr(pay), _ptr(thr), _ptr(tab),
                                                 _ptr(tr), _ptr(ld), _ptr(up), _ptr(nu), *ck))
        return tr, ld, up, nu, cx, cP, sc

    def _consts_tab(self, consts):
        """run_sweep's ``consts`` (a [R, B] float64 table or a list of B ModelConsts) on the device."""
        R = consts_rows(self.model)
        if isinstance(consts, (list, tuple)):
            if len(consts) != self.batch:
                raise KFError(_lib.KF_EINVAL, f'consts: {len(consts)} constant sets for B = {self.batch} filters')
            consts = consts_table(self.model, consts)
        if isinstance(consts, np.ndarray):
            consts = torch.from_numpy(np.ascontiguousarray(consts))
        if not torch.is_tensor(consts) or consts.dtype != torch.float64 or tuple(consts.shape) != (R, self.batch):
            raise KFError(_lib.KF_EINVAL, f'consts: expected a float64 [R, B] = {(R, self.batch)} table or a list of '
                                          f'ModelConsts, got {getattr(consts, "dtype", type(consts))} '
                                          f'{tuple(getattr(consts, "shape", ()))}')
        return self._dev(consts, (R, self.batch), 'consts', torch.float64)

    def smooth_sweep(self, etype, dt, filt_x, filt_P, consts=None, x=True, P=False, traj=False, logdet=False,
                     inplace=False):
        """The RTS smoother over a sweep's filtered record (kf_smooth_sweep): etype [T] uint8 and dt
        [T] float64 as run_sweep took them, filt_x [T, n, B] and filt_P [T, rows, B] the ckpt_x /
        ckpt_P of run_sweep(checkpoint_every=1) (device tensors or arrays), ``consts`` as in
        run_sweep (None: the handle's constants; only the Q rates are read).  An f64 ref15 / ref8
        handle, whose state and status are not touched.  Returns SmoothedSweep(x [T, n, B], P [T,
        rows, B], traj [T, W, B], logdet [T, B], status [B] int32), None where not asked for; row
        T - 1 is the filtered row, and row t is row t + 1 wherever etype[t + 1] is NONE.
        ``inplace``: x and P (where asked for) overwrite filt_x / filt_P, which must then be device
        tensors.  A filter whose record is not positive definite (or holds a NaN) has NaN rows from
        there down to 0 and KF_ENOTSPD in ``status``."""
        if self.model not in REF_MODELS:
            raise ValueError('smooth_sweep needs a ref15 or ref8 handle')
        if self.dtype != 'f64':
            raise KFError(_lib.KF_EINVAL, 'smooth_sweep: needs an f64 handle')
        T = int(etype.shape[0])
        if inplace and not (torch.is_tensor(filt_x) and torch.is_tensor(filt_P) and filt_x.device == self.device
                            and filt_P.device == self.device and filt_x.is_contiguous() and filt_P.is_contiguous()):
            raise KFError(_lib.KF_EINVAL, 'smooth_sweep: inplace needs contiguous device tensors filt_x / filt_P')
        fx = self._dev(filt_x, (T, self.n, self.batch), 'filt_x')
        fP = self._dev(filt_P, (T, self.ntri, self.batch), 'filt_P')
        tab = self._consts_tab(consts) if consts is not None else None
        et = self._dev(etype.reshape(T), (T,), 'etype', torch.uint8)
        dtd = self._dev(dt.reshape(T), (T,), 'dt', torch.float64)
        sx = (fx if inplace else self.empty(T, self.n, self.batch)) if x else None
        sP = (fP if inplace else self.empty(T, self.ntri, self.batch)) if P else None
        tr = self.empty(T, TRAJ_WIDTH[self.model], self.batch) if traj else None
        ld = self.empty(T, self.batch) if logdet else None
        st = torch.zeros(self.batch, dtype=torch.int32, device=self.device)
        check(_lib.lib().kf_smooth_sweep(self.handle, T, _ptr(et), _ptr(dtd), _ptr(tab), _ptr(fx), _ptr(fP), _ptr(sx),
                                         _ptr(sP), _ptr(tr), _ptr(ld), _ptr(st), self._stream()))
        return SmoothedSweep(sx, sP, tr, ld, st)

    def smooth_sweep_em(self, etype, dt, payload, updated, filt_x, filt_P, consts=None, x=True, P=False, traj=False,
                        logdet=False, status=True, em=True, inplace=False):
        """smooth_sweep that also gathers the EM statistics for the diagonals of Q, R_imu and R_gps,
        per filter (kf_smooth_sweep_em).  etype, dt, filt_x, filt_P, consts, x, P, traj, logdet and
        inplace are smooth_sweep's, and those outputs are its bits; ``payload`` [T, 9] is run_sweep's
        and ``updated`` [T, B] uint8 the record that forward sweep wrote (both None: only the Q
        rows are gathered).  Returns SmoothedSweepEm(x, P, traj, logdet, status, em), None where not
        asked for; ``em`` is a [ROWS, B] float64 tensor (ref_em_rows(model): a count before each of
        the blocks Q [n], R_imu [n], R_gps [m]; event 0 starts the interval and is not counted),
        whose M-step is kfmi.ref_em_update.  A filter that failed has NaN in its float rows and
        keeps its counts."""
        if self.model not in REF_MODELS:
            raise ValueError('smooth_sweep_em needs a ref15 or ref8 handle')
        if self.dtype != 'f64':
            raise KFError(_lib.KF_EINVAL, 'smooth_sweep_em: needs an f64 handle')
        if (payload is None) != (updated is None):
            raise KFError(_lib.KF_EINVAL, 'smooth_sweep_em: payload and updated are given together or not at all')
        T = int(etype.shape[0])
        if inplace and not (torch.is_tensor(filt_x) and torch.is_tensor(filt_P) and filt_x.device == self.device
                            and filt_P.device == self.device and filt_x.is_contiguous() and filt_P.is_contiguous()):
            raise KFError(_lib.KF_EINVAL, 'smooth_sweep_em: inplace needs contiguous device tensors filt_x / filt_P')
        fx = self._dev(filt_x, (T, self.n, self.batch), 'filt_x')
        fP = self._dev(filt_P, (T, self.ntri, self.batch), 'filt_P')
        tab = self._consts_tab(consts) if consts is not None else None
        et = self._dev(etype.reshape(T), (T,), 'etype', torch.uint8)
        dtd = self._dev(dt.reshape(T), (T,), 'dt', torch.float64)
        pay = self._dev(payload.reshape(T, 9), (T, 9), 'payload') if payload is not None else None
        up = self._dev(updated, (T, self.batch), 'updated', torch.uint8) if updated is not None else None
        sx = (fx if inplace else self.empty(T, self.n, self.batch)) if x else None
        sP = (fP if inplace else self.empty(T, self.ntri, self.batch)) if P else None
        tr = self.empty(T, TRAJ_WIDTH[self.model], self.batch) if traj else None
        ld = self.empty(T, self.batch) if logdet else None
        st = torch.zeros(self.batch, dtype=torch.int32, device=self.device) if status else None
        tb = torch.empty(em_rows(self.model), self.batch, dtype=torch.float64, device=self.device) if em else None
        check(_lib.lib().kf_smooth_sweep_em(self.handle, T, _ptr(et), _ptr(dtd), _ptr(pay), _ptr(up), _ptr(tab),
                                            _ptr(fx), _ptr(fP), _ptr(sx), _ptr(sP), _ptr(tr), _ptr(ld), _ptr(st),
                                            _ptr(tb), self._stream()))
        return SmoothedSweepEm(sx, sP, tr, ld, st, tb)

    def run_tails(self, etype, dt, payload, lo, hi, thresholds, src_x=None, src_P=None, src_row=None, src_col=None,
                  counts=False):
        """Ragged tails of ONE event stream in one launch (kf_run_tails): etype [T] uint8, dt [T]
        float64, payload [T, 9]; filter f runs the events [lo[f], hi[f]) (host int arrays [B]) with
        run_sweep's event step against thresholds[f], from row src_row[f], column src_col[f] of
        src_x [R, n, Bs] / src_P [R, rows, Bs] (run_sweep's ckpt_x / ckpt_P as they are) or, with
        src_row[f] = -1 (the default for every tail), from its own state in the handle.  No
        records: the end states are state() / status().  Returns n_updated [B] int32 if ``counts``
        else None.  A wave carries 8 tails and runs to its longest: sort the tails by length."""
        if self.model not in REF_MODELS:
            raise ValueError('run_tails needs a ref15 or ref8 handle')
        T, B = int(etype.shape[0]), self.batch
        et = self._dev(etype.reshape(T), (T,), 'etype', torch.uint8)
        dtd = self._dev(dt.reshape(T), (T,), 'dt', torch.float64)
        pay = self._dev(payload.reshape(T, 9), (T, 9), 'payload')
        thr = self._dev(thresholds, (B,), 'thresholds', torch.float64)

        def host(a, name, fill):
            a = np.full(B, fill, np.int32) if a is None else np.ascontiguousarray(a, dtype=np.int32)
            if a.shape != (B,):
                raise ValueError(f'{name}: shape {a.shape} != expected {(B,)}')
            return a

        lo_h, hi_h = host(lo, 'lo', 0), host(hi, 'hi', 0)
        row_h, col_h = host(src_row, 'src_row', -1), host(src_col, 'src_col', 0)
        if (src_x is None) != (src_P is None):
            raise ValueError('give src_x and src_P together')
        R = Bs = 0
        sx = sP = None
        if src_x is not None:
            if (src_x.ndim != 3 or src_P.ndim != 3 or src_P.shape[0] != src_x.shape[0]
                    or src_P.shape[2] != src_x.shape[2]):
                raise ValueError(f'src_x {tuple(src_x.shape)} / src_P {tuple(src_P.shape)}: expected [R, n, Bs] / '
                                 f'[R, rows, Bs]')
            R, Bs = int(src_x.shape[0]), int(src_x.shape[2])
            sx = self._dev(src_x, (R, self.n, Bs), 'src_x')
            sP = self._dev(src_P, (R, self.ntri, Bs), 'src_P')
        nu = torch.zeros(B, dtype=torch.int32, device=self.device) if counts else None
        as_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        check(_lib.lib().kf_run_tails(self.handle, T, _ptr(et), _ptr(dtd), _ptr(pay), as_p(lo_h), as_p(hi_h), _ptr(thr),
                                      _ptr(sx) if R and Bs else None, _ptr(sP) if R and Bs else None, R, Bs,
                                      as_p(row_h), as_p(col_h), _ptr(nu), self._stream()))
        return nu

    def stream_check(self):
        """The checks of the last run_stream (kf_stream_check; synchronises the stream)."""
        out = (ctypes.c_double * 8)()
        check(_lib.lib().kf_stream_check(self.handle, out, self._stream()))
        return dict(ok=bool(out[0]), failed_chunk=bool(out[1]), cov_gap=out[2], state_gap=out[3],
                    chunks=int(out[4]), chunk=int(out[5]), warmup=int(out[6]),
                    fallback={0: None, 2: 'chain', 4: 'gated'}[int(out[7])])

    def eval_combos(self, events, init, prev_time, target_end, k, combo_offset=0, logdets=True):
        """KF_MODEL_REF15 brute force (kf_eval_combos): filter f evaluates combination
        combo_offset + f of k out of the n candidate events.  events: host [n, 11] float64
        (t, type, payload[9]); init: host [42] float64 (x[15], block-packed P[27]).
        Returns (max_logdet [B], logdets [k+2, B] or None, n_records [B] int32)."""
        if self.model != 'ref15':
            raise ValueError('eval_combos needs a ref15 handle')
        ev = np.ascontiguousarray(events, dtype=np.float64)
        ini = np.ascontiguousarray(init, dtype=np.float64)
        if ev.ndim != 2 or ev.shape[1] != 11 or ini.shape != (42,):
            raise ValueError('events must be [n, 11] and init [42]')
        mx = self.empty(self.batch)
        ld = self.empty(k + 2, self.batch) if logdets else None
        nr = torch.empty(self.batch, dtype=torch.int32, device=self.device)
        check(_lib.lib().kf_eval_combos(self.handle, ev.shape[0], ev.ctypes.data_as(ctypes.c_void_p),
                                        ini.ctypes.data_as(ctypes.c_void_p), float(prev_time), float(target_end),
                                        int(k), int(combo_offset), _ptr(ld), _ptr(mx), _ptr(nr), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()  # host arrays were staged; keep them alive
        return mx, ld, nr

    def search_combos(self, events, init, prev_time, target_end, threshold, k_max=None, exhaustive=False,
                      subset_max=False, n_fixed=0, fixed_mask=0):
        """KF_MODEL_REF15 brute-force search with shared prefixes (kf_search_combos): sizes
        k = 1 .. k_max of the n candidate events, each subset's filter advanced from its prefix's
        by one event.  Stops after the first size with a subset whose max log-det is below
        threshold unless ``exhaustive``.  ``n_fixed`` / ``fixed_mask`` restrict it to the subsets
        whose intersection with candidates 0 .. n_fixed - 1 is fixed_mask (one shard of the
        search).  Returns (k_found, winner indices tuple or None, accepted count per size
        [k_max + 1], subset_max [2^n] or None).  ``subset_max`` may be a device tensor of 2^n
        entries of the handle's dtype, which receives this search's subsets (untouched
        elsewhere: the classes of one search fill one buffer)."""
        if self.model != 'ref15':
            raise ValueError('search_combos needs a ref15 handle')
        ev = np.ascontiguousarray(events, dtype=np.float64)
        ini = np.ascontiguousarray(init, dtype=np.float64)
        if ev.ndim != 2 or ev.shape[1] != 11 or ini.shape != (42,):
            raise ValueError('events must be [n, 11] and init [42]')
        n = ev.shape[0]
        k_max = n if k_max is None else int(k_max)
        win = ctypes.c_uint64(0)
        kf = ctypes.c_int(0)
        acc = np.zeros(max(k_max, 0) + 1, dtype=np.uint64)
        if isinstance(subset_max, torch.Tensor):
            sm = subset_max
            if (sm.numel() != 1 << n or sm.dtype != self.torch_dtype or sm.device != self.device
                    or not sm.is_contiguous()):
                raise ValueError(f'subset_max must be a contiguous {self.torch_dtype} tensor of 2^{n} entries on '
                                 f'{self.device}')
        else:
            sm = self.empty(1 << n) if subset_max else None
            if sm is not None:
                sm.fill_(float('nan'))
        check(_lib.lib().kf_search_combos(self.handle, n, ev.ctypes.data_as(ctypes.c_void_p),
                                          ini.ctypes.data_as(ctypes.c_void_p), float(prev_time), float(target_end),
                                          float(threshold), k_max, int(bool(exhaustive)), int(n_fixed),
                                          int(fixed_mask), ctypes.byref(win),
                                          ctypes.byref(kf), acc.ctypes.data_as(ctypes.c_void_p), _ptr(sm),
                                          self._stream()))
        combo = tuple(i for i in range(n) if (win.value >> i) & 1) if kf.value else None
        return kf.value, combo, acc, sm

    def search_windows(self, events, init, prev_time, target_end, thresholds, k_max, n_events=None):
        """Many windows' brute-force searches in one launch (kf_search_windows; the handle's
        batch size is not used).  events: host [W, n_max, 11] float64 (t, type, payload[9]; rows
        past n_events[w] are not read), init [W, 42], prev_time / target_end / thresholds [W],
        n_events [W] (None: n_max everywhere).  Window w's result is search_combos(events[w,
        :n_events[w]], init[w], prev_time[w], target_end[w], thresholds[w], min(k_max,
        n_events[w]))'s.  Returns (k_found [W] int32, winner masks [W] uint64 (bit i = candidate
        i), accepted counts [W, k_max + 1] uint64); mask_indices(mask) lists a winner's
        candidates."""
        if self.model != 'ref15':
            raise ValueError('search_windows needs a ref15 handle')
        ev = np.ascontiguousarray(events, dtype=np.float64)
        if ev.ndim != 3 or ev.shape[2] != 11:
            raise ValueError('events must be [W, n_max, 11]')
        W, n_max = int(ev.shape[0]), int(ev.shape[1])
        ini = np.ascontiguousarray(init, dtype=np.float64)
        if ini.shape != (W, 42):
            raise ValueError('init must be [W, 42]')

        def per_window(a, dtype=np.float64):  # [W], a scalar standing for every window
            return np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=dtype), (W,)))

        pt, te, th = per_window(prev_time), per_window(target_end), per_window(thresholds)
        ne = per_window(n_max if n_events is None else n_events, np.int32)
        k_max = int(k_max)
        win = np.zeros(W, dtype=np.uint64)
        kf = np.zeros(W, dtype=np.int32)
        acc = np.zeros((W, max(k_max, 0) + 1), dtype=np.uint64)
        vp = ctypes.c_void_p
        check(_lib.lib().kf_search_windows(self.handle, W, n_max, ne.ctypes.data_as(vp), ev.ctypes.data_as(vp),
                                           ini.ctypes.data_as(vp), pt.ctypes.data_as(vp), te.ctypes.data_as(vp),
                                           th.ctypes.data_as(vp), k_max, win.ctypes.data_as(vp),
                                           kf.ctypes.data_as(vp), acc.ctypes.data_as(vp), self._stream()))
        return kf, win, acc

    def search_schedules(self, events, q_len, ref_pos, init, prev_time=float('nan'), fixed=(), metrics=False):
        """The per-window schedule search scored by position RMSE (kf_search_schedules; the
        handle's batch size is not used).  events: host [C, 11] float64 (t, type, payload[9]), the
        windows' queues one after another, q_len [W] their lengths; ref_pos [C, 3] the reference
        position at each candidate's time; init [42] (x, block-packed P); prev_time the time of
        init (NaN: the first pick's dt is 0).  ``fixed``: the digits of the first len(fixed)
        windows; the rest are searched.  ``metrics``: True for a new device tensor of the N_free
        metrics in itertools.product order, or a contiguous float64 device tensor of N_free
        entries to fill (a slice of one search's buffer).  Returns (best_rank or None, the
        winner's digits over all W windows or None, best_metric, n_valid, metrics or None)."""
        ev = np.ascontiguousarray(events, dtype=np.float64)
        ql = np.ascontiguousarray(q_len, dtype=np.int32)
        rp = np.ascontiguousarray(ref_pos, dtype=np.float64)
        ini = np.ascontiguousarray(init, dtype=np.float64)
        fx = np.ascontiguousarray(fixed, dtype=np.int32)
        if ql.ndim != 1 or fx.ndim != 1 or fx.size > ql.size:
            raise ValueError('q_len must be [W] and fixed at most W digits')
        C = int(ql.sum())
        if ev.shape != (C, 11) or rp.shape != (C, 3) or ini.shape != (42,):
            raise ValueError(f'events must be [{C}, 11], ref_pos [{C}, 3] and init [42]')
        W, nf = int(ql.size), int(fx.size)
        n_free = math.prod(int(q) for q in ql[nf:])
        if isinstance(metrics, torch.Tensor):
            mt = metrics
            if (mt.numel() != n_free or mt.dtype != torch.float64 or mt.device != self.device
                    or not mt.is_contiguous()):
                raise ValueError(f'metrics must be a contiguous float64 tensor of {n_free} entries on {self.device}')
        else:
            mt = torch.empty(n_free, dtype=torch.float64, device=self.device) if metrics and n_free < 1 << 40 else None
        rank, best, nv = ctypes.c_uint64(0), ctypes.c_double(0.0), ctypes.c_uint64(0)
        vp = ctypes.c_void_p
        check(_lib.lib().kf_search_schedules(self.handle, W, ql.ctypes.data_as(vp), ev.ctypes.data_as(vp),
                                             rp.ctypes.data_as(vp), ini.ctypes.data_as(vp), float(prev_time), nf,
                                             fx.ctypes.data_as(vp), ctypes.byref(rank), ctypes.byref(best),
                                             ctypes.byref(nv), _ptr(mt), self._stream()))
        if nv.value == 0:
            return None, None, float('inf'), 0, mt
        digits, r = [], rank.value
        for q in reversed(ql[nf:]):
            digits.append(r % int(q))
            r //= int(q)
        return rank.value, tuple(int(d) for d in fx) + tuple(reversed(digits)), best.value, nv.value, mt

    def schedule_plan(self, q_len, n_fixed=0):
        """How search_schedules would run these windows (kf_schedule_plan, no device work):
        dict(n_free (None: 2^40 schedules or more), widest, workspace_bytes)."""
        ql = np.ascontiguousarray(q_len, dtype=np.int32)
        out = np.zeros(3, dtype=np.int64)
        check(_lib.lib().kf_schedule_plan(self.handle, int(ql.size), ql.ctypes.data_as(ctypes.c_void_p), int(n_fixed),
                                          out.ctypes.data_as(ctypes.c_void_p)))
        return {'n_free': None if out[0] < 0 else int(out[0]), 'widest': int(out[1]), 'workspace_bytes': int(out[2])}

    def search_plan(self, init, n, k_max=None, n_fixed=0, fixed_mask=0):
        """How search_combos would run over n candidates (kf_search_plan, no device work):
        dict(sym, workspace_bytes, widest, max_parents, over_cap)."""
        if self.model != 'ref15':
            raise ValueError('search_plan needs a ref15 handle')
        ini = np.ascontiguousarray(init, dtype=np.float64)
        if ini.shape != (42,):
            raise ValueError('init must be [42]')
        out = np.zeros(5, dtype=np.int64)
        check(_lib.lib().kf_search_plan(self.handle, int(n), ini.ctypes.data_as(ctypes.c_void_p), int(n_fixed),
                                        int(fixed_mask), int(n if k_max is None else k_max),
                                        out.ctypes.data_as(ctypes.c_void_p)))
        return {'sym': bool(out[0]), 'workspace_bytes': int(out[1]), 'widest': int(out[2]),
                'max_parents': int(out[3]), 'over_cap': int(out[4])}

    def search_info(self):
        """How the last search_combos ran (kf_search_info): axis-symmetric or not, the sizes its
        head launch covered, its level launches after the head, the bytes of one level buffer."""
        out = np.zeros(4, dtype=np.int64)
        check(_lib.lib().kf_search_info(self.handle, out.ctypes.data_as(ctypes.c_void_p)))
        return {'sym': bool(out[0]), 'head_sizes': int(out[1]), 'level_launches': int(out[2]),
                'level_bytes': int(out[3])}

    def score_candidates(self, types, full=False, posterior=False):
        """KF_MODEL_REF15 scheduler scoring (kf_score_candidates): [len(types), B] traces of the
        posterior covariance each candidate sensor would give (full=False: the reference's
        Scheduler.gain, first measurement row only).  posterior=True also returns the
        block-packed posterior covariances [len(types), 27, B] (Scheduler.cov_matrix)."""
        if self.model != 'ref15':
            raise ValueError('score_candidates needs a ref15 handle')
        ty = np.ascontiguousarray(types, dtype=np.int32)
        out = self.empty(len(ty), self.batch)
        post = self.empty(len(ty), 27, self.batch) if posterior else None
        check(_lib.lib().kf_score_candidates(self.handle, len(ty), ty.ctypes.data_as(ctypes.c_void_p), int(full),
                                             _ptr(out), _ptr(post), self._stream()))
        return (out, post) if posterior else out

    def score_rows(self, types, row_masks, posterior=False):
        """KF_MODEL_REF15 Scheduler.cov_matrix for any measurement rows (kf_score_rows):
        candidate c is sensor types[c] updated with the rows of row_masks[c] (bit i = 1-based row
        i + 1 of its H).  Returns gain [n, B] (posterior traces) and, with posterior=True, the
        block-packed posteriors [n, 27, B]."""
        if self.model != 'ref15':
            raise ValueError('score_rows needs a ref15 handle')
        ty = np.ascontiguousarray(types, dtype=np.int32)
        mk = np.ascontiguousarray(row_masks, dtype=np.uint32)
        if ty.shape != mk.shape or ty.ndim != 1:
            raise ValueError('score_rows: types and row_masks must be 1-D of one length')
        out = self.empty(len(ty), self.batch)
        post = self.empty(len(ty), 27, self.batch) if posterior else None
        check(_lib.lib().kf_score_rows(self.handle, len(ty), ty.ctypes.data_as(ctypes.c_void_p),
                                       mk.ctypes.data_as(ctypes.c_void_p), _ptr(out), _ptr(post), self._stream()))
        return (out, post) if posterior else out

    def run_scheduled(self, t, etype, payload, prev_time, freq, records=False):
        """KF_MODEL_REF15 rate-decimated greedy filter (kf_run_scheduled).  t [T, B] float64
        absolute times, etype [T, B] uint8, payload [T, 9, B] — or, with records=True, one record
        per event [T, B, rec] (rec >= 9, rec * element size a multiple of 16 B: kf_run_scheduled_rec)
        — prev_time [B] float64, freq scalar or [B] float64 (a sampling sweep in one launch).
        Returns (traj [T, 6, B], logdet [T, B], sel_time [T, B], n_sel [B]) with the first n_sel[f]
        rows of filter f valid."""
        if self.model != 'ref15':
            raise ValueError('run_scheduled needs a ref15 handle')
        T = int(t.shape[0])
        td = self._dev(t, (T, self.batch), 't', torch.float64)
        et = self._dev(etype, (T, self.batch), 'etype', torch.uint8)
        rec = int(payload.shape[2]) if records else 0
        pay = self._dev(payload, (T, self.batch, rec) if records else (T, 9, self.batch), 'payload')
        pv = self._dev(prev_time, (self.batch,), 'prev_time', torch.float64)
        fr = None
        if np.ndim(freq) != 0:
            fr = self._dev(freq, (self.batch,), 'freq', torch.float64)
        tr = self.empty(max(T, 1), 6, self.batch)
        ld = self.empty(max(T, 1), self.batch)
        stt = torch.empty(max(T, 1), self.batch, dtype=torch.float64, device=self.device)
        ns = torch.empty(self.batch, dtype=torch.int32, device=self.device)
        fa = float(freq) if fr is None else 0.0
        if records:
            check(_lib.lib().kf_run_scheduled_rec(self.handle, T, _ptr(td), _ptr(et), _ptr(pay), rec, _ptr(pv),
                                                  _ptr(fr), fa, _ptr(tr), _ptr(ld), _ptr(stt), _ptr(ns),
                                                  self._stream()))
        else:
            check(_lib.lib().kf_run_scheduled(self.handle, T, _ptr(td), _ptr(et), _ptr(pay), _ptr(pv), _ptr(fr),
                                              fa, _ptr(tr), _ptr(ld), _ptr(stt), _ptr(ns), self._stream()))
        return tr, ld, stt, ns

    def run_scheduled_random(self, t, etype, payload, prev_time, freq, words, records=False):
        """KF_MODEL_REF15 random-selection scheduled filter (kf_run_scheduled_random): the
        windows of run_scheduled, each pick np.random.choice(len(queue)) drawn on the device from
        ``words`` [n_words, B] uint32 — column f the raw 32-bit generator outputs filter f
        consumes, in order (see kfmi.ref15.legacy_words).  Returns (traj, logdet, sel_time, n_sel,
        words_used [B] int32: outputs taken, -1 if a column ran out)."""
        if self.model != 'ref15':
            raise ValueError('run_scheduled_random needs a ref15 handle')
        T = int(t.shape[0])
        td = self._dev(t, (T, self.batch), 't', torch.float64)
        et = self._dev(etype, (T, self.batch), 'etype', torch.uint8)
        rec = int(payload.shape[2]) if records else 0
        pay = self._dev(payload, (T, self.batch, rec) if records else (T, 9, self.batch), 'payload')
        pv = self._dev(prev_time, (self.batch,), 'prev_time', torch.float64)
        W = int(words.shape[0])
        if isinstance(words, np.ndarray):
            words = np.ascontiguousarray(words, np.uint32).view(np.int32)
        elif words.dtype == torch.uint32:
            words = words.view(torch.int32)
        wd = self._dev(words, (W, self.batch), 'words', torch.int32)  # the bits of the uint32 outputs
        fr = None
        if np.ndim(freq) != 0:
            fr = self._dev(freq, (self.batch,), 'freq', torch.float64)
        tr = self.empty(max(T, 1), 6, self.batch)
        ld = self.empty(max(T, 1), self.batch)
        stt = torch.empty(max(T, 1), self.batch, dtype=torch.float64, device=self.device)
        ns = torch.empty(self.batch, dtype=torch.int32, device=self.device)
        used = torch.empty(self.batch, dtype=torch.int32, device=self.device)
        check(_lib.lib().kf_run_scheduled_random(self.handle, T, _ptr(td), _ptr(et), _ptr(pay), rec, _ptr(pv), _ptr(fr),
                                                 float(freq) if fr is None else 0.0, _ptr(wd), W, _ptr(used),
                                                 _ptr(tr), _ptr(ld), _ptr(stt), _ptr(ns), self._stream()))
        return tr, ld, stt, ns, used

    def sched_random_picks(self, t, etype, prev_time, freq, words):
        """The random arm's picks alone (kf_sched_random_picks): t [T, B], etype [T, B],
        prev_time [B], freq scalar or [B], words [n_words, B] uint32.  Returns (pick [T, B] int32
        event indices, sel_time [T, B], n_sel [B], words_used [B]); run the picked events with
        run_events."""
        T = int(t.shape[0])
        td = self._dev(t, (T, self.batch), 't', torch.float64)
        et = self._dev(etype, (T, self.batch), 'etype', torch.uint8)
        pv = self._dev(prev_time, (self.batch,), 'prev_time', torch.float64)
        W = int(words.shape[0])
        if isinstance(words, np.ndarray):
            words = np.ascontiguousarray(words, np.uint32).view(np.int32)
        elif words.dtype == torch.uint32:
            words = words.view(torch.int32)
        wd = self._dev(words, (W, self.batch), 'words', torch.int32)
        fr = None
        if np.ndim(freq) != 0:
            fr = self._dev(freq, (self.batch,), 'freq', torch.float64)
        pick = torch.empty(max(T, 1), self.batch, dtype=torch.int32, device=self.device)
        stt = torch.empty(max(T, 1), self.batch, dtype=torch.float64, device=self.device)
        ns = torch.empty(self.batch, dtype=torch.int32, device=self.device)
        used = torch.empty(self.batch, dtype=torch.int32, device=self.device)
        check(_lib.lib().kf_sched_random_picks(self.handle, T, _ptr(td), _ptr(et), _ptr(pv), _ptr(fr),
                                               float(freq) if fr is None else 0.0, _ptr(wd), W, _ptr(used),
                                               _ptr(pick), _ptr(stt), _ptr(ns), self._stream()))
        return pick, stt, ns, used

    # -- synthetic streams -----------------------------------------------
    def synth(self, T, dt, update_every=1, seed=20251015, filter_offset=0):
        """Deterministic synthetic (x0 [n,B], u [T,c,B], z [U,m,B]) generated on the GPU."""
        U = T // update_every
        x0 = self.empty(self.n, self.batch)
        u = self.empty(T, self.c, self.batch)
        z = self.empty(max(U, 0), self.m, self.batch)
        check(_lib.lib().kf_synth(self.handle, int(seed), int(filter_offset), int(T), float(dt),
                                  int(update_every), _ptr(x0), _ptr(u), _ptr(z), self._stream()))
        return x0, u, z
