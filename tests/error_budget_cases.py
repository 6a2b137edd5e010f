"""The fixed inputs of the error-budget tests and, cached, their truth and reference errors.

``test_gpu_error_budget.py`` runs the kernels on these inputs; ``test_extended_oracle_cpu.py``
asserts, for the very same inputs, that the budgets they produce stay under the caps of the
regime table — so nobody loosens the GPU test by changing a seed or a shape here.

Regimes (per-filter streams, first event a GPS fix at dt = 0, etype drawn from [0, 1, 1, 1]):
A  benign: dt in U(0, 0.02) with exact zeros, a few PREDICT events, trailing NONE events;
B  as A with one 20 s gap mid-stream (even filters meet a GPS event there, odd ones an IMU event);
C  as A with one 100 s gap before a GPS event (fp64 only);
D  as A with one 300 s gap before an IMU event (fp64 only; the reference's (I - K H) P cancels).
W  as A on tracks that start within +-500 m (fp32 only: small components under positions of up to
   600 m, where an fp32 position has an ulp of 3e-5 to 6e-5 m; at +-800 m the velocity budget is 1.07e-4).
"""
import functools
import zlib

import numpy as np

import extended_oracle as xo

B = 70                                   # one full wave plus a ragged one; nine 8-lane groups
SEGMENT = 8                              # events per launch between two kf.state() reads
# T, gap length, gap position (never on a segment boundary), the event type at the gap
REGIMES = {'A': (96, None, None, None), 'B': (90, 20.0, 45, 'mixed'), 'C': (64, 100.0, 37, 'gps'),
           'D': (72, 300.0, 43, 'imu'), 'W': (96, None, None, None)}
TRACK_SPAN = {'W': 500.0}                # half-width of the tracks' starting box in metres; 150 elsewhere
# caps on the budget over scale (fp64, fp32); None: that regime is not run in that dtype
CAPS = {'A': (1e-9, 1e-4), 'B': (1e-9, 1e-4), 'C': (1e-7, None), 'D': (None, None), 'W': (None, 1e-4)}
FACTOR = {'A': 8.0, 'B': 8.0, 'C': 8.0, 'D': 1.0, 'W': 8.0}
CV_T, CV_GAP_AT = 64, 29
UTM_OFFSET = np.array([5e5, 4e6, 100.0])  # raw-UTM-size easting, northing, altitude
STREAM_T, STREAM_CHUNK, STREAM_GAP_AT = 3000, 256, 1408  # the gap in the middle of chunk 5


def custom_constants(model, seed):
    """Caller constants with the ranges of test_gpu_constants._custom, as ref_kf's K dict."""
    rng = np.random.default_rng(seed)
    n, g = (15, 3) if model == 'ref15' else (8, 2)
    return dict(q=rng.uniform(0.01, 8.0, n), r_imu=rng.uniform(0.02, 120.0, n), r_gps=rng.uniform(0.5, 9.0, g),
                p0=rng.uniform(20.0, 2e4, n))


def _seed(*parts):
    return zlib.crc32('/'.join(map(str, parts)).encode())


def _payloads(rng, etype, dt, nB, span=150.0):
    """Fixes along a per-filter track and IMU samples around it.  The tracks start within
    +-150 m and drift by up to ~100 m: an fp32 filter's velocity error is ulp(position) over its
    memory, and a 20 s gap multiplies it by 20 s, so at +-800 m the plain fp32 reference's own
    error (vel 3.0e-5, pos 2.7e-5 over scale) would put the regime-B budget above its 1e-4 cap.
    Regime W runs the benign stream on +-500 m tracks, where the cap still holds; raw-UTM-size
    coordinates are the cv route's offset runs."""
    T = etype.shape[0]
    t = np.cumsum(dt, axis=0)
    p0 = rng.uniform(-span, span, (3, nB))
    v = rng.normal(0.0, 5.0, (3, nB))
    pay = np.zeros((T, 9, nB))
    fix = p0[None] + v[None] * t[:, None, :] + rng.normal(0, 1.5, (T, 3, nB))
    imu = np.concatenate([rng.normal(0, 0.05, (T, 3, nB)) + np.cumsum(rng.normal(0, 2e-3, (T, 3, nB)), 0),
                          rng.normal(0, 0.02, (T, 3, nB)), rng.normal(0, 0.4, (T, 3, nB))], axis=1)
    g, i = (etype == xo.GPS)[:, None, :], (etype == xo.IMU)[:, None, :]
    pay[:, 0:3] = np.where(g, fix, pay[:, 0:3])
    pay = np.where(i, imu, pay)
    return pay


@functools.lru_cache(maxsize=None)
def event_case(model, regime, custom=False):
    """The inputs of one (model, regime, constants) case: dict(etype [T, B], dt [T, B], pay
    [T, 9, B], x0 [B, n], P0 [n, n], K)."""
    T, gap, at, kind = REGIMES[regime]
    rng = np.random.default_rng(_seed('events', model, regime, custom))
    n = 15 if model == 'ref15' else 8
    etype = rng.choice([0, 1, 1, 1], size=(T, B)).astype(np.uint8)
    etype[rng.random((T, B)) < 0.03] = xo.PREDICT
    etype[0] = xo.GPS
    etype[T - 6:, ::5] = xo.NONE
    dt = rng.uniform(0.0, 0.02, (T, B))
    dt[rng.random((T, B)) < 0.05] = 0.0
    dt[0] = 0.0
    if gap is not None:
        dt[at] = gap
        etype[at] = {'gps': xo.GPS, 'imu': xo.IMU}.get(kind, xo.GPS)
        if kind == 'mixed':
            etype[at, 1::2] = xo.IMU
    pay = _payloads(rng, etype, dt, B, TRACK_SPAN.get(regime, 150.0))
    x0 = rng.normal(0.0, 0.1, (B, n))
    m = 3 if model == 'ref15' else 2
    x0[:, :m] = pay[0, :m].T
    K = custom_constants(model, _seed('consts', model)) if custom else None
    return dict(etype=etype, dt=dt, pay=pay, x0=x0, P0=xo.Model(model, K).P0(), K=K)


@functools.lru_cache(maxsize=None)
def event_reference(model, regime, custom, dtype):
    """(truth, E_ref) of an event case in the kernel's dtype: the longdouble filter on the
    rounded inputs, and the plain same-precision reference's errors against it."""
    c = event_case(model, regime, custom)
    args = (c['x0'], c['P0'], c['etype'], c['dt'], c['pay'])
    truth = xo.run_truth(model, *args, K=c['K'], dtype=dtype)
    plain = xo.plain_f64(model, *args, K=c['K']) if dtype == 'f64' else xo.run_plain_f32(model, *args, K=c['K'])
    return truth, xo.errors(plain, truth, xo.Model(model).groups)


@functools.lru_cache(maxsize=None)
def cv_case(model, regime, update_every, offset):
    """dict(x0 [B, n], dt_steps [T], u [T, d, B], z [T // k, d, B]); ``offset``: x0 and the
    fixes moved by raw-UTM-size coordinates."""
    d = 2 if model == 'cv2' else 3
    rng = np.random.default_rng(_seed('cv', model, regime, update_every, offset))
    T, k = CV_T, update_every
    dt_steps = np.full(T, 0.1)
    if regime == 'B':
        dt_steps[CV_GAP_AT] = 20.0
    p0 = rng.uniform(-200, 200, (B, d)) + (UTM_OFFSET[:d] if offset else 0.0)
    v = rng.normal(0, 3.0, (B, d))
    x0 = np.zeros((B, 2 * d))
    x0[:, :d] = p0 + rng.normal(0, np.sqrt(3), (B, d))
    u = rng.normal(0, 0.3, (T, d, B))
    t_fix = np.cumsum(dt_steps)[k - 1::k][:T // k]
    z = p0.T[None] + v.T[None] * t_fix[:, None, None] + rng.normal(0, np.sqrt(3), (T // k, d, B))
    return dict(x0=x0, dt_steps=dt_steps, u=u, z=z)


@functools.lru_cache(maxsize=None)
def cv_reference(model, regime, update_every, offset, dtype):
    c = cv_case(model, regime, update_every, offset)
    M = xo.Model(model)
    etype, dt, pay = xo.cv_events(model, CV_T, B, c['dt_steps'], c['z'], update_every)
    truth = xo.run_truth(model, c['x0'], M.P0(), etype, dt, pay, u=c['u'], dtype=dtype)
    if dtype == 'f64':
        plain = xo.plain_f64_cv(model, c['x0'], c['dt_steps'], c['u'], c['z'], update_every)
    else:
        plain = xo.run_plain_f32(model, c['x0'], M.P0(), etype, dt, pay, u=c['u'])
    return truth, xo.errors(plain, truth, M.groups)


@functools.lru_cache(maxsize=None)
def stream_case(model):
    """One long stream per regime (A, B), as the two filters of one batch: 200 Hz IMU with 10 Hz
    fixes along a drive; filter 1 has the 20 s gap before an IMU event in the middle of a chunk."""
    T = STREAM_T
    rng = np.random.default_rng(_seed('stream', model))
    et = np.ones(T, np.uint8)
    et[::20] = xo.GPS
    et[rng.choice(np.arange(1, T), 12, replace=False)] = xo.NONE
    etype = np.stack([et, et], axis=1)
    dt = np.full((T, 2), 0.005)
    dt[0] = 0.0
    dt[STREAM_GAP_AT, 1] = 20.0
    etype[STREAM_GAP_AT, 1] = xo.IMU
    pay = _payloads(rng, etype, dt, 2)
    n = 15 if model == 'ref15' else 8
    x0 = np.zeros((2, n))
    m = 3 if model == 'ref15' else 2
    x0[:, :m] = pay[0, :m].T
    return dict(etype=etype, dt=dt, pay=pay, x0=x0, P0=xo.Model(model).P0(), K=None)


@functools.lru_cache(maxsize=None)
def stream_reference(model):
    """(truth, {regime: E_ref}) over the same 3000 events, both regimes in one oracle run."""
    c = stream_case(model)
    args = (c['x0'], c['P0'], c['etype'], c['dt'], c['pay'])
    truth = xo.run_truth(model, *args)
    plain = xo.plain_f64(model, *args)
    groups = xo.Model(model).groups
    return truth, {r: xo.errors(one_filter(plain, f), one_filter(truth, f), groups) for f, r in enumerate('AB')}


def one_filter(res, f):
    return {k: (v[:, f:f + 1] if k in ('x', 'P', 'logdet') else v) for k, v in res.items()}


def report(route, regime, dtype, e_gpu, e_ref, budget):
    """One line per group — the measured-value table — and the groups over budget."""
    over = {}
    for k, b in budget.items():
        ratio = e_gpu[k] / e_ref[k] if e_ref[k] > 0 else float('inf') if e_gpu[k] > 0 else 0.0
        print(f'error-budget | {route} | {regime} | {dtype} | {k} | E_gpu {e_gpu[k]:.3e} | E_ref {e_ref[k]:.3e} | '
              f'ratio {ratio:.3g} | budget {b:.3e}')
        if not e_gpu[k] <= b:
            over[k] = (e_gpu[k], b)
    return over
