"""The gated (adaptive-threshold) one-filter run of a long stream against the dense NumPy oracle
(tests/gated_oracle.py over oracle/ref_kf.py's matrices): kf_run_events' chunked route with its
seam check and both sequential fallbacks, the look-ahead kernel and the chain kernel themselves,
and the façade's list driver — needs an MI355X.

Every other test of this machinery takes the sequential chain kernel as the truth; here the truth
is the reference's arithmetic in fp64, so a gate that drifts from slogdet over tens of thousands
of events, or error that grows with the run, fails.

The margin rule (tests/test_gpu_sweep.py).  One flipped gate changes every later record, so a
threshold is compared only where the oracle itself is not on the fence: every test first asserts
that the smallest |logdet(P_pred) - threshold| of the oracle's own run is >= 1e-5, a condition on
the inputs.  The thresholds below were fixed in advance with margins of 6.8e-4 and more; none may
be excluded.  (-25, -30 and median + 0.5 / 1.0 / 2.0 of test_gpu_timeparallel.py have margins of
2e-7 to 4e-6 on this stream and are not used against the oracle.)

Each comparison prints one row (route, update share, margin, worst relative differences); the
module prints them as a table at its end (pytest -s).
"""
import numpy as np
import pytest
import torch

import gated_oracle
import kfmi
import test_gpu_sweep as tsw
import test_gpu_timeparallel as ttp
from kfmi import _lib, ingest, ref15
from oracle import ref_kf

pytestmark = pytest.mark.gpu
TOL = 1e-6             # against the oracle (north_star, fp64), _rel's normalisation by max(|ref|, 1)
MARGIN = tsw.MARGIN['f64']
T_LONG = 70000         # the smallest length the suite uses above kf_run_events' 65,536-event route threshold
REF15_THR = [-36.60, -36.20, -31.65, -25.65, -15.15, -10.65, 50.0]
REF8_THR = [-8.00, 0.00]
F32_THR = [-36.45, -36.40, -36.25, -36.20, -36.15, -36.00]
_rel = tsw._rel
_once = tsw._once
_ROWS = []


@pytest.fixture(scope='module', autouse=True)
def _table():
    yield
    print('\n| case | model | threshold | route | updated | margin | traj | logdet | cov | final |')
    print('|---|---|---|---|---|---|---|---|---|---|')
    for row in _ROWS:
        print(row)


# ---------------------------------------------------------------------------------------------
# inputs and oracle runs (computed once, never modified)
# ---------------------------------------------------------------------------------------------
def _long():
    return _once('gated_oracle_long', lambda: ttp._stream(T_LONG, seed=11))


def _dense_start(model, x0, K=None):
    """The oracle's start: the first fix in the leading states, the model's (or K's) P0."""
    n, k = (15, 3) if model == 'ref15' else (8, 2)
    xs = np.zeros(n)
    xs[0:k] = np.asarray(x0)[0:k]
    P0 = np.diag(np.asarray(K['p0'], np.float64)[:n]) if K is not None else \
        (ref_kf.P0_REF15 if model == 'ref15' else ref_kf.P0_REF8)
    return xs, np.array(P0, dtype=np.float64)


def _oracle(key, model, stream, thr, K=None):
    """run_gated once per (stream, model, threshold).  Its [T, n, n] covariance records are kept
    as the entries that are non-zero anywhere in the run (the rest are exactly 0.0: lossless)."""
    def run():
        et, dt, pay, x0 = stream
        xs, P0 = _dense_start(model, x0, K)
        r = gated_oracle.run_gated(model, et, dt, pay, xs, P0, thr, K=K, cov=True)
        support = (r.cov != 0).any(0)
        return r._replace(cov=None), support, np.ascontiguousarray(r.cov[:, support])
    return _once(('gated_oracle', key, model, thr), run)


def _device(model, stream, thr, dtype='f64', kernel=None, sequential=False, params=None):
    """One filter from the first fix and the model's P0 through kf_run_events(_seq) with every
    record.  Returns a dict of NumPy arrays in the handle's dtype (traj [T, W], logdet [T], updated
    [T], cov [T, rows], x [n], P [rows]), status, and chk: stream_check(), or None where the handle
    has run no kf_run_stream."""
    et, dt, pay, x0 = stream
    kf = tsw._handle(model, 1, dtype, params, x0, options={'events_kernel': kernel} if kernel else None)
    try:
        npd = np.float64 if dtype == 'f64' else np.float32
        tr, ld, up, cv = kf.run_events(et[:, None], dt[:, None], pay[:, :, None].astype(npd), updated=True, cov=True,
                                       threshold=thr, sequential=sequential)
        x, P = kf.state()
        out = dict(traj=tr[:, :, 0], logdet=ld[:, 0], updated=up[:, 0], cov=cv[:, :, 0], x=x[:, 0], P=P[:, 0])
        out = {k: v.cpu().numpy() for k, v in out.items()}
        out['status'] = int(kf.status().sum().item())
        try:
            out['chk'] = kf.stream_check()
        except kfmi.KFError:
            out['chk'] = None
        return out
    finally:
        kf.close()


def _route(chk):
    return 'stands' if chk['ok'] else chk['fallback']


def _compare(case, model, stream, dev, orc, thr, route, K=None, tol=TOL):
    """Flags equal the oracle's exactly; trajectory, log-det and covariance records (through
    from_blocks) and the final state and covariance within ``tol``.  The margin is asserted first."""
    r, support, packed = orc
    et, dt, pay, x0 = stream
    assert r.margin >= MARGIN, (case, model, thr, r.margin)
    assert dev['status'] == 0, (case, model, thr)
    if not np.array_equal(dev['updated'], r.updated):
        i = int(np.argmax(dev['updated'] != r.updated))
        P_prev = ref15.from_blocks(dev['cov'][i - 1].astype(np.float64)) if i else _dense_start(model, x0, K)[1]
        pytest.fail(f'{case} {model} threshold {thr}: {int((dev["updated"] != r.updated).sum())} flags differ, the '
                    f'first at event {i} (device {dev["updated"][i]}, oracle {r.updated[i]}): logdet(P_pred) from '
                    f'the device\'s covariance {gated_oracle.predicted_logdet(model, P_prev, dt[i], K)!r}, the '
                    f'oracle\'s {r.gate[i]!r}; oracle margin {r.margin:.3g}')
    dense = ref15.from_blocks(dev['cov'])
    outside = float(np.abs(dense[:, ~support]).max()) if (~support).any() else 0.0
    errs = dict(traj=_rel(dev['traj'], r.traj), logdet=_rel(dev['logdet'], r.logdet),
                cov=max(_rel(dense[:, support], packed), outside),
                final=max(_rel(dev['x'], r.x), _rel(ref15.from_blocks(dev['P']), r.P)))
    row = (f'| {case} | {model} | {thr:g} | {route} | {100 * r.updated.mean():.2f} % | {r.margin:.1e} | '
           + ' | '.join(f'{errs[k]:.1e}' for k in ('traj', 'logdet', 'cov', 'final')) + ' |')
    _ROWS.append(row)
    print(row)
    for k, v in errs.items():
        assert v <= tol, (case, model, thr, k, v)


# ---------------------------------------------------------------------------------------------
# (a) kf_run_events' own route
# ---------------------------------------------------------------------------------------------
_ROUTES = {}


def _route_run(model, thr):
    """The default-option run through the route, compared with the oracle; its route is kept."""
    if (model, thr) not in _ROUTES:
        dev = _device(model, _long(), thr)
        chk = dev['chk']
        assert chk is not None and chk['chunks'] > 1 and chk['warmup'] == 2048, chk
        _ROUTES[model, thr] = _route(chk)
        _compare('route', model, _long(), dev, _oracle('long', model, _long(), thr), thr, _ROUTES[model, thr])
    return _ROUTES[model, thr]


@pytest.mark.parametrize('model,thr', [('ref15', t) for t in REF15_THR] + [('ref8', t) for t in REF8_THR])
def test_gated_route_vs_oracle(model, thr):
    """kf_run_events on a one-filter f64 handle with default options over 70,000 events (the
    chunked route: chunk starts from 2,048 events of gated warm-up, the seam check, the fallback
    chosen on the device) against the oracle: flags exactly, every record and the final state
    within 1e-6.  Margins and update shares from the oracle's runs (CPU), routes as measured:

    | model | threshold | margin | updated | route |
    |---|---|---|---|---|
    | ref15 | -36.60 | 7.5e-2 | 100 % | chunked records stand |
    | ref15 | -36.20 | 1.5e-2 | 96.5 % | chunked records stand |
    | ref15 | -31.65 | 1.1e-3 | 55 % | chain fallback |
    | ref15 | -25.65 | 8.4e-3 | 25 % | chain fallback |
    | ref15 | -15.15 | 1.5e-3 | 6.3 % | look-ahead fallback |
    | ref15 | -10.65 | 2.1e-3 | 3.6 % | look-ahead fallback |
    | ref15 | 50.0 | 1.05e-3 | 0.06 % | look-ahead fallback |
    | ref8 | -8.00 | 6.8e-4 | 25 % | chain fallback |
    | ref8 | 0.00 | 7.4e-4 | 3.4 % | look-ahead fallback |

    On a flag mismatch the message carries the first differing event, logdet(P_pred) there from
    the device's covariance record and from the oracle, and the oracle's margin."""
    _route_run(model, thr)


def test_gated_route_coverage():
    """What the thresholds are for: over the seven ref15 thresholds the route reports the chunked
    records standing, the chain fallback and the look-ahead fallback at least once each; over the
    two ref8 thresholds both fallbacks."""
    r15 = {_route_run('ref15', t) for t in REF15_THR}
    r8 = {_route_run('ref8', t) for t in REF8_THR}
    assert {'stands', 'chain', 'gated'} <= r15, r15
    assert {'chain', 'gated'} <= r8, r8


# ---------------------------------------------------------------------------------------------
# (b), (c) the two sequential kernels themselves
# ---------------------------------------------------------------------------------------------
def _stream4():
    return tsw._stream4()


@pytest.mark.parametrize('thr', tsw.STREAM4_THR)
def test_lookahead_kernel_vs_oracle(thr):
    """events_kernel = 'gated' (KF_OPT_EVENTS_KERNEL = 4) with sequential=True, no route, on
    stream 4 (5,000 events, 300 of them NONE inside the look-ahead) at every STREAM4_THR value
    (margins >= 4e-5: none may be excluded), against the oracle."""
    dev = _device('ref15', _stream4(), thr, kernel='gated', sequential=True)
    assert dev['chk'] is None
    _compare('look-ahead s4', 'ref15', _stream4(), dev, _oracle('stream4', 'ref15', _stream4(), thr), thr, '-')


@pytest.mark.parametrize('thr', [-10.65, -15.15])
def test_lookahead_kernel_long_vs_oracle(thr):
    """The look-ahead kernel over the 70,000-event stream at the two thresholds where the route
    picks it, against (a)'s oracle runs."""
    dev = _device('ref15', _long(), thr, kernel='gated', sequential=True)
    assert dev['chk'] is None
    _compare('look-ahead', 'ref15', _long(), dev, _oracle('long', 'ref15', _long(), thr), thr, '-')


def _oracle_consts(model, params):
    n, g = (15, 3) if model == 'ref15' else (8, 2)
    return dict(q=np.array(params.ref_q[:n]), r_imu=np.array(params.ref_r_imu[:n]),
                r_gps=np.array(params.ref_r_gps[:g]), p0=np.array(params.ref_p0[:n]))


@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_lookahead_kernel_custom_constants_vs_oracle(model):
    """The look-ahead kernel's CUSTOM instantiation (Q, R, P0 from the handle) on both models with
    test_gpu_timeparallel._symmetric_params(model, 5), T = 5,000, against the oracle run with the
    same constants.  The threshold by test_lookahead_gated_kernel_models_and_constants' rule, here
    on the oracle's numbers: the median record of the ungated run plus 40, 20, 10, 5 or 2.5, the
    first at which at least 2 % of events update (under 50 %); then the nearest of nine candidates
    0.05 apart around it whose oracle margin is >= 1e-5 (at least one must qualify)."""
    stream = _once('gated_oracle_custom', lambda: ttp._stream(5000, seed=31, skips=40))
    et, dt, pay, x0 = stream
    params = ttp._symmetric_params(model, 5)
    K = _oracle_consts(model, params)
    base = _oracle('custom', model, stream, -np.inf, K)[0]
    for above in (40.0, 20.0, 10.0, 5.0, 2.5):
        thr0 = float(np.median(base.logdet)) + above
        if _oracle('custom', model, stream, thr0, K)[0].updated.mean() >= 0.02:
            break
    cand = [thr0 + 0.05 * k for k in (0, -1, 1, -2, 2, -3, 3, -4, 4)]
    margin, count, _, _ = tsw.gate_margins(et, dt, cand, model, K)
    ok = [c for c, m in zip(cand, margin) if m >= MARGIN]
    assert ok, (cand, margin)
    thr = ok[0]
    orc = _oracle('custom', model, stream, thr, K)
    assert 0.02 <= orc[0].updated.mean() < 0.5, (thr, orc[0].updated.mean())
    dev = _device(model, stream, thr, kernel='gated', sequential=True, params=params)
    _compare('look-ahead custom', model, stream, dev, orc, thr, '-', K=K)


@pytest.mark.parametrize('thr', [-31.65, -10.65])
def test_chain_kernel_long_gated_vs_oracle(thr):
    """The anchor every kernel-against-kernel test leans on: events_kernel = 'chain' with
    sequential=True over the 70,000-event ref15 stream, against the oracle (same assertions as the
    route's)."""
    dev = _device('ref15', _long(), thr, kernel='chain', sequential=True)
    assert dev['chk'] is None
    _compare('chain', 'ref15', _long(), dev, _oracle('long', 'ref15', _long(), thr), thr, '-')


# ---------------------------------------------------------------------------------------------
# (d) the façade's adaptive driver over a long list
# ---------------------------------------------------------------------------------------------
def _long_list():
    def build():
        et, dt, pay, _ = _long()
        t = np.cumsum(dt)
        events = []
        for k in range(T_LONG):
            if et[k] == ref15.GPS:
                sd = {'easting': float(pay[k, 0]), 'northing': float(pay[k, 1]), 'altitude': float(pay[k, 2])}
                events.append((k, 'GPS', float(t[k]), sd))
            else:
                events.append((k, 'IMU', float(t[k]), [repr(float(t[k])), *(float(v) for v in pay[k])]))
        return events
    return _once('gated_oracle_list', build)


@pytest.mark.parametrize('thr', [-10.65, -31.65])
def test_facade_adaptive_long_list_vs_oracle(thr):
    """ref15.run_adaptive_threshold_kalman_filter over a list of 70,000 (index, type, time, sdata)
    events (times = cumsum(dt), the driver's own dt = t - previous t) against
    oracle.ref_kf.run_adaptive_threshold on the same list: update times equal, states, log-dets and
    final P within 1e-6, the previous time equal.  A plain list goes through _driver_stream and
    _run_streams; the same events as an ingest.EventStream go through run_monotone_stream and
    _stream_states (the device-resident driver), and must give the same.  The margin is the array
    oracle's over the list's own dt."""
    events = _long_list()
    arrays = _once('gated_oracle_list_arrays', lambda: tsw._list_arrays(events))
    margin = _once(('gated_oracle_list_margin', thr), lambda: gated_oracle.run_gated(
        'ref15', *arrays[:3], arrays[3], ref_kf.P0_REF15, thr).margin)
    assert margin >= MARGIN, margin
    st, ld, P, prev, times = _once(('gated_oracle_list_run', thr),
                                   lambda: ref_kf.run_adaptive_threshold(events, 0, len(events), thr))
    assert len(st) == T_LONG + 1 and 100 < len(times) < T_LONG
    et, dt, pay, _ = _long()
    dev = torch.device('cuda', 0)
    n = T_LONG
    stream = ingest.EventStream(etype=torch.as_tensor(et, device=dev),
                                t=torch.as_tensor(np.array([e[2] for e in events]), device=dev),
                                payload=torch.as_tensor(pay, device=dev),
                                src=torch.zeros(n, dtype=torch.int32, device=dev),
                                zone_number=torch.zeros(n, dtype=torch.int8, device=dev),
                                zone_letter=torch.zeros(n, dtype=torch.uint8, device=dev),
                                first_valid_index=0, gyro_bias=np.zeros(3), accel_bias=np.zeros(3),
                                utm_origin=np.zeros(2), n_fixes=int((et == 0).sum()), n_imu=int((et == 1).sum()))
    assert ref15._device_stream(events) is None and ref15._device_stream(stream) is stream
    for form, ev in (('list', events), ('stream', stream)):
        rs, rl, rP, rprev, rtimes = ref15.run_adaptive_threshold_kalman_filter(ev, 0, n, R_threshold=thr)
        np.testing.assert_array_equal(np.array(rtimes), np.array(times), err_msg=form)
        assert np.array(rs).shape == np.array(st).shape, form
        errs = (_rel(rs, st), _rel(rl, ld), _rel(rP, P))
        print(f'| façade {form} | ref15 | {thr:g} | margin {margin:.1e} | states {errs[0]:.1e} | logdet {errs[1]:.1e} | '
              f'P {errs[2]:.1e} |')
        assert max(errs) <= TOL, (form, errs)
        assert rprev == prev, form


# ---------------------------------------------------------------------------------------------
# (e) the route in f32
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thr', F32_THR)
def test_gated_route_f32_flags(thr):
    """An f32 handle over the 70,000-event stream through the route against the same handle's
    sequential run (kf_run_events_seq), kernel against kernel on purpose: does the route change the
    decisions of the same-precision sequential filter?  The thresholds sit in the band where the
    chunked records stand and the f64 margins run from 1e-5 to 1e-2, where a chunk start that is
    off by f32 rounding could flip a near-threshold gate and still pass the 1e-5 seam check.
    Flags equal at every one, records within 1e-3 (test_parallel_f32's tolerance)."""
    par = _device('ref15', _long(), thr, dtype='f32')
    seq = _once(('gated_oracle_f32_seq', thr), lambda: _device('ref15', _long(), thr, dtype='f32', sequential=True))
    chk = par['chk']
    assert chk is not None and chk['chunks'] > 1 and chk['warmup'] == 2048, chk
    assert seq['chk'] is None and par['status'] == seq['status'] == 0
    diff = int((par['updated'] != seq['updated']).sum())
    errs = {k: _rel(par[k], seq[k]) for k in ('traj', 'logdet', 'cov', 'x', 'P')}
    print(f'| route f32 | ref15 | {thr:g} | {_route(chk)} | {100 * seq["updated"].mean():.2f} % | flags differing {diff} | '
          + ' | '.join(f'{k} {v:.1e}' for k, v in errs.items()) + ' |')
    assert diff == 0, (thr, diff, int(np.argmax(par['updated'] != seq['updated'])))
    for k, v in errs.items():
        assert v <= 1e-3, (thr, k, v)


# ---------------------------------------------------------------------------------------------
# the lane option on a long one-filter stream; kf_stream_check's fallback word
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thr', [-10.65, None])
def test_lane_option_stays_off_the_stream_route(thr):
    """events_kernel = 'lane' with one filter over 70,000 events, gated and ungated: the lane
    kernel cannot run the route's fallback, so kf_run_events keeps the run sequential on the
    kernel the caller asked for — bitwise the sequential=True lane run, and no kf_run_stream on
    the handle."""
    a = _device('ref15', _long(), thr, kernel='lane')
    b = _device('ref15', _long(), thr, kernel='lane', sequential=True)
    assert a['chk'] is None and b['chk'] is None and a['status'] == b['status'] == 0
    for k in ('traj', 'logdet', 'updated', 'cov', 'x', 'P'):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a['updated'].any() and (thr is None) == bool(a['updated'].all())


def test_run_stream_rejects_the_lane_option():
    """A direct kf_run_stream with the lane option is KF_EINVAL before anything is queued: output
    buffers pre-filled with a sentinel and the handle's state are untouched."""
    et, dt, pay, x0 = _long()
    kf = tsw._handle('ref15', 1, 'f64', x0=x0, options={'events_kernel': 'lane'})
    try:
        d = kf.device
        e, t, p = (torch.as_tensor(v, device=d) for v in (et, dt, pay))
        tr, ld, cv = kf.empty(T_LONG, 6, 1), kf.empty(T_LONG, 1), kf.empty(T_LONG, 27, 1)
        up = torch.empty(T_LONG, 1, dtype=torch.uint8, device=d)
        for v in (tr, ld, cv):
            v.fill_(-7.25)
        up.fill_(93)
        x_in, P_in = (v.cpu().numpy() for v in kf.state())
        rc = _lib.lib().kf_run_stream(kf.handle, T_LONG, e.data_ptr(), t.data_ptr(), p.data_ptr(), tr.data_ptr(),
                                      cv.data_ptr(), ld.data_ptr(), up.data_ptr(), 0, -1, kf._stream())
        assert rc == _lib.KF_EINVAL and 'lane' in _lib.last_error(), (rc, _lib.last_error())
        with pytest.raises(kfmi.KFError) as err:
            kf.run_stream(e, t, p)
        assert err.value.code == _lib.KF_EINVAL
        torch.cuda.synchronize()
        for v in (tr, ld, cv):
            assert bool((v == -7.25).all())
        assert bool((up == 93).all())
        x, P = (v.cpu().numpy() for v in kf.state())
        np.testing.assert_array_equal(x, x_in)
        np.testing.assert_array_equal(P, P_in)
    finally:
        kf.close()


def test_stream_check_reports_the_forced_lookahead_fallback():
    """events_kernel = 'gated' forced through the route at -10.65: the seam check fails and the
    fallback the host queued is the look-ahead kernel, which stream_check must name (it used to
    derive the word from a device flag that only the device-chosen fallback writes: 'chain')."""
    dev = _device('ref15', _long(), -10.65, kernel='gated')
    chk = dev['chk']
    assert chk['chunks'] > 1 and not chk['ok'] and chk['fallback'] == 'gated', chk
    _compare('route, look-ahead forced', 'ref15', _long(), dev, _oracle('long', 'ref15', _long(), -10.65), -10.65,
             _route(chk))
    chain = _device('ref15', _long(), -10.65, kernel='chain')['chk']
    assert chain['chunks'] > 1 and not chain['ok'] and chain['fallback'] == 'chain', chain


@pytest.mark.parametrize('T,chunk', [(100, 128), (20, 0)])
def test_stream_check_of_an_unsplit_stream_reports_no_fallback(T, chunk):
    """A run_stream too short to split (100 events in chunks of 128; 20 events with the default
    chunk length, which is at least 32: 100 events would make four chunks of it) is one chunk: it
    ran sequentially and there was no fallback (the word used to say 'chain')."""
    et, dt, pay, x0 = (v[:T] if v.ndim and len(v) == T_LONG else v for v in _long())
    kf = tsw._handle('ref15', 1, 'f64', x0=x0)
    try:
        tr, ld, _, _ = kf.run_stream(et, dt, pay, chunk=chunk)
        chk = kf.stream_check()
        assert chk['chunks'] == 1 and chk['fallback'] is None, chk
        r = gated_oracle.run_gated('ref15', et, dt, pay, x0, ref_kf.P0_REF15, -np.inf)
        assert _rel(tr[:, :, 0].cpu().numpy(), r.traj) <= TOL and _rel(ld[:, 0].cpu().numpy(), r.logdet) <= TOL
    finally:
        kf.close()
