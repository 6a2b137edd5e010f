"""Ragged tails of one event stream in one launch (kf_run_tails through BatchedKF.run_tails,
kfmi.ref15.AdaptiveSweep.warm_starts and the façade's run_experiment_windows /
run_experiment_grid) — needs an MI355X.

A tail is the sweep kernel's group run over its own range of the stream from its own source
column, so every comparison with the one-filter kf_run_sweep from the same state is bit for bit
(the same arithmetic, the state crossing HBM in the handle's dtype either way); only the oracle
comparison carries a tolerance (TOL, under tests/test_gpu_sweep.py's margin rule).  The shapes are
the smallest at which the kernel can go wrong: a partial wave, a wave mixing empty and long tails,
lengths around the input ring's depth of 4, a tail ending at the stream's end, a tail starting at
event 0 from the handle's own column, NONE events inside tails.
"""
import random

import numpy as np
import pytest
import torch

import kfmi
from kfmi import _lib, ref15
from kfmi import kf_workers as kfw
from oracle import ref_kf
from test_gpu_sweep import (F32_THR, MARGIN, STREAM4_THR, TOL, WARM_THR, _golden, _golden_arrays, _handle, _margins,
                            _np, _once, _rel, _stream, _stream4, _sweep, _symmetric_consts, gate_margins,
                            pick_thresholds)

pytestmark = pytest.mark.gpu
INF = float('inf')
STATE = ('x', 'P', 'status', 'n_updated')


# ---------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------
def _tails(et, dt, pay, x0, specs, thr, src=None, dtype='f64', model='ref15', params=None):
    """One run_tails call on a cold-started handle of len(specs) filters; specs: (lo, hi, src_row,
    src_col) per tail, src: (src_x, src_P).  Returns the end x, P, status and n_updated."""
    npd = np.float64 if dtype == 'f64' else np.float32
    kf = _handle(model, len(specs), dtype, params, x0)
    try:
        lo, hi, row, col = (np.array([s[k] for s in specs], np.int32) for k in range(4))
        nu = kf.run_tails(et, dt, pay.astype(npd), lo, hi, np.asarray(thr, np.float64),
                          src_x=None if src is None else src[0], src_P=None if src is None else src[1],
                          src_row=row, src_col=col, counts=True)
        x, P = kf.state()
        return dict(x=_np(x), P=_np(P), status=_np(kf.status()), n_updated=_np(nu))
    finally:
        kf.close()


def _source(src, row, col):
    """Source column (row, col) as a one-filter state, or None for the handle's own cold start."""
    return None if row < 0 else (src[0][row][:, col:col + 1], src[1][row][:, col:col + 1])


def _one(et, dt, pay, x0, spec, thr, src, **kw):
    """The one-filter kf_run_sweep over the tail's events from its source column."""
    lo, hi, row, col = spec
    assert hi > lo
    return _sweep(et[lo:hi], dt[lo:hi], pay[lo:hi], x0, [thr], state=_source(src, row, col), traj=False, logdet=False,
                  **kw)


def _assert_tail(got, f, want):
    for k in STATE:
        np.testing.assert_array_equal(got[k][..., f], want[k][..., 0], err_msg=f'tail {f}: {k}')


def _assert_untouched(got, f, x0, spec, src, model='ref15', dtype='f64', params=None):
    """A tail of length 0: its source column bit for bit, no updates."""
    _, _, row, col = spec
    if row < 0:
        kf = _handle(model, 1, dtype, params, x0)
        sx, sP = (_np(v) for v in kf.state())
        kf.close()
    else:
        sx, sP = _source(src, row, col)
    assert got['x'][:, f].tobytes() == np.ascontiguousarray(sx[:, 0]).tobytes()
    assert got['P'][:, f].tobytes() == np.ascontiguousarray(sP[:, 0]).tobytes()
    assert got['status'][f] == 0 and got['n_updated'][f] == 0


def _same(a, b):
    """Deep equality of the drivers' results (tuples, lists, dicts, arrays, numbers, None)."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys()
        for k in a:
            _same(a[k], b[k])
    elif isinstance(a, (tuple, list)):
        assert isinstance(b, (tuple, list)) and len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    elif isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    else:
        assert a == b, (a, b)


# ---------------------------------------------------------------------------------------------
# 1, 2: warm_starts against warm_start and against the oracle
# ---------------------------------------------------------------------------------------------
WARM_ENDS = (1, 3, 5, 6, 64, 65, 68, 200, 427)


def _warm(golden_dir):
    """(pairs, warm_starts' list, the warm_start loop's list) over WARM_ENDS x WARM_THR, shuffled."""
    def run():
        _, events = _golden(golden_dir)
        pairs = [(i, e) for e in WARM_ENDS for i in range(len(WARM_THR))]
        random.Random(7).shuffle(pairs)
        sw = ref15.AdaptiveSweep(events, WARM_THR, checkpoint_every=64, records=False)
        try:
            got = sw.warm_starts([i for i, _ in pairs], [e for _, e in pairs])
            want = [sw.warm_start(i, e) for i, e in pairs]
            assert len(sw._kft) == 1  # one handle, cached by batch size
            again = sw.warm_starts([i for i, _ in pairs], [e for _, e in pairs])
            assert len(sw._kft) == 1
        finally:
            sw.close()
        assert sw._kft == {}
        return pairs, got, want, again
    return _once('tails_warm', run)


def test_warm_starts_equal_warm_start(golden_dir):
    """warm_starts over ends (1, 3, 5, 6, 64, 65, 68, 200, 427) x the three WARM_THR thresholds
    in shuffled order (checkpoint_every = 64: tails of 0 to 63 events from row -1 and from
    checkpoint rows, the last ending at the stream's end) equals [warm_start(i, e) ...] entry by
    entry: None where None (ends at or before the first fix, index 5), tuples equal with ==, P
    equal with assert_array_equal.  A second call on the cached handle gives the same."""
    pairs, got, want, again = _warm(golden_dir)
    assert len(got) == len(want) == 27
    assert sum(w is None for w in want) == 9
    for (i, e), g, w, a in zip(pairs, got, want, again):
        if w is None:
            assert g is None and a is None and e <= 5, (i, e)
            continue
        for r in (g, a):
            assert type(r) is tuple and len(r) == 3 and type(r[0]) is tuple and len(r[0]) == 7
            assert all(type(v) is float for v in r[0]) and type(r[2]) is float
            assert r[0] == w[0] and r[2] == w[2], (i, e)
            assert r[1].shape == (15, 15) and r[1].dtype == w[1].dtype
            np.testing.assert_array_equal(r[1], w[1])


def test_warm_starts_vs_oracle(golden_dir):
    """The non-None entries against the NumPy oracle's run_adaptive_threshold(events, 0, end,
    R_threshold): states[-1] and P within TOL = 1e-6, previous_time equal.  Margin rule: all
    three WARM_THR thresholds must have a margin >= 1e-5 over the golden run (none excluded)."""
    _, events = _golden(golden_dir)
    et, dt, _, _ = _golden_arrays(golden_dir)
    margin, _, _, _ = _margins('golden_warm', et, dt, WARM_THR)
    assert np.all(margin >= MARGIN['f64']), margin
    pairs, got, _, _ = _warm(golden_dir)
    n = 0
    for (i, e), g in zip(pairs, got):
        if g is None:
            continue
        ost, _, oP, oprev, _ = ref_kf.run_adaptive_threshold(events, 0, e, R_threshold=WARM_THR[i])
        state, P, prev = g
        print(f'end {e} thr {WARM_THR[i]}: state {_rel(state, ost[-1]):.2e} P {_rel(P, oP):.2e}')
        assert _rel(state, ost[-1]) <= TOL and _rel(P, oP) <= TOL, (i, e)
        assert prev == oprev and state[0] == ost[-1][0]
        n += 1
    assert n == 18


# ---------------------------------------------------------------------------------------------
# 3, 4: raw shapes through BatchedKF.run_tails
# ---------------------------------------------------------------------------------------------
def _stream4_sources():
    """Stream 4 (5,000 events, 300 NONE) under STREAM4_THR with checkpoint_every = 512: the
    sources ckpt_x [9, 15, 10], ckpt_P [9, 27, 10]."""
    def run():
        et, dt, pay, x0 = _stream4()
        r = _sweep(et, dt, pay, x0, STREAM4_THR, traj=False, logdet=False, checkpoint_every=512)
        assert r['ckpt_x'].shape == (9, 15, 10) and int(np.abs(r['status']).sum()) == 0
        return r['ckpt_x'], r['ckpt_P']
    return _once('tails_stream4_src', run)


def _stream4_specs():
    """Nine tails (lo, hi, src_row, src_col): lengths 0, 1, 3, 4, 5 and 511 from lo = 0 (row -1)
    and lo = 512 (row + 1), and one of 392 events that ends at the stream's end (row 8, hi = T).
    The first wave holds a length-0 tail next to two of 511; the ninth tail is a second wave of
    one group, empty from row -1."""
    T = 5000
    rows = [(-1, 511), (0, 0), (3, 1), (-1, 3), (5, 4), (8, T - 512 * 9), (2, 5), (7, 511), (-1, 0)]
    specs = []
    for f, (row, n) in enumerate(rows):
        lo = 512 * (row + 1)
        specs.append((lo, lo + n, row, (3 * f + 1) % 10))
    et = _stream4()[0]
    assert len(et) == T and specs[5][1] == T
    assert all((et[s[0]:s[1]] == ref15.NONE).any() for s in specs if s[1] - s[0] > 300)  # NONE events inside tails
    return specs


def _stream4_want(spec):
    et, dt, pay, x0 = _stream4()
    return _once(('tails_stream4_one', spec),
                 lambda: _one(et, dt, pay, x0, spec, STREAM4_THR[spec[3]], _stream4_sources()))


def _check_stream4(specs):
    et, dt, pay, x0 = _stream4()
    src = _stream4_sources()
    got = _tails(et, dt, pay, x0, specs, [STREAM4_THR[s[3]] for s in specs], src)
    for f, spec in enumerate(specs):
        if spec[1] == spec[0]:
            _assert_untouched(got, f, x0, spec, src)
        else:
            _assert_tail(got, f, _stream4_want(spec))
    return got


@pytest.mark.parametrize('B', [1, 8, 9])
def test_tails_equal_one_filter_sweeps(B):
    """B = 1, 8 (one full wave) and 9 (a second, partial wave) tails of stream 4 from one sweep's
    checkpoints: each tail's end x, P, status and n_updated equal, bit for bit, the one-filter
    sweep over its events from its source column; a tail of length 0 leaves its source column
    bit for bit with n_updated = 0."""
    got = _check_stream4(_stream4_specs()[:B])
    assert int(np.abs(got['status']).sum()) == 0 and got['n_updated'][0] > 0


def test_order_does_not_matter():
    """The B = 9 call with its tails permuted gives the permuted results bit for bit, and two
    identical tails in one call (one in each wave) give identical columns."""
    specs = _stream4_specs()
    base = _check_stream4(specs)
    perm = [4, 8, 0, 7, 2, 5, 1, 3, 6]
    got = _check_stream4([specs[p] for p in perm])
    for k in STATE:
        np.testing.assert_array_equal(got[k], base[k][..., perm], err_msg=k)
    twice = _check_stream4(specs[:8] + [specs[7]])
    for k in STATE:
        np.testing.assert_array_equal(twice[k][..., 7], twice[k][..., 8], err_msg=k)


# ---------------------------------------------------------------------------------------------
# 5: failures
# ---------------------------------------------------------------------------------------------
def test_failure_is_per_tail(golden_dir):
    """One of eight tails starts from a source column whose covariance is not positive definite
    (P[0] = -1e6, as in test_failure_is_per_filter): it ends NaN with KF_ENOTSPD; the other seven
    of its wave equal their one-filter runs bit for bit with status 0."""
    et, dt, pay, x0 = _golden_arrays(golden_dir)
    T = len(et)
    thr = [-INF] * 4 + [-25.0, -11.4, 0.3, INF]
    kf = _handle('ref15', 8, 'f64', x0=x0)
    x, P = (_np(v) for v in kf.state())
    kf.close()
    bad = 2
    P[0, bad] = -1e6
    src = (x[None].copy(), P[None].copy())
    specs = [(0, T, 0, f) for f in range(8)]
    got = _tails(et, dt, pay, x0, specs, thr, src)
    assert got['status'][bad] == _lib.KF_ENOTSPD
    assert np.isnan(got['x'][:, bad]).all() and np.isnan(got['P'][:, bad]).all()
    for f in range(8):
        if f == bad:
            continue
        assert got['status'][f] == 0
        _assert_tail(got, f, _one(et, dt, pay, x0, specs[f], thr[f], src))


# ---------------------------------------------------------------------------------------------
# 6: models, constants, f32
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['ref8', 'ref15_custom', 'ref15_f32'])
def test_models_constants_f32(golden_dir, case):
    """ref8 with the reference's constants, ref15 with custom axis-symmetric constants, and ref15
    in f32 on the golden stream: four tails of lengths 0, 5, 64 and 300 (rows 2, 1, 0 of a
    checkpoint_every = 128 sweep and row -1), bit for bit against the one-filter sweep from the
    same source column."""
    model, dtype, params = 'ref15', 'f64', None
    if case == 'ref15_f32':
        et, dt, pay, x0 = _golden_arrays(golden_dir)
        dtype, thr = 'f32', F32_THR[:4]
    else:
        et, dt, pay, x0 = _stream(1500, seed=23, skips=40)
        consts = None
        if case == 'ref8':
            model = 'ref8'
        else:
            consts = _symmetric_consts('ref15', 5)
            params = consts.params()
        cand, _ = pick_thresholds(et, dt, model, consts.oracle() if consts else None, MARGIN['f64'])
        thr = [float(v) for v in cand[:4]]
    kw = dict(dtype=dtype, model=model, params=params)
    r = _sweep(et, dt, pay, x0, thr, traj=False, logdet=False, checkpoint_every=128, **kw)
    src = (r['ckpt_x'], r['ckpt_P'])
    assert src[0].shape[0] >= 3 and len(et) >= 300
    specs = [(128 * (row + 1), 128 * (row + 1) + n, row, f)
             for f, (row, n) in enumerate([(2, 0), (1, 5), (0, 64), (-1, 300)])]
    got = _tails(et, dt, pay, x0, specs, thr, src, **kw)
    assert got['x'].dtype == (np.float32 if dtype == 'f32' else np.float64)
    _assert_untouched(got, 0, x0, specs[0], src, **kw)
    for f in (1, 2, 3):
        _assert_tail(got, f, _one(et, dt, pay, x0, specs[f], thr[f], src, **kw))
    assert got['n_updated'][3] > 0


# ---------------------------------------------------------------------------------------------
# 7: argument errors
# ---------------------------------------------------------------------------------------------
def test_argument_errors(golden_dir):
    """KF_EINVAL with its text for a cv3 handle, T = -1, null thresholds, lo > hi, hi > T, lo < 0,
    src_row >= src_rows, src_col >= src_batch and src_row >= 0 with null src_x; nothing is
    launched (the handle's state stays bitwise), and the same call with valid arguments runs."""
    et, dt, pay, x0 = _golden_arrays(golden_dir)
    T = len(et)
    L = _lib.lib()
    kf = _handle('ref15', 2, 'f64', x0=x0)
    cv = kfmi.BatchedKF('cv3', 2, 'f64')
    try:
        d = kf.device
        e, t, p, th = (torch.as_tensor(v, device=d) for v in (et, dt, pay, np.array([-10.0, 0.0])))
        sx, sP = kf.state()
        sx, sP = sx[None].repeat(3, 1, 1).contiguous(), sP[None].repeat(3, 1, 1).contiguous()  # [3, ., 2]
        x_in, P_in = (_np(v) for v in kf.state())

        def call(h, n, thr, lo, hi, row, col, srcx=sx.data_ptr()):
            arr = [np.array(v, np.int32) for v in (lo, hi, row, col)]
            return L.kf_run_tails(h.handle, n, e.data_ptr(), t.data_ptr(), p.data_ptr(), arr[0].ctypes.data,
                                  arr[1].ctypes.data, thr, srcx, sP.data_ptr(), 3, 2, arr[2].ctypes.data,
                                  arr[3].ctypes.data, None, kf._stream())
        ok = ([0, 64], [40, T], [-1, 2], [0, 1])
        for args, text in (((cv, T, th.data_ptr(), *ok), 'KF_MODEL_REF15'),
                           ((kf, -1, th.data_ptr(), *ok), 'T = -1'),
                           ((kf, T, None, *ok), 'null thresholds'),
                           ((kf, T, th.data_ptr(), [0, 65], [40, 64], [-1, 2], [0, 1]), 'tail 1'),
                           ((kf, T, th.data_ptr(), [0, 64], [T + 1, T], [-1, 2], [0, 1]), 'tail 0'),
                           ((kf, T, th.data_ptr(), [0, -1], [40, T], [-1, 2], [0, 1]), 'tail 1'),
                           ((kf, T, th.data_ptr(), [0, 64], [40, T], [-1, 3], [0, 1]), 'src_row = 3'),
                           ((kf, T, th.data_ptr(), [0, 64], [40, T], [0, 2], [2, 1]), 'src_col = 2'),
                           ((kf, T, th.data_ptr(), *ok, None), 'null src_x')):
            assert call(*args) == _lib.KF_EINVAL, text
            assert text in _lib.last_error(), (text, _lib.last_error())
            with pytest.raises(kfmi.KFError) as err:
                _lib.check(call(*args))
            assert err.value.code == _lib.KF_EINVAL
        with pytest.raises(ValueError):
            cv.run_tails(et, dt, pay, [0, 0], [1, 1], np.array([-10.0, 0.0]))
        with pytest.raises(ValueError):
            kf.run_tails(et, dt, pay, [0], [1], np.array([-10.0, 0.0]))
        torch.cuda.synchronize()
        x, P = (_np(v) for v in kf.state())
        assert x.tobytes() == x_in.tobytes() and P.tobytes() == P_in.tobytes()
        assert call(kf, T, th.data_ptr(), *ok) == _lib.KF_OK, _lib.last_error()
        torch.cuda.synchronize()
        assert not np.array_equal(_np(kf.state()[0]), x_in)
        # T = 0 with every lo = hi = 0 is legal, and copies the source states
        assert call(kf, 0, th.data_ptr(), [0, 0], [0, 0], [-1, 1], [0, 1]) == _lib.KF_OK, _lib.last_error()
        torch.cuda.synchronize()
        assert _np(kf.state()[0])[:, 1].tobytes() == _np(sx)[1][:, 1].tobytes()
    finally:
        kf.close()
        cv.close()


# ---------------------------------------------------------------------------------------------
# 8: the façade
# ---------------------------------------------------------------------------------------------
RATIOS = [0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]
KEYS = ('full', 'adaptive', 'no_update', 'brute_force', 'threshold')


def _facade(events):
    sf = kfw.KF_SensorFusion('gps.csv', 'imu.csv')  # nothing is loaded: the events are the golden list
    sf.indexed_sensor_data = events
    return sf


def test_facade_windows_and_grid(golden_dir):
    """run_experiment_windows(starts, sweep=sw, sweep_index=...) over twenty 25-event golden
    windows equals the same call given initial_pts / initial_states from a warm_start loop: every
    window's full, adaptive, no_update, brute_force and threshold.  run_experiment_grid over five
    starts x the sweep's three thresholds equals those fifteen windows, start-major."""
    _, events = _golden(golden_dir)
    sf = _facade(events)
    starts = [30 + 19 * w for w in range(20)]
    index = [w % 3 for w in range(20)]
    ratios = [RATIOS[w % 7] for w in range(20)]
    sw = ref15.AdaptiveSweep(events, WARM_THR, 0, len(events), checkpoint_every=64, records=False)
    try:
        got = sf.run_experiment_windows(starts, ratios=ratios, sweep=sw, sweep_index=index)
        warm = [sw.warm_start(i, s) for i, s in zip(index, starts)]
        want = sf.run_experiment_windows(starts, ratios=ratios, initial_pts=[w[1] for w in warm],
                                         initial_states=[w[0] for w in warm])
        assert len(got) == len(want) == 20
        for w in range(20):
            for k in KEYS:
                _same(got[w][k], want[w][k])
        with pytest.raises(ValueError):
            sf.run_experiment_windows([3], ratios=[0.5], sweep=sw, sweep_index=[0])  # no fix before event 3
        g_starts = starts[2:7]
        g_ratios = RATIOS[1:4]
        grid = sf.run_experiment_grid(g_starts, sw, ratios=g_ratios)
        flat = [(s, i) for s in g_starts for i in range(3)]
        warm = [sw.warm_start(i, s) for s, i in flat]
        want = sf.run_experiment_windows([s for s, _ in flat], ratios=[g_ratios[i] for _, i in flat],
                                         initial_pts=[w[1] for w in warm], initial_states=[w[0] for w in warm])
        assert len(grid) == len(want) == 15
        for w in range(15):
            for k in KEYS:
                _same(grid[w][k], want[w][k])
        with pytest.raises(ValueError):
            sf.run_experiment_grid(g_starts, sw)  # seven ratios for a sweep of three thresholds
    finally:
        sw.close()
