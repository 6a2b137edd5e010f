"""kf_search_schedules and kf_schedule_plan are part of the C ABI; kfmi.ref15's host side of the
schedule search (the windowing, the metric track) equals the NumPy oracle helper; and that helper
reproduces the reference's own results (tests/golden/ref15_schedules.npz).  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest

import schedule_oracle as so
from golden_events import unpack_events
from kfmi import _lib, ref15

NAMES = {'kf_search_schedules': 14, 'kf_schedule_plan': 5}
CASES = ('f050', 'f120', 'f400', 'f030')
_cache = {}


def _golden(golden_dir):
    if 'g' not in _cache:
        g = np.load(os.path.join(golden_dir, 'ref15_schedules.npz'))
        _cache['g'] = (g, unpack_events(g))
    return _cache['g']


@pytest.mark.parametrize('name', sorted(NAMES))
def test_entry_point_is_declared_exported_and_bound(name):
    assert name in _lib.header_functions()
    assert name in _lib.SIGNATURES
    assert hasattr(_lib.lib(), name)
    assert len(_lib.SIGNATURES[name][1]) == NAMES[name]


def test_null_handle_is_einval():
    L = _lib.lib()
    rc = L.kf_search_schedules(None, 1, None, None, None, None, 0.0, 0, None, None, None, None, None, None)
    assert rc == _lib.KF_EINVAL
    assert 'null' in _lib.last_error()


# ---------------------------------------------------------------------------------------------
# the planner (it needs no handle: the plan depends on the queue lengths alone)
# ---------------------------------------------------------------------------------------------
def _plan(q_len, n_fixed=0):
    q = np.asarray(q_len, np.int32)
    out = np.full(3, -7, np.int64)
    rc = _lib.lib().kf_schedule_plan(None, len(q), q.ctypes.data_as(ctypes.c_void_p), n_fixed,
                                     out.ctypes.data_as(ctypes.c_void_p))
    return rc, [int(v) for v in out]


def _bytes(C, W, widest):
    a = lambda n: (n + 255) // 256 * 256  # noqa: E731
    # candidates [14][C], init [42], fixed picks [W] int32, 4096 x 3 partials, two levels of 28 rows
    return a(14 * 8 * C) + a(42 * 8) + a(4 * W) + a(4096 * 3 * 8) + 2 * a(28 * 8 * widest)


@pytest.mark.parametrize('q_len, n_fixed, n_free, widest', [
    ((5,), 0, 5, 0),                       # one window: nothing stored
    ((3, 1, 4), 0, 12, 3),                 # stored levels 3, 3: the widest before the last
    ((4, 4, 4, 4, 3, 3), 0, 2304, 768),
    ((4, 4, 4, 4, 3, 3), 2, 144, 48),      # the first two windows fixed
    ((4, 3, 5, 2), 3, 2, 0),               # one free window
    ((4, 3, 5, 2), 4, 1, 0),               # every window fixed: the one schedule
    ((65, 3), 0, 195, 65),
    ((3, 65), 0, 195, 3),
    ((2,) * 10, 0, 1024, 512),
])
def test_plan_counts(q_len, n_fixed, n_free, widest):
    rc, out = _plan(q_len, n_fixed)
    assert rc == _lib.KF_OK, _lib.last_error()
    assert out == [n_free, widest, _bytes(sum(q_len), len(q_len), widest)]


def test_plan_reports_a_space_of_2_to_the_40_or_more():
    rc, out = _plan((1024,) * 4)           # exactly 2^40
    assert rc == _lib.KF_OK and out[0] == -1 and out[1] == 1 << 30
    rc, out = _plan((1024,) * 4, 1)        # 2^30 once the first window is fixed
    assert rc == _lib.KF_OK and out[0] == 1 << 30 and out[1] == 1 << 20
    rc, out = _plan((1024,) * 3 + (1023,))
    assert rc == _lib.KF_OK and out[0] == 1023 << 30
    rc, out = _plan((1000,) * 40)          # far beyond 64 bits: still -1, never wrapped
    assert rc == _lib.KF_OK and out[0] == -1 and out[2] == np.iinfo(np.int64).max


@pytest.mark.parametrize('q_len, n_fixed, text', [
    ((3, 0, 2), 0, 'q_len[1]'), ((3, 1025), 0, 'q_len[1]'), ((2,) * 65, 0, 'W = 65'), ((), 0, 'W = 0'),
    ((3, 2), 3, 'n_fixed'), ((3, 2), -1, 'n_fixed')])
def test_plan_limits_are_einval(q_len, n_fixed, text):
    rc, out = _plan(q_len, n_fixed)
    assert rc == _lib.KF_EINVAL and text in _lib.last_error()
    assert out == [-7, -7, -7]


# ---------------------------------------------------------------------------------------------
# the windowing and the metric track against the oracle helper
# ---------------------------------------------------------------------------------------------
def _same_queues(a, b):
    return [[e[0] for e in q] for q in a] == [[e[0] for e in q] for q in b]


@pytest.mark.parametrize('freq', [20.0, 50.0, 120.0, 400.0])
def test_schedule_queues_equal_the_oracles(golden_dir, freq):
    _, events = _golden(golden_dir)
    first_fix = next(i for i, e in enumerate(events) if e[1] == 'GPS')
    assert first_fix > 0                       # the stream opens with IMU samples: nothing before the fix is queued
    for start, end in [(0, None), (0, len(events)), (first_fix + 3, None), (0, 150), (7, 211), (40, 41), (0, 0)]:
        got = ref15.schedule_queues(events, start, end, freq)
        want = so.queues(events, start, end, freq)
        assert _same_queues(got, want), (start, end)
        stop = len(events) if end is None else end
        if start <= first_fix < stop:          # windows that start before the first fix open at it
            assert not got or got[0][0][0] == first_fix
    whole = so.queues(events, 0, None, freq)
    lens = {len(q) for q in whole}
    if freq == 400.0:                          # every trigger meets an empty queue and is queued alone
        assert lens == {1}
    else:
        assert len(lens) > 1
    # an end_idx that cuts the third window (before its last candidate): the partial queue is discarded
    assert len(ref15.schedule_queues(events, 0, whole[2][-1][0], freq)) == 2


@pytest.mark.parametrize('case', CASES)
def test_golden_queues_are_the_references(golden_dir, case):
    g, events = _golden(golden_dir)
    qs = ref15.schedule_queues(events, 0, int(g[case + '_end_idx']), float(g[case + '_freq']))
    assert [len(q) for q in qs] == list(g[case + '_q_len'])
    assert [e[0] for q in qs for e in q] == list(g[case + '_cand'])
    # one event less and the last window is not complete
    assert len(ref15.schedule_queues(events, 0, int(g[case + '_end_idx']) - 1, float(g[case + '_freq']))) == len(qs) - 1


def test_track_positions_equal_scipy_interp1d():
    from scipy.interpolate import interp1d
    rng = np.random.default_rng(3)
    t = 1.7e9 + np.cumsum(rng.uniform(0.05, 0.15, 25))
    p = np.cumsum(rng.normal(0, 2.0, (25, 3)), 0) + [300.0, -200.0, 30.0]
    tq = np.concatenate([t[0] - rng.uniform(0, 1, 5), rng.uniform(t[0], t[-1], 40), t[-1] + rng.uniform(0, 1, 5),
                         t[[0, 7, 24]]])
    want = np.stack([interp1d(t, p[:, k], kind='linear', fill_value='extrapolate')(tq) for k in range(3)], 1)
    for got in (ref15.track_positions(t, p, tq), so.track_positions(t, p, tq)):
        assert got.shape == (len(tq), 3)
        assert np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0)) <= 1e-12
    for bad in (t[::-1], np.concatenate([t[:5], t[4:]])):   # decreasing; a repeated time
        with pytest.raises(ValueError):
            ref15.track_positions(bad, np.zeros((len(bad), 3)), tq)


# ---------------------------------------------------------------------------------------------
# the oracle helper against the reference's own results
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_oracle_reproduces_the_golden(golden_dir, case):
    g, events = _golden(golden_dir)
    qs = so.queues(events, 0, int(g[case + '_end_idx']), float(g[case + '_freq']))
    m, states = so.metrics(qs, *so.fixes(events), with_states=True)
    want = g[case + '_metrics']
    assert m.shape == want.shape
    assert np.max(np.abs(m - want) / np.abs(want)) <= 1e-12
    rank, best = so.winner(m)
    assert rank == int(g[case + '_best_rank'])
    traj, x, P = states[rank]
    for got, ref in ((traj, g[case + '_traj']), (x, g[case + '_x']), (P, g[case + '_P'])):
        assert np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)) <= 1e-12


def test_driver_refuses_a_space_it_cannot_enumerate(golden_dir):
    """Before any device work: a space over max_schedules is a ValueError naming log10 of the
    count (the notebook prints a warning and never finishes); no complete window is the
    notebook's empty result."""
    _, events = _golden(golden_dir)
    qs = so.queues(events, 0, None, 20.0)
    log_n = sum(np.log10(len(q)) for q in qs)
    assert log_n > 12
    with pytest.raises(ValueError, match=f'log10 = {log_n:.2f}'):
        ref15.search_schedules(events, 0, None, 20.0)
    with pytest.raises(ValueError, match='log10'):
        ref15.search_schedules(events, 0, 60, 50.0, max_schedules=100)
    r = ref15.search_schedules(events, 0, 8, 20.0)
    assert r['accuracy_metric'] == float('inf') and r['q_len'] == [] and r['n_schedules'] == 0
    assert all(r[k] is None for k in ('selected_sensors', 'final_state', 'final_covariance', 'trajectory', 'rank'))


def test_host_arrays_of_a_window_set(golden_dir):
    g, events = _golden(golden_dir)
    qs = ref15.schedule_queues(events, 0, int(g['f030_end_idx']), 30.0)
    ft, fp = so.fixes(events)
    q_len, ev, ref = ref15.schedule_arrays(qs, ft, fp)
    flat = [e for q in qs for e in q]
    assert list(q_len) == [len(q) for q in qs] and ev.shape == (len(flat), 11) and ref.shape == (len(flat), 3)
    for row, (_, stype, t, sd) in zip(ev, flat):
        assert row[0] == t and row[1] == (0 if stype == 'GPS' else 1)
        assert list(row[2:]) == [float(v) for v in ref15.event_payload(stype, sd)]
    assert np.array_equal(ref, ref15.track_positions(ft, fp, ev[:, 0]))
    t2, p2 = ref15._track_of(events, None)       # the list's own fixes
    assert np.array_equal(t2, ft) and np.array_equal(p2, fp)
