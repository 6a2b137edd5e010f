"""The per-window schedule search scored by position RMSE (kf_search_schedules through
BatchedKF.search_schedules, kfmi.ref15.search_schedules and the façade's
run_brute_force_kalman_filter) against the reference's own results and the NumPy oracle helper
(tests/schedule_oracle.py) — needs an MI355X.

The winner rule.  Two schedules' metrics can lie closer than the device agrees with the oracle
(the closest pair of the rankings below is ~1e-11 apart), so only the best is compared, and only
where the oracle's best lies at least MARGIN (relative) below its second best; that gap is
asserted first, as a condition on the seed.
"""
import os

import numpy as np
import pytest
import torch

import kfmi
import schedule_oracle as so
from golden_events import unpack_events
from kfmi import _lib, ref15
from kfmi import kf_workers as kfw
from test_gpu_sweep import KERNELS, MARGIN, TOL, _rel, _stream, _symmetric_consts

pytestmark = pytest.mark.gpu
NAN = float('nan')
SHAPES = [(1,), (5,), (1, 1, 1), (3, 1, 4), (4, 4, 4, 4, 3, 3), (7, 6, 6, 6), (2,) * 10, (65, 3), (3, 65)]
CASES = ('f050', 'f120', 'f400', 'f030')
_cache = {}


def _once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


# ---------------------------------------------------------------------------------------------
# inputs (computed once, never modified)
# ---------------------------------------------------------------------------------------------
def _events(seed):
    """_stream(400, seed) as the reference's event tuples with absolute times."""
    def build():
        et, _, pay, _ = _stream(400, seed)
        t = 1000.0 + np.arange(400) * 0.005
        out = []
        for i in range(400):
            if et[i] == ref15.GPS:
                out.append((i, 'GPS', float(t[i]), {'time': float(t[i]), 'easting': pay[i, 0], 'northing': pay[i, 1],
                                                    'altitude': pay[i, 2]}))
            else:
                out.append((i, 'IMU', float(t[i]), [repr(t[i]), *pay[i]]))
        return out
    return _once(('events', seed), build)


WARM_EVENTS = 6   # the warm start: the oracle's filter over the stream's first events


def _consts(kind):
    return None if kind == 'reference' else _symmetric_consts('ref15', 2)


SEED = 8   # of seeds 1 .. 8 the one whose oracle gaps are >= MARGIN for every shape below (1.7e-5 at the least;
           # a cold start's metrics are ~360 m, x0 = 0 being that far from the track, so its gaps are small)


def _case(q_len, kind, warm, seed=SEED):
    """One random queue set: consecutive events of the stream, window after window.  Returns
    dict(queues, q_len, ev, ref, init, prev, metrics (the oracle's), consts)."""
    def build():
        events = _events(seed)
        consts = _consts(kind)
        K = consts.oracle() if consts is not None else None
        ft, fp = so.fixes(events)
        x, P, prev = np.zeros(15), so.P0, None
        if warm:
            for _, stype, t, sd in events[:WARM_EVENTS]:
                x, P = so.ref_kf.step15(x, P, stype, sd, 0.0 if prev is None else t - prev, K)
                prev = t
        pos, queues = WARM_EVENTS + 1, []
        for q in q_len:
            queues.append(events[pos:pos + q])
            pos += q
        assert pos <= len(events)
        ql, ev, ref = ref15.schedule_arrays(queues, ft, fp)
        m = so.metrics(queues, ft, fp, x, P, prev, K)
        return dict(queues=queues, q_len=ql, ev=ev, ref=ref, init=np.concatenate([x, ref15.to_blocks(P)]),
                    prev=NAN if prev is None else prev, metrics=m, consts=consts)
    return _once(('case', tuple(q_len), kind, warm, seed), build)


def _handle(consts=None):
    return kfmi.BatchedKF('ref15', 1, 'f64', params=consts.params() if consts is not None else None)


def _gap(m):
    """Relative gap between the oracle's best and second-best finite metrics (inf with one)."""
    s = np.sort(m[np.isfinite(m)])
    return float('inf') if len(s) < 2 else float((s[1] - s[0]) / max(s[0], 1.0))


def _golden(golden_dir):
    def load():
        g = np.load(os.path.join(golden_dir, 'ref15_schedules.npz'))
        return g, unpack_events(g)
    return _once('golden', load)


# ---------------------------------------------------------------------------------------------
# 1. the reference's own results
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_golden_metrics_and_winner(golden_dir, case):
    g, events = _golden(golden_dir)
    r = ref15.search_schedules(events, 0, int(g[case + '_end_idx']), float(g[case + '_freq']), metrics=True)
    want = g[case + '_metrics']
    got = r['metrics'].cpu().numpy()
    assert r['q_len'] == list(g[case + '_q_len']) and got.shape == want.shape
    print(case, 'metrics', _rel(got, want), 'gap', _gap(want))
    assert _rel(got, want) <= TOL
    assert r['n_valid'] == r['n_schedules'] == len(want)
    assert _gap(want) >= MARGIN['f64']
    assert r['rank'] == int(g[case + '_best_rank'])
    assert _rel(r['accuracy_metric'], float(g[case + '_best_metric'])) <= TOL


@pytest.mark.parametrize('case', CASES)
def test_facade_returns_the_notebooks_dict(golden_dir, case):
    g, events = _golden(golden_dir)
    sf = kfw.KF_SensorFusion('gps.csv', 'imu.csv')
    sf.indexed_sensor_data = events
    freq = float(g[case + '_freq'])
    if case == 'f050':      # the metric track from utm_data, the rate from set_processing_frequency
        sf.utm_data = [e[3] for e in events if e[1] == 'GPS']
        sf.set_processing_frequency(freq)
        r = sf.run_brute_force_kalman_filter(0, int(g[case + '_end_idx']))
    else:                   # no utm_data: the list's own fixes
        r = sf.run_brute_force_kalman_filter(0, int(g[case + '_end_idx']), overwrite_sampling_freq=freq,
                                             max_combos_in_memory=10)
    assert sorted(r) == ['accuracy_metric', 'final_covariance', 'final_state', 'selected_sensors', 'trajectory']
    digits = so.digits_of(int(g[case + '_best_rank']), [int(q) for q in g[case + '_q_len']])
    off = np.concatenate([[0], np.cumsum(g[case + '_q_len'])])
    assert [e[0] for e in r['selected_sensors']] == [int(g[case + '_cand'][off[w] + d]) for w, d in enumerate(digits)]
    errs = (_rel(np.array(r['trajectory']), g[case + '_traj']), _rel(r['final_state'], g[case + '_x']),
            _rel(r['final_covariance'], g[case + '_P']), _rel(r['accuracy_metric'], float(g[case + '_best_metric'])))
    print(case, 'trajectory, x, P, metric', errs)
    assert max(errs) <= TOL
    assert r['final_state'].shape == (15,) and r['final_covariance'].shape == (15, 15)


def test_facade_without_a_complete_window(golden_dir):
    g, events = _golden(golden_dir)
    sf = kfw.KF_SensorFusion('gps.csv', 'imu.csv')
    sf.indexed_sensor_data = events
    r = sf.run_brute_force_kalman_filter(0, int(g['f050_end_idx']) - 20, overwrite_sampling_freq=10.0)
    assert r == {'selected_sensors': None, 'final_state': None, 'final_covariance': None, 'trajectory': None,
                 'accuracy_metric': float('inf')}


# ---------------------------------------------------------------------------------------------
# 2. random queue sets against the oracle helper
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('warm', [False, True], ids=['cold', 'warm'])
@pytest.mark.parametrize('kind', ['reference', 'custom'])
@pytest.mark.parametrize('q_len', SHAPES, ids=lambda q: 'x'.join(str(v) for v in q))
def test_random_queue_sets(q_len, kind, warm):
    c = _case(q_len, kind, warm)
    n = int(np.prod(q_len))
    want = c['metrics']
    assert want.shape == (n,) and np.all(np.isfinite(want))
    with _handle(c['consts']) as kf:
        rank, digits, metric, n_valid, mt = kf.search_schedules(c['ev'], c['q_len'], c['ref'], c['init'], c['prev'],
                                                                metrics=True)
        plan = kf.schedule_plan(c['q_len'])
    got = mt.cpu().numpy()
    print(q_len, kind, 'warm' if warm else 'cold', 'metrics', _rel(got, want), 'gap', _gap(want))
    assert got.shape == (n,) and _rel(got, want) <= TOL
    assert n_valid == n and plan['n_free'] == n
    assert got[rank] == metric == got.min()           # the winner is the smallest of the device's own metrics,
    assert rank == int(np.argmin(got))                # at its first rank
    assert digits == so.digits_of(rank, q_len)
    if n > 1:
        assert _gap(want) >= MARGIN['f64']            # a condition on the seed
        assert rank == so.winner(want)[0]


# ---------------------------------------------------------------------------------------------
# 3. ties, NaN and inf
# ---------------------------------------------------------------------------------------------
TIE_SHAPE = (3, 4, 2)


def _tie_case():
    c = _case(TIE_SHAPE, 'reference', False)
    return c, np.concatenate([[0], np.cumsum(TIE_SHAPE)])


def _digit(ranks, w, shape=TIE_SHAPE):
    return np.array([so.digits_of(int(r), shape)[w] for r in ranks])


def test_identical_candidates_tie_to_the_smaller_rank():
    c, off = _tie_case()
    ev, ref = c['ev'].copy(), c['ref'].copy()
    ev[off[1]:off[2]] = ev[off[1]]                    # window 1: four copies of its first candidate
    ref[off[1]:off[2]] = ref[off[1]]
    with _handle() as kf:
        rank, digits, metric, n_valid, mt = kf.search_schedules(ev, c['q_len'], ref, c['init'], c['prev'], metrics=True)
    got = mt.cpu().numpy().reshape(TIE_SHAPE)
    assert n_valid == got.size
    for d in range(1, 4):                             # the twins' metrics are the same bits
        assert np.array_equal(got[:, d, :], got[:, 0, :])
    assert digits[1] == 0 and metric == got.min()
    assert rank == int(np.argmin(got.reshape(-1)))    # argmin: the first of the equal minima


def test_nan_candidate_poisons_exactly_its_schedules():
    c, off = _tie_case()
    want = c['metrics']
    assert _gap(want) >= MARGIN['f64']
    best = so.winner(want)[0]
    d = (so.digits_of(best, TIE_SHAPE)[1] + 1) % TIE_SHAPE[1]     # a candidate of window 1 off the winner's path
    ev = c['ev'].copy()
    row = off[1] + d
    ev[row, 2 if ev[row, 1] == ref15.GPS else 8] = NAN            # a fix's easting, or an IMU sample's ax
    with _handle() as kf:
        rank, _, metric, n_valid, mt = kf.search_schedules(ev, c['q_len'], c['ref'], c['init'], c['prev'], metrics=True)
    got = mt.cpu().numpy()
    through = _digit(range(len(got)), 1) == d
    assert through.sum() == 6
    assert np.all(np.isnan(got[through])) and np.all(np.isfinite(got[~through]))
    assert _rel(got[~through], want[~through]) <= TOL
    assert n_valid == len(got) - 6
    assert rank == best and _rel(metric, want[best]) <= TOL


def test_infinite_metric_never_wins_and_is_not_counted():
    c, off = _tie_case()
    ev = c['ev'].copy()
    row = off[2] + 1                                              # the last window's second candidate
    ev[row, 2 if ev[row, 1] == ref15.GPS else 8] = 1e200          # its squared position error overflows
    with _handle() as kf:
        rank, digits, metric, n_valid, mt = kf.search_schedules(ev, c['q_len'], c['ref'], c['init'], c['prev'],
                                                                metrics=True)
    got = mt.cpu().numpy()
    through = _digit(range(len(got)), 2) == 1
    assert _gap(c['metrics'][~through]) >= MARGIN['f64']
    assert np.all(np.isinf(got[through])) and np.all(np.isfinite(got[~through]))
    assert n_valid == int((~through).sum()) and digits[2] == 0 and np.isfinite(metric)
    assert rank == so.winner(c['metrics'][~through])[0] * 2       # the other candidate's ranks are the even ones


def test_a_window_of_nan_candidates_has_no_winner():
    c, off = _tie_case()
    ev = c['ev'].copy()
    ev[off[1]:off[2], 2:] = NAN
    with _handle() as kf:
        rank, digits, metric, n_valid, mt = kf.search_schedules(ev, c['q_len'], c['ref'], c['init'], c['prev'],
                                                                metrics=True)
    assert rank is None and digits is None and metric == float('inf') and n_valid == 0
    assert bool(torch.isnan(mt).all())


# ---------------------------------------------------------------------------------------------
# 4. classes
# ---------------------------------------------------------------------------------------------
CLASS_SHAPE = (4, 3, 5, 2)


@pytest.mark.parametrize('kind', ['reference', 'custom'])
def test_classes_equal_the_whole_search(kind):
    c = _case(CLASS_SHAPE, kind, True)
    args = (c['ev'], c['q_len'], c['ref'], c['init'], c['prev'])
    with _handle(c['consts']) as kf:
        rank, digits, metric, n_valid, mt = kf.search_schedules(*args, metrics=True)
        whole = mt.cpu().numpy()
        assert _gap(whole) >= MARGIN['f64']
        for n_fixed in (1, 2, 4):
            n_free = int(np.prod(CLASS_SHAPE[n_fixed:]))
            buf = torch.full((whole.size,), NAN, dtype=torch.float64, device=kf.device)
            best, valid = (float('inf'), None, None), 0
            for k, fixed in enumerate(np.ndindex(*CLASS_SHAPE[:n_fixed])):
                r, dg, m, nv, _ = kf.search_schedules(*args, fixed=fixed, metrics=buf[k * n_free:(k + 1) * n_free])
                assert dg[:n_fixed] == tuple(fixed) and kf.schedule_plan(c['q_len'], n_fixed)['n_free'] == n_free
                valid += nv
                if m < best[0]:
                    best = (m, k * n_free + r, dg)
            print(kind, 'n_fixed', n_fixed, 'classes vs whole', _rel(buf.cpu().numpy(), whole))
            assert _rel(buf.cpu().numpy(), whole) <= KERNELS
            assert valid == n_valid == whole.size
            assert best[1] == rank and best[2] == digits and _rel(best[0], metric) <= KERNELS


def test_driver_splits_a_search_that_does_not_fit():
    events = _events(3)
    with _handle() as kf:
        q = [len(w) for w in ref15.schedule_queues(events, 0, 31, 50.0)]
        fits = kf.schedule_plan(q)['workspace_bytes']
    assert q == [5, 4, 3, 4, 4, 4]
    whole = ref15.search_schedules(events, 0, 31, 50.0, metrics=True)
    split = ref15.search_schedules(events, 0, 31, 50.0, metrics=True, mem_bytes=fits - 1)
    assert whole['n_fixed'] == 0 and split['n_fixed'] >= 1
    assert _gap(whole['metrics'].cpu().numpy()) >= MARGIN['f64']
    assert _rel(split['metrics'].cpu().numpy(), whole['metrics'].cpu().numpy()) <= KERNELS
    for k in ('rank', 'digits', 'n_valid', 'n_schedules', 'q_len'):
        assert split[k] == whole[k], k
    assert [e[0] for e in split['selected_sensors']] == [e[0] for e in whole['selected_sensors']]
    for k in ('trajectory', 'final_state', 'final_covariance', 'accuracy_metric'):
        assert _rel(np.array(split[k]), np.array(whole[k])) <= KERNELS, k
    # and against the oracle
    qs = so.queues(events, 0, 31, 50.0)
    want, states = so.metrics(qs, *so.fixes(events), with_states=True)
    assert _rel(whole['metrics'].cpu().numpy(), want) <= TOL and whole['rank'] == so.winner(want)[0]
    traj, x, P = states[whole['rank']]
    assert max(_rel(np.array(whole['trajectory']), traj), _rel(whole['final_state'], x),
               _rel(whole['final_covariance'], P)) <= TOL


def test_ranks_past_32_bits():
    """2^33 schedules in one call (23 windows of 2 candidates, one of 1024): the last level's ranks
    need 64 bits, and the call takes the kernel's 64-bit index arithmetic (a level of at most
    2^32 - 1 nodes takes the 32-bit one).  The first window's first candidate is NaN, so half of
    the schedules are not counted and the winner's rank is at least 2^32.  It is the reduced
    winner of the four classes of 2^31 schedules (32-bit arithmetic; the same step function, so
    the same bits), and the winner's own schedule, every window fixed, scores the same metric.
    About 0.3 s a pass over the 2^33."""
    shape = (2,) * 23 + (1024,)
    et, _, pay, _ = _stream(1100, 5)
    t = 1000.0 + np.arange(1100) * 0.005
    ev = np.zeros((sum(shape), 11))
    ev[:, 0], ev[:, 1], ev[:, 2:] = t[:len(ev)], et[:len(ev)], pay[:len(ev)]
    assert ev[0, 1] == ref15.GPS
    ev[0, 2] = NAN      # the first window's first candidate: ranks below 2^32 score NaN, so the winner lies past them
    g = et == ref15.GPS
    ref = ref15.track_positions(t[g], pay[g, 0:3], ev[:, 0])
    init = np.concatenate([np.zeros(15), ref15.to_blocks(so.P0)])
    args = (ev, np.array(shape, np.int32), ref, init)
    n = 1 << 33
    with _handle() as kf:
        plan = kf.schedule_plan(shape)
        assert plan == {'n_free': n, 'widest': 1 << 23, 'workspace_bytes': plan['workspace_bytes']}
        rank, digits, metric, n_valid, _ = kf.search_schedules(*args)
        assert n_valid == n // 2 and rank >= 1 << 32 and digits == so.digits_of(rank, shape)
        best = (float('inf'), None, None)
        for k, fixed in enumerate(np.ndindex(2, 2)):
            r, dg, m, nv, _ = kf.search_schedules(*args, fixed=fixed)
            assert nv == (0 if fixed[0] == 0 else n // 4) and (r is None) == (fixed[0] == 0)
            if m < best[0]:
                best = (m, k * (n // 4) + r, dg)
        print('2^33 schedules: rank', rank, 'metric', metric, 'classes', best[:2])
        assert best == (metric, rank, digits)
        one = kf.search_schedules(*args, fixed=digits, metrics=True)
        assert one[0] == 0 and one[2] == metric and float(one[4][0]) == metric


# ---------------------------------------------------------------------------------------------
# 5. determinism
# ---------------------------------------------------------------------------------------------
def test_the_same_call_twice_is_bit_for_bit():
    c = _case((4, 4, 4, 4, 3, 3), 'reference', False)
    args = (c['ev'], c['q_len'], c['ref'], c['init'], c['prev'])
    with _handle() as kf:
        a = kf.search_schedules(*args, metrics=True)
        b = kf.search_schedules(*args, metrics=True)
    assert a[:4] == b[:4] and torch.equal(a[4], b[4])


# ---------------------------------------------------------------------------------------------
# 6. errors
# ---------------------------------------------------------------------------------------------
def _refused(kf, text, ev, q_len, ref, init, prev=NAN, fixed=()):
    x0, P0 = (t.clone() for t in kf.state())
    st0 = kf.status().clone()
    with pytest.raises(kfmi.KFError) as e:
        kf.search_schedules(ev, q_len, ref, init, prev, fixed=fixed, metrics=True)
    assert e.value.code == _lib.KF_EINVAL and text in str(e.value), (text, str(e.value))
    x1, P1 = kf.state()
    assert torch.equal(x0, x1) and torch.equal(P0, P1) and torch.equal(st0, kf.status())


def test_errors_are_einval_with_their_text():
    c, off = _tie_case()
    good = (c['ev'], c['q_len'], c['ref'], c['init'])
    for model, dtype, text in (('ref15', 'f32', 'f64 handle'), ('cv3', 'f64', 'KF_MODEL_REF15'),
                               ('ref8', 'f64', 'KF_MODEL_REF15')):
        with kfmi.BatchedKF(model, 4, dtype) as other:
            _refused(other, text, *good)
    with _handle() as kf:
        _refused(kf, 'q_len[1] = 0', c['ev'][:5], np.array([3, 0, 2], np.int32), c['ref'][:5], c['init'])
        _refused(kf, 'fixed[1] = 4', *good, fixed=(1, 4))
        _refused(kf, 'fixed[0] = -1', *good, fixed=(-1,))
        swapped = np.concatenate([c['ev'][off[1]:off[2]], c['ev'][off[0]:off[1]], c['ev'][off[2]:]])
        _refused(kf, 'window 1 has a candidate', swapped, np.array([4, 3, 2], np.int32), c['ref'], c['init'])
        _refused(kf, 'earlier than prev_time', *good, prev=float(c['ev'][0, 0]) + 1e-3)
        bad = c['ev'].copy()
        bad[4, 1] = 2
        _refused(kf, 'window 1 candidate 1 has type 2', bad, *good[1:])
        bad = c['ev'].copy()
        bad[8, 0] = NAN
        _refused(kf, 'window 2 candidate 1 has time', bad, *good[1:])
        # inside a graph capture (torch captures on a side stream); the capture ends before the asserts
        x = torch.zeros(4, device=kf.device)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        err = None
        with torch.cuda.graph(g):
            x += 1
            try:
                kf.search_schedules(*good)
            except kfmi.KFError as e:
                err = e
        assert err is not None and err.code == _lib.KF_EINVAL and 'capturable' in str(err)
        g.replay()
        torch.cuda.synchronize()
        assert float(x[0]) == 1.0
        # a correct call afterwards works
        rank, _, metric, n_valid, _ = kf.search_schedules(*good)
        assert n_valid == 24 and _rel(metric, c['metrics'][rank]) <= TOL
