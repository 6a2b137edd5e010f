"""The experiment loop's windows as batches — needs an MI355X.

kf_run_events_gates (BatchedKF.run_events_gates): per-filter streams under per-filter gates, so
the loop's full, adaptive and no-update filters of many windows share a launch.
kf_search_windows (BatchedKF.search_windows): many windows' brute-force searches in one launch.
kfmi.ref15.run_window_batch: the loop's window phase (kf_workers.py:2320-2345) on both.

Shapes are the smallest at which the kernels can still go wrong (partial waves and 8-lane
groups, more than one workgroup, the chain kernel's x2 unroll, several subset sizes in one wave),
not the workload's.
"""
import ctypes
from itertools import combinations

import numpy as np
import pytest
import torch

import bench
import kfmi
from kfmi import _lib, ref15
from oracle import ref_kf
from test_gpu_sweep import MARGIN, TOL, KERNELS, _golden, _list_arrays, _rel, _symmetric_consts, gate_margins

pytestmark = pytest.mark.gpu
INF = float('inf')
NAN = float('nan')


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---------------------------------------------------------------------------------------------
# 1. per-filter gates equal the scalar runs, bit for bit
# ---------------------------------------------------------------------------------------------
# finite thresholds inside the log-det range of a short run from the reset covariance (117.4 for
# ref15, 46.1 for ref8, falling with every update), so their gates open for some events only
FINITE = {'ref15': (60.0, 20.0), 'ref8': (30.0, 10.0)}
BATCHES = (1, 7, 8, 9, 64, 65, 130)
LDS_BATCHES = (16, 64, 80)
LENGTHS = (1, 2, 3, 25)
SCALE = np.array([20, 20, 20, 0.05, 0.05, 0.05, 0.5, 0.5, 0.5])


def _ragged(B, T, n, seed):
    """B ragged per-filter streams of at most T events, NONE-padded; filter 0 has all T."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, T + 1, B)
    lens[0] = T
    live = np.arange(T)[:, None] < lens[None, :]
    et = np.where(live, rng.choice([ref15.GPS, ref15.IMU, ref15.IMU, ref15.PREDICT], (T, B)), ref15.NONE).astype(np.uint8)
    dt = np.where(live, rng.uniform(0.001, 0.05, (T, B)), 0.0)
    pay = rng.normal(0, 1, (T, 9, B)) * SCALE[None, :, None]
    return et, dt, pay, rng.normal(0, 1, (n, B))


def _records(kf, x0, P0, run):
    kf.set_state(x0, P0)
    tr, ld, up, cv = run()
    x, P = kf.state()
    out = dict(traj=tr, cov=cv, logdet=ld, updated=up, x=x, P=P, status=kf.status())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize('kernel', ['lane', 'chain', 'lds'])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_gates_equal_scalar_runs_bitwise(model, dtype, kernel):
    """Thresholds cycling through {-inf, t1, t2, +inf, NaN} over the filters: the columns holding
    one threshold equal, in every record, the final state and the status, kf_run_events_seq on
    the same handle with that scalar (gate = 0 for -inf).  Same kernel, same operands: no
    tolerance.  The LDS kernel is legal for B % 16 == 0 only: B = 16 and 80 (a partial wave, whose
    dead lanes read the last filter's threshold) and 64."""
    t1, t2 = FINITE[model]
    cycle = [-INF, t1, t2, INF, NAN]
    npd = np.float64 if dtype == 'f64' else np.float32
    seen = set()
    for B in (LDS_BATCHES if kernel == 'lds' else BATCHES):
        kf = kfmi.BatchedKF(model, B, dtype, options={'events_kernel': kernel})
        P0 = kf.state()[1].cpu().numpy()
        thr = np.array([cycle[f % 5] for f in range(B)])
        for T in LENGTHS:
            et, dt, pay, x0 = _ragged(B, T, kf.n, 1000 * B + T)
            pay, x0 = pay.astype(npd), x0.astype(npd)
            got = _records(kf, x0, P0, lambda: kf.run_events_gates(et, dt, pay, thr, updated=True, cov=True))
            for j, v in enumerate(cycle[:min(5, B)]):
                cols = np.arange(j, B, 5)
                want = _records(kf, x0, P0, lambda: kf.run_events(et, dt, pay, updated=True, cov=True, sequential=True,
                                                                  threshold=None if j == 0 else v))
                for k in got:
                    assert np.array_equal(_bits(got[k][..., cols]), _bits(want[k][..., cols])), (B, T, v, k)
                events = (et[:, cols] == ref15.GPS) | (et[:, cols] == ref15.IMU)
                flags = got['updated'][:, cols][events]
                if j == 0:
                    assert flags.all()
                elif j >= 3:
                    assert not flags.any()
                else:
                    seen.update(flags.tolist())
        kf.close()
    assert seen == {0, 1}   # the finite gates opened for some events and stayed shut for others


def test_gates_argument_errors():
    """KF_OPT_EVENTS_KERNEL = 4 (the one-filter look-ahead kernel), null thresholds and a cv3
    handle are KF_EINVAL with their text; nothing is launched."""
    et, dt, pay, x0 = _ragged(1, 3, 15, 1)
    kf = kfmi.BatchedKF('ref15', 1, 'f64')
    kf.set_state(x0, kf.state()[1])
    x_in = kf.state()[0].cpu().numpy()
    L = _lib.lib()
    d = kf.device
    e, t, p = (torch.as_tensor(v, device=d) for v in (et, dt, pay))
    assert L.kf_run_events_gates(kf.handle, 3, e.data_ptr(), t.data_ptr(), p.data_ptr(), None, None, None, None, None,
                                 kf._stream()) == _lib.KF_EINVAL
    assert 'null thresholds' in _lib.last_error()
    kf.set_option('events_kernel', 'gated')
    with pytest.raises(kfmi.KFError) as err:
        kf.run_events_gates(et, dt, pay, np.array([0.0]))
    assert err.value.code == _lib.KF_EINVAL and 'KF_OPT_EVENTS_KERNEL = 4' in str(err.value)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(kf.state()[0].cpu().numpy(), x_in)
    kf.close()
    cv = kfmi.BatchedKF('cv3', 1, 'f64')
    with pytest.raises(ValueError):
        cv.run_events_gates(et, dt, pay, np.array([0.0]))
    cv.close()


# ---------------------------------------------------------------------------------------------
# 2. gates against the oracle
# ---------------------------------------------------------------------------------------------
# cold-start windows of the golden stream and one threshold each; margins measured on the CPU with
# the oracle's matrices: 0.0124, 0.0321, 0.0117, 0.0523, 2.3955, 0.0155
ORACLE_WINDOWS = [((0, 60), -33.01), ((3, 110), 2.77), ((40, 200), -17.24), ((100, 260), -36.4),
                  ((150, 427), 20.9), ((0, 427), -36.75)]


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_gates_vs_oracle(golden_dir, dtype):
    """B = 12 filters in one launch: six windows of the golden stream under their adaptive
    thresholds (oracle.ref_kf.run_adaptive_threshold) and the same six as no-update filters
    (run_no_update: KF_EVENT_PREDICT events, gate -inf).  Every threshold must meet the margin
    rule for the dtype (a condition on the inputs: none is dropped).  Flags equal in both dtypes;
    records within TOL in f64 (tests/test_gpu_sweep.py's bound against the oracle; it has none for
    f32 against the fp64 oracle, and test_gates_equal_scalar_runs_bitwise ties the f32 records to
    the scalar kernel's)."""
    _, events = _golden(golden_dir)
    arrays = [_list_arrays(events, s, e) for (s, e), _ in ORACLE_WINDOWS]
    for (et, dt, _, _), (_, thr) in zip(arrays, ORACLE_WINDOWS):
        margin, _, _, _ = gate_margins(et, dt, [thr])
        assert margin[0] >= MARGIN[dtype], (thr, margin)
    W = len(arrays)
    L = 1 + max(len(a[0]) for a in arrays)   # a leading NONE entry records the initial state
    et = np.full((L, 2 * W), ref15.NONE, np.uint8)
    dt = np.zeros((L, 2 * W))
    pay = np.zeros((L, 9, 2 * W))
    x0 = np.zeros((15, 2 * W))
    for w, (e, d, p, x) in enumerate(arrays):
        n = len(e)
        et[1:n + 1, w], dt[1:n + 1, w], pay[1:n + 1, :, w], x0[:, w] = e, d, p, x
        et[1:n + 1, W + w] = np.where(e != ref15.NONE, ref15.PREDICT, ref15.NONE)
        dt[1:n + 1, W + w], x0[:, W + w] = d, x
    gates = np.array([thr for _, thr in ORACLE_WINDOWS] + [-INF] * W)
    npd = np.float64 if dtype == 'f64' else np.float32
    kf = kfmi.BatchedKF('ref15', 2 * W, dtype)
    kf.set_state(x0.astype(npd), kf.state()[1])
    tr, ld, up, _ = kf.run_events_gates(et, dt, pay.astype(npd), gates, updated=True)
    Pb = kf.state()[1].double().cpu().numpy()
    assert int(kf.status().abs().sum()) == 0
    tr, ld, up = tr.cpu().numpy(), ld.cpu().numpy(), up.cpu().numpy()
    kf.close()
    for w, ((s, e), thr) in enumerate(ORACLE_WINDOWS):
        first = next(i for i in range(s, e) if events[i][1] == 'GPS')
        t = np.array([ev[2] for ev in events[first:e]])
        for col, want in ((w, ref_kf.run_adaptive_threshold(events, s, e, R_threshold=thr)),
                          (W + w, ref_kf.run_no_update(events, s, e))):
            st, lds, P, prev, times = want
            keep = et[:, col] != ref15.NONE
            keep[0] = True
            states = np.column_stack([np.concatenate([[t[0]], t])[keep[:len(t) + 1]], tr[keep, :, col]])
            assert states.shape == np.array(st).shape, (w, col)
            if dtype == 'f64':
                assert _rel(states, st) <= TOL and _rel(ld[keep, col], lds) <= TOL, (w, col)
                assert _rel(ref15.from_blocks(Pb[:, col]), P) <= TOL, (w, col)
            flagged = up[1:len(t) + 1, col].astype(bool) & keep[1:len(t) + 1]
            np.testing.assert_array_equal(np.concatenate([[t[0]], t[flagged]]), np.array(times), err_msg=str((w, col)))
            if col >= W:
                assert len(times) == 1   # run_no_update: the cold start's fix only


# ---------------------------------------------------------------------------------------------
# 3. many windows in one search
# ---------------------------------------------------------------------------------------------
SIZES = (12, 5, 1, 2, 12, 8, 5, 12)   # per-window candidates, cycled; n = 12 puts two sizes into one wave
N_MAX = 12
N_WINDOWS = 65
GAP = {'f64': 1e-9, 'f32': 1e-4}
_cache = {}


def _window_inputs():
    """65 windows: bench.bf_events' candidates (their own seed each) with the target half a second
    past the last one, so that a subset's score is its final predict's log-det and differs from
    subset to subset; each window's root covariance is bf_events' scaled by its own factor (equal
    on the three axes, so the axis-symmetric search applies)."""
    if 'inputs' not in _cache:
        ev = np.zeros((N_WINDOWS, N_MAX, 11))
        ev[:, :, 1] = 7   # rows past a window's n are never read: an illegal type would be refused
        init, prev, tend, ns = np.zeros((N_WINDOWS, 42)), np.zeros(N_WINDOWS), np.zeros(N_WINDOWS), []
        for w in range(N_WINDOWS):
            n = SIZES[w % len(SIZES)]
            e, ini, Pw, t0, t_end = bench.bf_events(n, seed=500 + w)
            ev[w, :n] = e
            init[w] = np.concatenate([np.zeros(15), ref15.to_blocks(Pw * (1.0 + 0.03 * w))])
            prev[w], tend[w] = t0, t_end + 0.5
            ns.append(n)
        _cache['inputs'] = (ev, init, prev, tend, np.array(ns, np.int32))
    return _cache['inputs']


CONFIGS = {
    'every_chain': dict(dtype='f64', options={'axis_sym': 'off'}, consts=None),
    'default': dict(dtype='f64', options=None, consts=None),
    'custom': dict(dtype='f64', options=None, consts=('ref15', 9)),
    'default_f32': dict(dtype='f32', options=None, consts=None),
}


def _search_handle(cfg):
    c = CONFIGS[cfg]
    params = _symmetric_consts(*c['consts']).params() if c['consts'] else None
    return kfmi.BatchedKF('ref15', 1, c['dtype'], options=c['options'], params=params)


def _pick_threshold(scores, target, gap):
    """A threshold midway between two neighbouring distinct scores whose relative gap is at
    least ``gap``, the pair nearest position ``target`` (0 .. 1) of the sorted scores; target < 0:
    below every score."""
    s = np.unique(scores[np.isfinite(scores)])
    if target < 0 or len(s) < 2:
        return float(s[0] - 0.01 * max(1.0, abs(s[0]))) if target < 0 else float(s[-1] + 0.01 * max(1.0, abs(s[-1])))
    ok = np.nonzero((s[1:] - s[:-1]) >= gap * np.maximum(np.abs(s[1:]), np.abs(s[:-1])))[0]
    assert len(ok), 'no two scores far enough apart'
    i = ok[np.argmin(np.abs(ok - target * (len(s) - 2)))]
    return float(0.5 * (s[i] + s[i + 1]))


def _reference(cfg, k_max):
    """Per window: its threshold (from an exhaustive one-window search's subset scores) and
    kf_search_combos' (k_found, winner mask, n_accepted) on that window alone.  Once per
    (configuration, k_max)."""
    key = (cfg, k_max)
    if key not in _cache:
        ev, init, prev, tend, ns = _window_inputs()
        kf = _search_handle(cfg)
        # where the threshold sits among a window's scores: accept everything (the winner is
        # rank 0 of size 1), nothing, or a part
        targets = (2.0, -1.0, 0.5, 0.15, 0.03, 0.3, 0.8, 0.08)
        thr, kf_, win, acc = np.zeros(N_WINDOWS), np.zeros(N_WINDOWS, np.int32), [], np.zeros((N_WINDOWS, k_max + 1), np.uint64)
        for w in range(N_WINDOWS):
            n = int(ns[w])
            kk = min(k_max, n)
            _, _, _, sm = kf.search_combos(ev[w, :n], init[w], prev[w], tend[w], -1e30, k_max=kk, exhaustive=True,
                                           subset_max=True)
            sm = sm.double().cpu().numpy()
            sized = np.array([bin(m).count('1') for m in range(1 << n)])
            scores = sm[(sized >= 1) & (sized <= kk)]
            assert np.isfinite(scores).all()
            t = targets[(w // len(SIZES) + w) % len(targets)]
            thr[w] = _pick_threshold(scores, t, GAP[CONFIGS[cfg]['dtype']]) if t <= 1 else float(scores.max() + 1.0)
            k, idx, a, _ = kf.search_combos(ev[w, :n], init[w], prev[w], tend[w], thr[w], k_max=kk)
            kf_[w] = k
            win.append(idx)
            acc[w, :kk + 1] = a
        kf.close()
        _cache[key] = (thr, kf_, win, acc)
    return _cache[key]


@pytest.mark.parametrize('W', [1, 2, N_WINDOWS])
@pytest.mark.parametrize('k_max', [1, 3, 4])
@pytest.mark.parametrize('cfg', sorted(CONFIGS))
def test_search_windows_equal_one_window_searches(cfg, k_max, W):
    """k_found, winner and n_accepted of every window equal kf_search_combos on that window
    alone (k_max clamped to the window's n: windows of 1 and 2 candidates are in every call),
    with KF_OPT_AXIS_SYM = 1, by default on axis-symmetric inits, with custom constants, in f32."""
    ev, init, prev, tend, ns = _window_inputs()
    thr, want_k, want_win, want_acc = _reference(cfg, k_max)
    kf = _search_handle(cfg)
    k, masks, acc = kf.search_windows(ev[:W], init[:W], prev[:W], tend[:W], thr[:W], k_max, n_events=ns[:W])
    kf.close()
    np.testing.assert_array_equal(k, want_k[:W])
    got_win = [tuple(i for i in range(int(ns[w])) if (int(masks[w]) >> i) & 1) if k[w] else None for w in range(W)]
    assert got_win == want_win[:W]
    np.testing.assert_array_equal(acc, want_acc[:W])
    if W == N_WINDOWS and k_max >= 3 and cfg == 'default':
        # a condition on the inputs: the winners cover what the kernel can get wrong
        assert {0, 1, 2, 3} <= set(want_k.tolist())
        ranks = [(list(combinations(range(int(ns[w])), len(c))).index(c), len(list(combinations(range(int(ns[w])), len(c)))))
                 for w, c in enumerate(want_win) if c]
        assert any(r == 0 for r, _ in ranks) and any(0 < r < m - 1 for r, m in ranks)


def test_search_windows_vs_oracle():
    """Three windows of 8 candidates, sizes up to 3: the winner equals
    oracle.ref_kf.run_brute_force's (the reference's serial search in NumPy).  The last candidate
    lies half a second after the others, so the window's target (its last event's time, as the
    reference sets it) is far from every other subset's end and the scores differ."""
    W, n = 3, 8
    ev, init, prev, tend, lists = np.zeros((W, n, 11)), np.zeros((W, 42)), np.zeros(W), np.zeros(W), []
    for w in range(W):
        e, ini, Pw, t0, _ = bench.bf_events(n, seed=900 + w)
        e[n - 1, 0] += 0.5
        ev[w], init[w], prev[w], tend[w] = e, ini, t0, e[n - 1, 0]
        lists.append([(i, 'GPS', float(e[i, 0]), {'easting': e[i, 2], 'northing': e[i, 3], 'altitude': e[i, 4]})
                      if e[i, 1] == ref15.GPS else (i, 'IMU', float(e[i, 0]), [repr(e[i, 0]), *e[i, 2:]])
                      for i in range(n)])
    kf = _search_handle('default')
    thr = np.zeros(W)
    sized = np.array([bin(m).count('1') for m in range(1 << n)])
    for w, target in enumerate((0.5, 0.1, 0.03)):
        _, _, _, sm = kf.search_combos(ev[w], init[w], prev[w], tend[w], -1e30, k_max=3, exhaustive=True, subset_max=True)
        thr[w] = _pick_threshold(sm.cpu().numpy()[(sized >= 1) & (sized <= 3)], target, GAP['f64'])
    k, masks, _ = kf.search_windows(ev, init, prev, tend, thr, 3)
    kf.close()
    for w in range(W):
        P = ref15.from_blocks(init[w, 15:])
        best = ref_kf.run_brute_force(lists[w], 0, n, thr[w], P, (float(prev[w]), *init[w, 0:6]))
        want = tuple(c[0] for c in best['selected_sensors'])
        assert 1 <= len(want) <= 3, want   # the threshold lies above a score of these sizes
        assert want == tuple(i for i in range(n) if (int(masks[w]) >> i) & 1) and k[w] == len(want), (w, want)


def test_search_windows_limits():
    """Each limit is KF_EINVAL with its text and launches nothing; inside a graph capture the
    call is KF_EINVAL; a correct call afterwards works."""
    ev, init, prev, tend, ns = _window_inputs()
    thr, want_k, _, _ = _reference('default', 3)
    kf = _search_handle('default')
    L = _lib.lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    win, kfound = np.zeros(4, np.uint64), np.zeros(4, np.int32)

    def call(W=2, n_max=N_MAX, k_max=3, n_events=ns, events=ev):
        return L.kf_search_windows(kf.handle, W, n_max, vp(np.ascontiguousarray(n_events)), vp(events), vp(init),
                                   vp(prev), vp(tend), vp(thr), k_max, vp(win), vp(kfound), None, kf._stream())
    bad_n = ns.copy()
    bad_n[1] = N_MAX + 1
    bad_ev = ev.copy()
    bad_ev[0, 3, 1] = 2
    for kw, text in ((dict(W=0), 'W = 0'), (dict(n_max=65), 'n_max = 65'), (dict(n_max=0), 'n_max = 0'),
                     (dict(k_max=0), 'k_max = 0'), (dict(k_max=9), 'k_max = 9'),
                     (dict(n_events=bad_n), 'n_events[1] = 13'), (dict(events=bad_ev), 'window 0 event 3 has type 2')):
        assert call(**kw) == _lib.KF_EINVAL, text
        assert text in _lib.last_error(), (text, _lib.last_error())
    # W x the widest window's subsets: 40 windows of 64 candidates at k_max = 6 hold 8.3e7 each
    big_n = np.full(40, 64, np.int32)
    big_ev = np.zeros((40, 64, 11))
    big_ev[:, :, 1] = 1
    rc = L.kf_search_windows(kf.handle, 40, 64, vp(big_n), vp(big_ev), vp(np.zeros((40, 42))), vp(np.zeros(40)),
                             vp(np.ones(40)), vp(np.zeros(40)), 6, vp(np.zeros(40, np.uint64)), vp(np.zeros(40, np.int32)),
                             None, kf._stream())
    assert rc == _lib.KF_EINVAL and '2^31' in _lib.last_error()
    cvh = kfmi.BatchedKF('ref8', 1, 'f64')
    assert L.kf_search_windows(cvh.handle, 2, N_MAX, vp(ns), vp(ev), vp(init), vp(prev), vp(tend), vp(thr), 3, vp(win),
                               vp(kfound), None, cvh._stream()) == _lib.KF_EINVAL
    assert 'KF_MODEL_REF15' in _lib.last_error()
    cvh.close()
    x = torch.zeros(4, device=kf.device)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        x += 1
        rc = call()
    assert rc == _lib.KF_EINVAL and 'capturable' in _lib.last_error()
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    assert call() == _lib.KF_OK, _lib.last_error()
    np.testing.assert_array_equal(kfound[:2], want_k[:2])
    kf.close()


# ---------------------------------------------------------------------------------------------
# 4. the batch equals the loop
# ---------------------------------------------------------------------------------------------
SWEEP_THR = [-25.0, -11.4, 0.3]   # tests/test_gpu_sweep.py's WARM_THR (margins >= 1e-5 over the golden run)
RATIOS = (0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8)


def _tuple_close(a, b, n_arrays=3):
    for x, y in zip(a[:n_arrays], b[:n_arrays]):
        assert np.array(x).shape == np.array(y).shape
        assert _rel(x, y) <= KERNELS, _rel(x, y)
    assert list(a[n_arrays:]) == list(b[n_arrays:])


def _bf_close(a, b):
    assert (a is None) == (b is None)
    if a is None:
        return
    assert [e[0] for e in a['selected_sensors']] == [e[0] for e in b['selected_sensors']]
    assert a['num_measurements_used'] == b['num_measurements_used']
    for k in ('log_determinants', 'final_state', 'trajectory'):
        assert np.array(a[k]).shape == np.array(b[k]).shape, k
        assert _rel(a[k], b[k]) <= KERNELS, (k, _rel(a[k], b[k]))


def _check_batch(events, starts, ends):
    """run_window_batch over the windows (warm starts from one AdaptiveSweep, the loop's ratios)
    against the four single drivers per window."""
    margin, _, _, _ = gate_margins(*_list_arrays(events)[:2], SWEEP_THR)
    assert np.all(margin >= MARGIN['f64']), margin
    sw = ref15.AdaptiveSweep(events, SWEEP_THR, 0, len(events), checkpoint_every=64, records=False)
    warm = [sw.warm_start(w % 3, s) for w, s in enumerate(starts)]
    sw.close()
    W = len(starts)
    states, Ps = [x[0] for x in warm], [x[1] for x in warm]
    ratios = [RATIOS[w % 7] for w in range(W)]
    batch = ref15.run_window_batch(events, starts, ends, Ps, states, ratios=ratios, k_max=4)
    assert len(batch) == W and int(np.abs(batch.status).sum()) == 0
    for w, (s, e) in enumerate(zip(starts, ends)):
        kw = dict(initial_pt=Ps[w], initial_state=states[w])
        full = ref15.run_kalman_filter_full(events, s, e, **kw)
        thr = ratios[w] * min(full[1])
        adaptive = ref15.run_adaptive_threshold_kalman_filter(events, s, e, R_threshold=thr, **kw)
        bf = ref15.run_brute_force_kalman_filter_no_sampling_min_usage(events, s, e, R_threshold=thr, **kw)
        no_update = ref15.run_no_update_kalman_filter(events, s, e, R_threshold=thr, **kw)
        got = batch[w]
        assert 2 <= len(got['full'][0]) <= 1 + min(e, len(events)) - s
        assert abs(got['threshold'] - thr) <= KERNELS * abs(thr)
        _tuple_close(got['full'], full)
        _tuple_close(got['adaptive'], adaptive)
        _tuple_close(got['no_update'], no_update)
        _bf_close(got['brute_force'], bf)
        n_bf = len(bf['selected_sensors']) if bf else 0
        assert batch.k_found[w] == (n_bf if n_bf <= 4 else 0)
        if batch.k_found[w]:
            assert batch.winners[w] == tuple(ev[0] - s for ev in bf['selected_sensors'])
    assert [r['threshold'] for r in batch[:]] == [float(t) for t in batch.thresholds]


def test_window_batch_equals_the_loop(golden_dir):
    """Twenty 25-event windows of the golden stream through run_window_batch and through
    run_kalman_filter_full, run_adaptive_threshold_kalman_filter,
    run_brute_force_kalman_filter_no_sampling_min_usage and run_no_update_kalman_filter per
    window: equal flags (measurement times), winners and sizes; full, adaptive and no-update
    records, and the winners' log-determinants, within 1e-9 relative."""
    _, events = _golden(golden_dir)
    starts = [30 + 19 * w for w in range(20)]
    ends = [s + 25 for s in starts]
    assert ends[-1] <= len(events)
    _check_batch(events, starts, ends)


def test_window_batch_of_unequal_windows(golden_dir):
    """Windows of 25, 7, 12, 3 and 1 events and one whose end lies past the stream's (clipped to
    its last 10 events), in one batch: every window against the four single drivers, the shorter
    ones' records ending where their window does."""
    _, events = _golden(golden_dir)
    n = len(events)
    starts = [40, 120, 250, 300, 350, n - 10]
    ends = [65, 127, 262, 303, 351, n + 15]
    _check_batch(events, starts, ends)


def test_window_batch_fallback(golden_dir):
    """A window whose threshold lies below every single event's score, searched with k_max = 1,
    reports k_found = 0 and goes through the one-window search:
    run_brute_force_kalman_filter_no_sampling_min_usage's result."""
    _, events = _golden(golden_dir)
    sw = ref15.AdaptiveSweep(events, SWEEP_THR, 0, len(events), checkpoint_every=64, records=False)
    s, e = 200, 212   # 12 candidates: every subset's score fits a 2^12 table
    state, P, _ = sw.warm_start(1, s)
    sw.close()
    _, _, _, prev, target_end, ev, init = ref15.brute_force_setup(events, s, e, P, state)
    kf = kfmi.BatchedKF('ref15', 1, 'f64')
    _, _, _, sm = kf.search_combos(ev, init, prev, target_end, -1e30, k_max=2, exhaustive=True, subset_max=True)
    kf.close()
    sm = sm.cpu().numpy()
    singles = sm[[1 << i for i in range(len(ev))]]
    pairs = sm[[(1 << i) | (1 << j) for i, j in combinations(range(len(ev)), 2)]]
    m1 = singles.min()
    lower = pairs[pairs < m1 - 1e-6 * abs(m1)]
    # below every single's score; above a pair's where one lies lower (the fallback then finds it)
    thr = 0.5 * (m1 + lower.max()) if len(lower) else m1 - 1.0
    batch = ref15.run_window_batch(events, [s], [e], [P], [state], thresholds=[thr], k_max=1)
    assert batch.k_found[0] == 0 and batch.fallback == [0]
    want = ref15.run_brute_force_kalman_filter_no_sampling_min_usage(events, s, e, R_threshold=thr, initial_pt=P,
                                                                     initial_state=state)
    _bf_close(batch[0]['brute_force'], want)
