"""The experiment loop's window phase (kf_workers.py:2320-2345: full, adaptive and no-update
filters and the brute-force search over a window of 25 events, 40 in the visualizing variant) as
one batch against one window after another, over the 583k-event synthetic drive log with the
loop's 284 start points and its thresholds lb x {0.2 .. 0.8}:

  (a) the four single drivers per window (run_kalman_filter_full, run_adaptive_threshold_kalman_filter,
      run_brute_force_kalman_filter_no_sampling_min_usage, run_no_update_kalman_filter), one window
      after another
  (b) ref15.run_window_batch over the same 284 windows
  (c) the 284 x 7 grid (every start point under every threshold ratio) in one batch
  (d) kf.search_windows alone against 284 kf.search_combos calls

The warm starts come from one AdaptiveSweep and are timed separately.  Each arm is warmed once,
then timed ``--runs`` times (``--slow-runs`` times where the warm call took over ``--slow-s``
seconds; wall clock around a synchronised call): every run, median, min and max per arm,
one JSON line each, then the ratios; (b)'s winners and sizes must equal (a)'s.  (b)'s host array
building and the per-window result dicts (built on access, outside (b)) are timed on their own.

    python tools/window_batch_timing.py [--T 583000] [--runs 5] [--windows 25 40] [--grid-windows 25]
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'sensorfusion-kalmanfilter_amd'), os.path.join(ROOT, 'tests')]
RATIOS = [0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=583000)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--windows', type=int, nargs='+', default=[25, 40])
    ap.add_argument('--grid-windows', type=int, nargs='*', default=[25],
                    help='window lengths that also run the 284 x 7 grid (c); at 40 events the windows without a '
                         'subset of at most k-max events go through the one-window search, ~0.5 s each')
    ap.add_argument('--slow-s', type=float, default=5.0, help='an arm whose warm call takes longer than this ...')
    ap.add_argument('--slow-runs', type=int, default=2, help='... is timed this many times instead of --runs')
    ap.add_argument('--k-max', type=int, default=4)
    ap.add_argument('--checkpoint-every', type=int, default=4096)
    args = ap.parse_args()
    import numpy as np
    import torch
    import kfmi
    from kfmi import ingest, ref15
    from kfmi import kf_workers as kfw
    from test_gpu_timeparallel import _stream
    T = args.T
    et, dt, pay, x0 = _stream(T, seed=11)
    dev = torch.device('cuda', 0)
    d_et, d_dt, d_pay = (torch.as_tensor(v, device=dev) for v in (et, dt, pay))
    t_abs = 1.7e9 + np.cumsum(dt)
    stream = ingest.EventStream(etype=d_et, t=torch.as_tensor(t_abs, device=dev), payload=d_pay,
                                src=torch.zeros(T, dtype=torch.int32, device=dev),
                                zone_number=torch.zeros(T, dtype=torch.int8, device=dev),
                                zone_letter=torch.zeros(T, dtype=torch.uint8, device=dev),
                                first_valid_index=0, gyro_bias=np.zeros(3), accel_bias=np.zeros(3),
                                utm_origin=np.zeros(2), n_fixes=int((et == 0).sum()), n_imu=int((et == 1).sum()))
    events = kfw.EventList(stream)

    def timed(fn, runs=args.runs):
        t = time.perf_counter()
        fn()  # warm
        torch.cuda.synchronize()
        if time.perf_counter() - t > args.slow_s:  # an arm of many seconds a run: fewer runs
            runs = min(runs, args.slow_runs)
        ms = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t) * 1e3)
        return out, ms

    def stats(name, ms, **kw):
        row = dict(arm=name, median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3),
                   max_ms=round(max(ms), 3), runs=len(ms), runs_ms=[round(m, 1) for m in ms], **kw)
        print(json.dumps(row), flush=True)
        return row

    # the loop's bound (:2301-2302) and its start points (:2306-2310): offsets of i * 2775 / 300 s
    n_lb = min(100000, T)
    _, ld_full, _, _ = ref15.run_kalman_filter_full(stream, 0, n_lb)
    lb = min(ld_full)
    span = (t_abs[-1] - t_abs[0]) / 2915.0   # the offsets scaled to a shorter --T
    starts = [int(np.searchsorted(t_abs - t_abs[0], int(i * (2800 - 25) / 300) * span)) for i in range(16, 300)]
    rng = random.Random(2025)
    draw = [rng.randrange(len(RATIOS)) for _ in starts]
    thr = [lb * r for r in RATIOS]
    print(json.dumps(dict(lb=lb, thresholds=thr, windows=len(starts), first_start=starts[0], last_start=starts[-1])),
          flush=True)
    t0 = time.perf_counter()
    sweep = ref15.AdaptiveSweep(stream, thr, records=False, checkpoint_every=args.checkpoint_every)
    torch.cuda.synchronize()
    stats('sweep_build', [(time.perf_counter() - t0) * 1e3])
    warm, ms = timed(lambda: [sweep.warm_start(i, s) for i, s in zip(draw, starts)])
    stats('warm_starts', ms, calls=len(starts))
    grid_warm = [sweep.warm_start(i, s) for s in starts for i in range(len(RATIOS))]
    sweep.close()
    states, Ps = [w[0] for w in warm], [w[1] for w in warm]
    ratios = [RATIOS[i] for i in draw]

    for n_win in args.windows:
        ends = [s + n_win for s in starts]

        def loop():
            out = []
            for w, (s, e) in enumerate(zip(starts, ends)):
                kw = dict(initial_pt=Ps[w], initial_state=states[w])
                full = ref15.run_kalman_filter_full(events, s, e, **kw)
                r = ratios[w] * min(full[1])
                ad = ref15.run_adaptive_threshold_kalman_filter(events, s, e, R_threshold=r, **kw)
                bf = ref15.run_brute_force_kalman_filter_no_sampling_min_usage(events, s, e, R_threshold=r, **kw)
                nu = ref15.run_no_update_kalman_filter(events, s, e, R_threshold=r, **kw)
                out.append((full, ad, bf, nu, r))
            return out
        want, ms = timed(loop)
        a = stats('a_four_calls_per_window', ms, window=n_win, windows=len(starts),
                  ms_per_window=round(float(np.median(ms)) / len(starts), 3))

        def batch():
            return ref15.run_window_batch(events, starts, ends, Ps, states, ratios=ratios, k_max=args.k_max)
        got, ms = timed(batch)
        b = stats('b_window_batch', ms, window=n_win, windows=len(starts), fallback_windows=len(got.fallback),
                  ms_per_window=round(float(np.median(ms)) / len(starts), 4))
        # (b)'s windows without a subset of at most k-max events: their one-window searches alone
        fb = got.fallback

        def fallbacks():
            return [ref15.run_brute_force_kalman_filter_no_sampling_min_usage(
                events, starts[w], ends[w], R_threshold=float(got.thresholds[w]), initial_pt=Ps[w],
                initial_state=states[w]) for w in fb]
        if fb:
            _, ms = timed(fallbacks)
            stats('b_part_fallback_searches', ms, window=n_win, calls=len(fb))
        equal, worst = True, 0.0
        for w, (full, ad, bf, nu, r) in enumerate(want):
            g = got[w]
            wi = tuple(ev[0] - starts[w] for ev in bf['selected_sensors']) if bf else None
            gi = tuple(ev[0] - starts[w] for ev in g['brute_force']['selected_sensors']) if g['brute_force'] else None
            equal = equal and wi == gi and g['adaptive'][4] == ad[4]
            for x, y in ((g['full'][1], full[1]), (g['adaptive'][1], ad[1]), (g['no_update'][1], nu[1])):
                worst = max(worst, float(np.max(np.abs(np.array(x) - np.array(y)) / np.maximum(np.abs(np.array(y)), 1.0))))
        print(json.dumps(dict(check='b_equals_a', window=n_win, winners_sizes_flags_equal=bool(equal),
                              logdet_max_rel=worst, sizes=sorted(set(int(k) for k in got.k_found)))), flush=True)
        assert equal

        c = None
        if n_win in args.grid_windows:
            g_starts = [s for s in starts for _ in RATIOS]
            g_ends = [s + n_win for s in g_starts]
            g_ratios = RATIOS * len(starts)
            g_states, g_Ps = [w[0] for w in grid_warm], [w[1] for w in grid_warm]
            gg, ms = timed(lambda: ref15.run_window_batch(events, g_starts, g_ends, g_Ps, g_states, ratios=g_ratios,
                                                          k_max=args.k_max))
            c = stats('c_grid_batch', ms, window=n_win, windows=len(g_starts), fallback_windows=len(gg.fallback),
                      ms_per_window=round(float(np.median(ms)) / len(g_starts), 4))

        # (d) the searches alone, on (b)'s thresholds
        setups = [ref15.brute_force_setup(events, s, e, Ps[w], states[w]) for w, (s, e) in enumerate(zip(starts, ends))]
        ev = np.stack([st[5] for st in setups])
        init = np.stack([st[6] for st in setups])
        prev = np.array([st[3] for st in setups])
        tend = np.array([st[4] for st in setups])
        kf = kfmi.BatchedKF('ref15', 1, 'f64')
        one, ms = timed(lambda: [kf.search_combos(ev[w], init[w], prev[w], tend[w], got.thresholds[w], k_max=args.k_max)[:2]
                                 for w in range(len(starts))])
        d1 = stats('d_search_combos_calls', ms, window=n_win, calls=len(starts))
        many, ms = timed(lambda: kf.search_windows(ev, init, prev, tend, got.thresholds, args.k_max))
        d2 = stats('d_search_windows', ms, window=n_win, windows=len(starts))
        kf.close()
        assert [k for k, _ in one] == many[0].tolist()
        spread = a['max_ms'] - a['min_ms']
        summary = dict(summary=True, window=n_win, a_over_b=round(a['median_ms'] / b['median_ms'], 2),
                       a_minus_b_ms=round(a['median_ms'] - b['median_ms'], 3), a_spread_ms=round(spread, 3),
                       b_beats_a_by_more_than_spread=bool(a['median_ms'] - b['median_ms'] > spread),
                       c_over_b=round(c['median_ms'] / b['median_ms'], 2) if c else None,
                       search_calls_over_search_windows=round(d1['median_ms'] / d2['median_ms'], 2))
        print(json.dumps(summary), flush=True)
        # where (b)'s time goes: the host arrays of both dt rules, the searches (d), and, outside
        # (b)'s own time, the per-window result dicts a caller builds on access
        idx, valid = ref15._window_index(starts, [n_win] * len(starts))
        h = stream.host()
        _, ms = timed(lambda: [ref15._window_rule(h['t'][idx], h['etype'][idx], h['payload'][idx], valid,
                                                  [s[0] for s in states], rule) for rule in (0, 1)])
        stats('b_part_host_window_arrays', ms, window=n_win)
        _, ms = timed(lambda: [got[w] for w in range(len(got))])
        stats('b_result_dicts_on_access', ms, window=n_win, windows=len(got))


if __name__ == '__main__':
    main()
