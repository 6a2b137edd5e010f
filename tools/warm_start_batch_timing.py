"""The experiment loop's warm starts (kf_workers.py:2306-2317: the adaptive filter from event 0 to
each start point) from one AdaptiveSweep, one call per start point against all of them as one
batch of ragged tails (kf_run_tails), over the 583k-event synthetic drive log with the loop's 284
start points, its seven thresholds lb x {0.2 .. 0.8} and checkpoint_every = 4096:

  (a) 284 AdaptiveSweep.warm_start calls (set_state, a one-filter sweep, a state read-back each)
  (b) one AdaptiveSweep.warm_starts call over the same 284 (threshold, start point) pairs
  (c) the 284 x 7 grid, every start point under every threshold: one warm_starts call of 1,988 tails
  (d) (b) split: its run_tails launch, synchronised (the device part), and everything else (host)

Each arm is warmed once, then timed ``--runs`` times (wall clock around a synchronised call):
every run, median, min and max per arm, one JSON line each, then the summary.  (b)'s results must
equal (a)'s, tuple by tuple and covariance by covariance, and (c)'s entries those of (a) where
they share a pair.  Acceptance: (b)'s median lies below (a)'s minimum by more than (a)'s own
max - min spread.

    python tools/warm_start_batch_timing.py [--T 583000] [--runs 5] [--checkpoint-every 4096]
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
    ap.add_argument('--checkpoint-every', type=int, default=4096)
    args = ap.parse_args()
    import numpy as np
    import torch
    import kfmi
    from kfmi import ingest, ref15
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

    def timed(fn, runs=args.runs):
        fn()  # warm
        torch.cuda.synchronize()
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
                   max_ms=round(max(ms), 3), runs=len(ms), runs_ms=[round(m, 3) for m in ms], **kw)
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
    every = args.checkpoint_every
    tails = [(1 + s) % every for s in starts]  # array entries past each start point's checkpoint
    print(json.dumps(dict(lb=lb, thresholds=thr, start_points=len(starts), first_start=starts[0],
                          last_start=starts[-1], checkpoint_every=every, longest_tail=max(tails),
                          tail_events=sum(tails))), flush=True)
    t0 = time.perf_counter()
    sweep = ref15.AdaptiveSweep(stream, thr, records=False, checkpoint_every=every)
    torch.cuda.synchronize()
    stats('sweep_build', [(time.perf_counter() - t0) * 1e3])

    one, ms = timed(lambda: [sweep.warm_start(i, s) for i, s in zip(draw, starts)])
    a = stats('a_warm_start_calls', ms, calls=len(starts), ms_per_call=round(float(np.median(ms)) / len(starts), 4))
    many, ms = timed(lambda: sweep.warm_starts(draw, starts))
    b = stats('b_warm_starts_batch', ms, tails=len(starts))

    def equal(x, y):
        return (x is None and y is None) or (x is not None and y is not None and x[0] == y[0] and x[2] == y[2]
                                             and np.array_equal(x[1], y[1]))
    b_equals_a = len(one) == len(many) and all(equal(x, y) for x, y in zip(one, many))
    print(json.dumps(dict(check='b_equals_a', entries=len(many), equal=bool(b_equals_a))), flush=True)
    assert b_equals_a

    g_index = [i for _ in starts for i in range(len(RATIOS))]
    g_starts = [s for s in starts for _ in RATIOS]
    grid, ms = timed(lambda: sweep.warm_starts(g_index, g_starts))
    c = stats('c_grid_batch', ms, tails=len(g_starts), ms_per_tail=round(float(np.median(ms)) / len(g_starts), 5))
    c_equals_a = all(equal(grid[w * len(RATIOS) + i], one[w]) for w, i in enumerate(draw))
    print(json.dumps(dict(check='c_equals_a_on_shared_pairs', entries=len(draw), equal=bool(c_equals_a))), flush=True)
    assert c_equals_a

    # (d): (b) again with its launch timed on its own (synchronised before and after)
    run_tails = kfmi.BatchedKF.run_tails
    dev_ms = []

    def timed_run_tails(self, *a_, **kw):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = run_tails(self, *a_, **kw)
        torch.cuda.synchronize()
        dev_ms.append((time.perf_counter() - t) * 1e3)
        return out
    kfmi.BatchedKF.run_tails = timed_run_tails
    try:
        _, ms = timed(lambda: sweep.warm_starts(draw, starts))
    finally:
        kfmi.BatchedKF.run_tails = run_tails
    dev_ms = dev_ms[1:]  # without the warm call's
    d = stats('d_batch_with_split', ms, tails=len(starts))
    d_dev = stats('d_part_run_tails_synchronised', dev_ms, tails=len(starts))
    d_host = stats('d_part_host_and_copies', [t - k for t, k in zip(ms, dev_ms)], tails=len(starts))
    sweep.close()

    spread_a = a['max_ms'] - a['min_ms']
    spread_b = b['max_ms'] - b['min_ms']
    ok = bool(a['min_ms'] - b['median_ms'] > spread_a)
    print(json.dumps(dict(summary=True, a_over_b_medians=round(a['median_ms'] / b['median_ms'], 2),
                          a_spread_ms=round(spread_a, 3), b_spread_ms=round(spread_b, 3),
                          a_min_minus_b_median_ms=round(a['min_ms'] - b['median_ms'], 3),
                          b_median_below_a_min_by_more_than_a_spread=ok,
                          c_over_b_medians=round(c['median_ms'] / b['median_ms'], 2),
                          c_tails_over_b_tails=round(len(g_starts) / len(starts), 2),
                          d_device_share=round(d_dev['median_ms'] / d['median_ms'], 3),
                          d_host_ms=d_host['median_ms'])), flush=True)
    assert ok


if __name__ == '__main__':
    main()
