"""The threshold sweep (kf_run_sweep: one event stream under B adaptive gates in one launch)
against what it replaces, over the 583k-event synthetic drive log with the experiment loop's seven
thresholds lb x {0.2 .. 0.8} (kf_workers.py:2298-2317; lb = the minimum log-det of an ungated run
over the first 100k events):

  (a) seven run_events(..., threshold=r) calls, default route, summed (the baseline)
  (b) one sweep with records (trajectory, log-det, update flags, counts)
  (c) one sweep with checkpoints only
  (d) 40 warm_start calls at spread end_idx against the same 40 through
      run_adaptive_threshold_kalman_filter
  (e) the chain kernel alone (one filter, sequential) at the sweep's lowest threshold, the one
      that updates most: the divergence model says a sweep costs about this

Each arm is warmed once, then timed ``--runs`` times (wall clock around a synchronised call, the
inputs already on the device): median, min and max per arm, one JSON line each, then the ratios.

    python tools/threshold_sweep_timing.py [--T 583000] [--runs 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'sensorfusion-kalmanfilter_amd'), os.path.join(ROOT, 'tests')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=583000)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--warm-starts', type=int, default=40)
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
    P0 = ref15.to_blocks(ref15.P0)
    d_et, d_dt, d_pay = (torch.as_tensor(v, device=dev) for v in (et, dt, pay))

    def timed(fn, runs=args.runs):
        fn()  # warm
        ms = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t) * 1e3)
        return out, ms

    def stats(name, ms, **kw):
        row = dict(arm=name, T=T, median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3),
                   max_ms=round(max(ms), 3), runs=len(ms), **kw)
        print(json.dumps(row), flush=True)
        return row

    one = kfmi.BatchedKF('ref15', 1, 'f64')

    def reset(kf, B=1):
        kf.set_state(np.repeat(x0[:, None], B, 1), np.repeat(P0[:, None], B, 1))

    n_lb = min(100000, T)
    reset(one)
    _, ld, _, _ = one.run_events(d_et[:n_lb, None], d_dt[:n_lb, None], d_pay[:n_lb, :, None], traj=False)
    lb = float(ld.min())
    thr = [lb * k / 10 for k in range(2, 9)]
    print(json.dumps(dict(lb=lb, thresholds=thr)), flush=True)

    # (a) the parent's offer: one gated run per threshold, default route
    per, shares = [], []
    for r in thr:
        def run_one(r=r):
            reset(one)
            return one.run_events(d_et[:, None], d_dt[:, None], d_pay[:, :, None], updated=True, threshold=r)
        out, ms = timed(run_one)
        per.append(ms)
        shares.append(float(out[2].float().mean()))
        stats('a_one_threshold', ms, threshold=r, updated_share=round(shares[-1], 4),
              fallback=one.stream_check()['fallback'])
    a = stats('a_seven_run_events', [sum(m[i] for m in per) for i in range(args.runs)])

    # (e) the chain kernel alone at the most-updating threshold
    chain = kfmi.BatchedKF('ref15', 1, 'f64', options={'events_kernel': 'chain'})

    def run_chain():
        reset(chain)
        return chain.run_events(d_et[:, None], d_dt[:, None], d_pay[:, :, None], updated=True, threshold=min(thr),
                                sequential=True)
    _, ms = timed(run_chain)
    e = stats('e_chain_kernel_lowest_threshold', ms, threshold=min(thr), us_per_event=round(np.median(ms) * 1e3 / T, 4))
    chain.close()

    # (b), (c) the sweep
    sw = kfmi.BatchedKF('ref15', len(thr), 'f64')
    d_thr = torch.as_tensor(np.array(thr), device=dev)

    def run_sweep(**kw):
        reset(sw, len(thr))
        return sw.run_sweep(d_et, d_dt, d_pay, d_thr, **kw)
    out, ms = timed(lambda: run_sweep(updated=True))
    n_up = out[3].cpu().numpy()
    b = stats('b_sweep_records', ms, us_per_event=round(np.median(ms) * 1e3 / T, 4), n_updated=n_up.tolist())
    _, ms = timed(lambda: run_sweep(traj=False, logdet=False, checkpoint_every=args.checkpoint_every))
    c = stats('c_sweep_checkpoints_only', ms, us_per_event=round(np.median(ms) * 1e3 / T, 4))
    sw.close()
    one.close()

    # (d) warm starts: the checkpoint + tail against the driver's whole prefix
    t_abs = 1.7e9 + np.cumsum(dt)
    stream = ingest.EventStream(etype=d_et, t=torch.as_tensor(t_abs, device=dev), payload=d_pay,
                                src=torch.zeros(T, dtype=torch.int32, device=dev),
                                zone_number=torch.zeros(T, dtype=torch.int8, device=dev),
                                zone_letter=torch.zeros(T, dtype=torch.uint8, device=dev),
                                first_valid_index=0, gyro_bias=np.zeros(3), accel_bias=np.zeros(3),
                                utm_origin=np.zeros(2), n_fixes=int((et == 0).sum()), n_imu=int((et == 1).sum()))
    t0 = time.perf_counter()
    sweep = ref15.AdaptiveSweep(stream, thr, records=False, checkpoint_every=args.checkpoint_every)
    torch.cuda.synchronize()
    stats('d_sweep_object_build', [(time.perf_counter() - t0) * 1e3])
    n = args.warm_starts
    ends = [int(v) for v in np.linspace(T // n, T, n)]

    def warm_all():
        return [sweep.warm_start(i % len(thr), end) for i, end in enumerate(ends)]
    got, ms = timed(warm_all)
    dw = stats('d_warm_starts', ms, calls=n)

    def driver_all():
        return [ref15.run_adaptive_threshold_kalman_filter(stream, 0, end, R_threshold=thr[i % len(thr)])
                for i, end in enumerate(ends)]
    want, ms = timed(driver_all, runs=1)
    dd = stats('d_driver_calls', ms, calls=n)
    worst = 0.0
    for (state, P, prev), w in zip(got, want):
        ws = np.array(w[0][-1])
        worst = max(worst, float(np.max(np.abs(np.array(state) - ws) / np.maximum(np.abs(ws), 1.0))),
                    float(np.max(np.abs(P - w[2]) / np.maximum(np.abs(w[2]), 1.0))))
        assert prev == w[3]
    sweep.close()
    spread_a = a['max_ms'] - a['min_ms']
    print(json.dumps(dict(summary=True, a_over_b=round(a['median_ms'] / b['median_ms'], 3),
                          a_over_c=round(a['median_ms'] / c['median_ms'], 3),
                          a_minus_b_ms=round(a['median_ms'] - b['median_ms'], 3), a_spread_ms=round(spread_a, 3),
                          b_beats_a_by_more_than_spread=bool(a['median_ms'] - b['median_ms'] > spread_a),
                          b_over_e=round(b['median_ms'] / e['median_ms'], 3),
                          driver_over_warm_start=round(dd['median_ms'] / dw['median_ms'], 2),
                          warm_start_max_rel=worst)), flush=True)


if __name__ == '__main__':
    main()
