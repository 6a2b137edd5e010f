"""The notebook's per-window schedule search (KF_SensorFusion.ipynb, run_brute_force_kalman_filter)
as the shared-prefix search against one filter per schedule, over a 200 Hz IMU / 10 Hz GPS stream
cut at f = 20 Hz (queues of about 10 candidates):

  (a) W = 6 (~10^6 schedules): every schedule as its own filter through kf_run_events on
      materialised [W][9][N] streams, then the RMSE and the argmin in torch — the only route
      before kf_search_schedules.  The streams are built once, outside the timed call (their
      host build is reported on its own).
  (b) W = 6: kf_search_schedules with every metric written (metrics=True).
  (c) W = 7 and 8 (~10^7, 10^8): (b) alone, with the plan's node and byte counts.

Wall clock around a synchronised call: one warm call, then ``--runs`` runs; median (min - max),
one JSON line per arm.  At W = 6 both arms must give the same winner and their metrics agree to
1e-9 relative.  The acceptance rule: (a)'s minimum minus (b)'s median must exceed
the spread (max - min) of both arms.  As context, not a claim about like hardware: schedules/s
against the NumPy oracle helper on this host and the notebook's recorded 12.9-13.9 schedules/s
(SURVEY.md §6).

    python tools/schedule_search_timing.py [--runs 5] [--windows 6 7 8] [--freq 20]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'sensorfusion-kalmanfilter_amd'), os.path.join(ROOT, 'tests')]
KERNELS = 1e-9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--windows', type=int, nargs='+', default=[6, 7, 8])
    ap.add_argument('--each', type=int, default=6, help='the W at which arm (a) runs too')
    ap.add_argument('--freq', type=float, default=20.0)
    ap.add_argument('--seed', type=int, default=11)
    args = ap.parse_args()
    import numpy as np
    import torch
    import kfmi
    import schedule_oracle as so
    from kfmi import ref15
    from test_gpu_timeparallel import _stream
    T = 40 + int(max(args.windows) * 1.2 * 200 / args.freq)
    et, _, pay, _ = _stream(T, seed=args.seed)
    t_abs = 1.7e9 + np.arange(T) * 0.005
    events = []
    for i in range(T):
        if et[i] == ref15.GPS:
            events.append((i, 'GPS', float(t_abs[i]), {'time': float(t_abs[i]), 'easting': pay[i, 0],
                                                       'northing': pay[i, 1], 'altitude': pay[i, 2]}))
        else:
            events.append((i, 'IMU', float(t_abs[i]), [repr(t_abs[i]), *pay[i]]))
    all_queues = ref15.schedule_queues(events, 0, None, args.freq)
    track = ref15._track_of(events, None)
    init = np.concatenate([np.zeros(15), ref15.to_blocks(ref15.SCHEDULE_P0)])
    dev = torch.device('cuda', 0)

    def timed(fn):
        fn()  # warm
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.runs):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t) * 1e3)
        return out, ms

    def stats(name, ms, **kw):
        row = dict(arm=name, median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3),
                   max_ms=round(max(ms), 3), runs=len(ms), runs_ms=[round(m, 2) for m in ms], **kw)
        print(json.dumps(row), flush=True)
        return row

    # context: the NumPy oracle helper on this host (shared prefixes, three windows)
    t = time.perf_counter()
    m3 = so.metrics(all_queues[:3], *track)
    oracle_rate = len(m3) / (time.perf_counter() - t)
    print(json.dumps(dict(context='numpy_oracle_host', schedules=len(m3), schedules_per_s=round(oracle_rate, 1),
                          notebook_recorded_schedules_per_s=[12.9, 13.9])), flush=True)

    kf1 = kfmi.BatchedKF('ref15', 1, 'f64')
    for W in args.windows:
        queues = all_queues[:W]
        assert len(queues) == W, 'the stream is too short for this many windows'
        q_len, ev, ref = ref15.schedule_arrays(queues, *track)
        N = int(np.prod(q_len.astype(np.int64)))
        plan = kf1.schedule_plan(q_len)
        shape = dict(W=W, q_len=[int(q) for q in q_len], schedules=N, widest_nodes=plan['widest'],
                     workspace_bytes=plan['workspace_bytes'],
                     event_steps_search=int(sum(np.cumprod(q_len.astype(np.int64)))), event_steps_each=N * W)
        res, ms = timed(lambda: kf1.search_schedules(ev, q_len, ref, init, metrics=True))
        b = stats('b_search_schedules' if W == args.each else 'c_search_schedules', ms,
                  schedules_per_s=round(N / (float(np.median(ms)) * 1e-3)), **shape)
        rank_b, digits_b, metric_b, n_valid, mt_b = res
        assert n_valid == N
        if W != args.each:
            continue
        # (a) one filter per schedule: the streams, schedule-major columns in product order
        t = time.perf_counter()
        off = np.concatenate([[0], np.cumsum(q_len)])
        digits = np.stack(np.unravel_index(np.arange(N), q_len))          # [W, N]
        pick = digits + off[:W, None]                                      # candidate rows
        tt = ev[pick, 0]                                                   # [W, N]
        dts = np.concatenate([np.zeros((1, N)), np.diff(tt, axis=0)])
        h_et = ev[pick, 1].astype(np.uint8)
        h_pay = np.ascontiguousarray(ev[pick, 2:].transpose(0, 2, 1))      # [W, 9, N]
        h_ref = np.ascontiguousarray(ref[pick].transpose(0, 2, 1))         # [W, 3, N]
        build_ms = (time.perf_counter() - t) * 1e3
        d_et, d_dt, d_pay, d_ref = (torch.as_tensor(v, device=dev) for v in (h_et, dts, h_pay, h_ref))
        kfN = kfmi.BatchedKF('ref15', N, 'f64')
        x0 = torch.zeros(15, N, dtype=torch.float64, device=dev)
        P0 = torch.as_tensor(init[15:], device=dev)[:, None].repeat(1, N).contiguous()

        def each():
            kfN.set_state(x0, P0)
            tr, _, _, _ = kfN.run_events(d_et, d_dt, d_pay, logdet=False)
            mt = torch.sqrt(((tr[:, :3] - d_ref) ** 2).sum(dim=(0, 1)) / W)
            return mt, int(torch.argmin(mt))
        (mt_a, rank_a), ms = timed(each)
        a = stats('a_one_filter_per_schedule', ms, schedules_per_s=round(N / (float(np.median(ms)) * 1e-3)),
                  stream_bytes=int(h_pay.nbytes + dts.nbytes + h_et.nbytes), host_stream_build_ms=round(build_ms, 1),
                  **shape)
        kfN.close()
        rel = float(torch.max(torch.abs(mt_a - mt_b) / torch.clamp(torch.abs(mt_b), min=1.0)))
        print(json.dumps(dict(check='a_equals_b', same_winner=bool(rank_a == rank_b), rank=rank_b, digits=digits_b,
                              metric=metric_b, metrics_max_rel=rel)), flush=True)
        assert rank_a == rank_b and rel <= KERNELS
        spread = (a['max_ms'] - a['min_ms']) + (b['max_ms'] - b['min_ms'])
        gain = a['min_ms'] - b['median_ms']
        print(json.dumps(dict(summary=True, W=W, a_over_b=round(a['median_ms'] / b['median_ms'], 2),
                              a_min_minus_b_median_ms=round(gain, 3), spread_of_both_ms=round(spread, 3),
                              accepted=bool(gain > spread),
                              expected_ratio_from_event_steps=round(shape['event_steps_each'] /
                                                                    shape['event_steps_search'], 2),
                              b_over_numpy_oracle_host=round(b['schedules_per_s'] / oracle_rate),
                              b_over_notebook_recorded=round(b['schedules_per_s'] / 13.0))), flush=True)
    kf1.close()


if __name__ == '__main__':
    main()
