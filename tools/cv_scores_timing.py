"""What scoring a constant-velocity run in its launch costs, and what it saves, at bench.py's
config-3 shape (cv3, f64, T = 256, B = 2^20), update_every 1 and 5.

Without arguments this is the driver: one child process per (update_every, group), each under its
own ``timeout``, every exit status checked, nothing more started after the first failure.  A child
(``--group forward|smooth --update-every K``) alternates every arm with the yardstick, kf_run with
both records, in one process on the same buffers (HBM placement differs from process to process,
DESIGN.md §4); times are device events around the arm, ``--rounds`` rounds, the two sides in
alternating order.  One JSON line per arm: the median ms, the ratio to kf_run in the same rounds
and the arm's algorithmic bytes per filter-step.

group forward
  scores            kf_run_scores, no record, no track, no table: reads u, z          48 B (k = 1)
  scores_track      ... with a track                                                  72 B
  scores_consts     ... with a table (5 doubles per filter, once)                     48 B
  scores_track_consts                                                                 72 B
  run_rec           kf_run_rec with traj, cov, logdet                                176 B
  run_traj_rmse     kf_run with traj only, then the torch reduction of
                    sum (traj[:, :3] - track)^2 over steps and axes (timed together)
  parent_run / parent_run_rec   with --parent PATH (tools/build_rev.sh REV parent): that
                    library's kf_run / kf_run_rec, in the same process
group smooth
  smooth            kf_smooth_run out of place over a kf_run_rec record              272 B
  smooth_params     kf_smooth_run_params with a table, same record                   272 B
With update_every = k the fixes are read on every k-th step only: 24 (1 + 1 / k) B of u and z.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'sensorfusion-kalmanfilter_amd')]
SETS = [(0.0625, 0.5, (2.0, 3.0, 4.0)), (0.5, 0.125, (1.0, 1.0, 1.0)), (0.015625, 2.0, (9.0, 0.5, 3.0)),
        (1.0, 1.0, (4.0, 4.0, 0.25)), (0.25, 0.03125, (0.75, 6.0, 2.5))]


def driver(args):
    for k in (1, 5):
        for group, limit in (('forward', 240), ('smooth', 240)):
            cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--group', group,
                   '--update-every', str(k), '--B', str(args.B), '--T', str(args.T), '--rounds', str(args.rounds)]
            if args.parent:
                cmd += ['--parent', args.parent]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print(json.dumps(dict(failed=group, update_every=k, exit_status=rc)), flush=True)
                return rc
    return 0


def child(args):
    import numpy as np
    import torch
    import kfmi
    from kfmi import _lib
    B, T, k, dt = args.B, args.T, args.update_every, 0.1
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    head = _lib.lib()
    parent = None
    if args.parent:
        parent = ctypes.CDLL(os.path.abspath(args.parent))
        for name, (res, argt) in _lib.SIGNATURES.items():
            if hasattr(parent, name):
                fn = getattr(parent, name)
                fn.restype, fn.argtypes = res, argt
    kf = kfmi.BatchedKF('cv3', B, 'f64')
    x0, u, z = kf.synth(T=T, dt=dt, update_every=k, seed=1)
    U = T // k
    ptr = lambda v: None if v is None else ctypes.c_void_p(v.data_ptr())  # noqa: E731
    stream = torch.cuda.current_stream(dev)
    tab = torch.from_numpy(np.ascontiguousarray(
        np.array([[s[0], s[1], *s[2]] for s in SETS]).T[:, np.arange(B) % len(SETS)])).to(dev)
    sc = torch.empty(_lib.KF_SCORE_ROWS, B, dtype=torch.float64, device=dev)
    fwd = args.group == 'forward'
    tr, ld = kf.empty(T, 6, B), kf.empty(T, B)
    cv = kf.empty(T, 9, B)
    track = sse = sx = sP = sl = st = None
    if fwd:
        # a track a few metres from the fixes: each step against the fix its update interval ends with
        idx = torch.clamp(torch.arange(T, device=dev) // k, max=U - 1)
        track = (z[idx] + 2.0 * torch.randn(T, 3, B, dtype=torch.float64, device=dev)).contiguous()
        sse = torch.empty(B, dtype=torch.float64, device=dev)
    else:
        sx, sP, sl = kf.empty(T, 6, B), kf.empty(T, 9, B), kf.empty(T, B)
        st = torch.zeros(B, dtype=torch.int32, device=dev)

    def ok(rc):
        assert rc == _lib.KF_OK, (rc, _lib.last_error())

    def run(lib, traj=True, logdet=True):
        ok(lib.kf_run(kf.handle, T, dt, None, ptr(u), ptr(z), None, k, ptr(tr) if traj else None,
                      ptr(ld) if logdet else None, kf._stream()))

    def run_rec(lib):
        ok(lib.kf_run_rec(kf.handle, T, dt, None, ptr(u), ptr(z), None, k, ptr(tr), ptr(cv), ptr(ld), kf._stream()))

    def scores(consts, tk):
        ok(head.kf_run_scores(kf.handle, T, dt, None, ptr(u), ptr(z), None, k, ptr(consts), ptr(tk), ptr(sc), None,
                              None, None, kf._stream()))

    def run_rmse():
        run(head, logdet=False)
        e = tr[:, :3] - track
        torch.sum(e * e, dim=(0, 1), out=sse)

    def smooth(consts):
        if consts is None:
            ok(head.kf_smooth_run(kf.handle, T, dt, None, ptr(u), ptr(tr), ptr(cv), ptr(sx), ptr(sP), ptr(sl), ptr(st),
                                  kf._stream()))
        else:
            ok(head.kf_smooth_run_params(kf.handle, T, dt, None, ptr(u), ptr(tr), ptr(cv), ptr(sx), ptr(sP), ptr(sl),
                                         ptr(st), ptr(consts), kf._stream()))

    def timed(launch):
        kf.reset(x0)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(stream)
        launch()
        e.record(stream)
        torch.cuda.synchronize(dev)
        return s.elapsed_time(e)

    zb = 24.0 * (1.0 + 1.0 / k)
    if fwd:
        arms = [('scores', zb, lambda: scores(None, None)), ('scores_track', zb + 24, lambda: scores(None, track)),
                ('scores_consts', zb, lambda: scores(tab, None)),
                ('scores_track_consts', zb + 24, lambda: scores(tab, track)),
                ('run_rec', zb + 128, lambda: run_rec(head)), ('run_traj_rmse', None, run_rmse)]
        if parent is not None:
            arms += [('parent_run', zb + 56, lambda: run(parent)), ('parent_run_rec', zb + 128, lambda: run_rec(parent))]
    else:
        arms = [('smooth', 272.0, lambda: smooth(None)), ('smooth_params', 272.0, lambda: smooth(tab))]
    for _, _, launch in arms:        # warm: module load, first-launch costs, the allocator's blocks
        kf.reset(x0)
        launch()
    kf.reset(x0)
    run(head)
    torch.cuda.synchronize(dev)
    for name, nbytes, launch in arms:
        if not fwd:
            kf.reset(x0)
            run_rec(head)            # the record the smoother reads (the yardstick overwrites traj)
        t_arm, t_yard = [], []
        for r in range(args.rounds):
            for side in ('arm', 'yard') if r % 2 == 0 else ('yard', 'arm'):
                if side == 'yard':
                    t_yard.append(timed(lambda: run(head)))
                    if not fwd:
                        kf.reset(x0)
                        run_rec(head)
                else:
                    t_arm.append(timed(launch))
        m, y = statistics.median(t_arm), statistics.median(t_yard)
        bad = int((kf.status() != 0).sum()) + (int((st != 0).sum()) if st is not None else 0)
        print(json.dumps(dict(arm=name, update_every=k, B=B, T=T, median_ms=round(m, 3), yardstick_ms=round(y, 3),
                              ratio=round(m / y, 3), bytes_per_filter_step=nbytes,
                              TB_per_s=round(nbytes * B * T / m / 1e9, 3) if nbytes else None,
                              yardstick_TB_per_s=round((zb + 56) * B * T / y / 1e9, 3),
                              rounds_ms=[round(v, 3) for v in t_arm], yardstick_rounds_ms=[round(v, 3) for v in t_yard],
                              status_ok=bad == 0)), flush=True)
        assert bad == 0
    kf.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=1 << 20)
    ap.add_argument('--T', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent', default=None)
    ap.add_argument('--group', choices=('forward', 'smooth'), default=None)
    ap.add_argument('--update-every', type=int, default=1)
    args = ap.parse_args()
    sys.exit(child(args) if args.group else driver(args))


if __name__ == '__main__':
    main()
