"""What the EM statistics cost on top of the constant-velocity smoother: kf_smooth_run_em at 2^20 cv3
f64 filters x 256 steps, update_every 4, against kf_smooth_run_params.

Without ``--child`` this is the driver: one child process under its own ``timeout``, its exit status
checked.  The child alternates every arm with the yardstick, kf_smooth_run_params with every output
and a table (the parent commit's build with ``--parent PATH``, tools/build_rev.sh REV parent; else
this tree's), in one process on the same buffers (HBM placement differs from process to process,
DESIGN.md §4); times are device events around the arm, ``--rounds`` rounds, the two sides in
alternating order.  One JSON line per arm: the median ms, the ratio to the yardstick in the same
rounds, the arm's algorithmic bytes per filter-step, and what the yardstick's time scaled by the byte
ratio predicts, with the yardstick's own spread (max - min over its rounds, over its median) as the
margin.

  params        this tree's kf_smooth_run_params, every output           144 B read + 120 B written
  em_full       kf_smooth_run_em, every output, initial row, em          150 B read (z: 24 B every 4th step) + 120 B
  em_only       kf_smooth_run_em, em and status only, initial row        150 B read
  fit_iter      one fit_noise iteration: kf_reset, kf_run_scores with traj and cov (reads u, z: 30 B; writes
                120 B), kf_smooth_run_em with em only (150 B), the M-step in torch
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
    cmd = ['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--child', '--B', str(args.B),
           '--T', str(args.T), '--rounds', str(args.rounds), '--update-every', str(args.update_every)]
    if args.parent:
        cmd += ['--parent', args.parent]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(json.dumps(dict(failed='child', exit_status=rc)), flush=True)
    return rc


def child(args):
    import numpy as np
    import torch
    import kfmi
    from kfmi import _lib
    B, T, k, dt = args.B, args.T, args.update_every, 0.1
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    head = _lib.lib()
    yard_lib, yard_name = head, 'head'
    if args.parent:
        yard_lib, yard_name = ctypes.CDLL(os.path.abspath(args.parent)), 'parent'
        fn = yard_lib.kf_smooth_run_params
        fn.restype, fn.argtypes = _lib.SIGNATURES['kf_smooth_run_params']
    kf = kfmi.BatchedKF('cv3', B, 'f64')
    x0, u, z = kf.synth(T=T, dt=dt, update_every=k, seed=1)
    ptr = lambda v: None if v is None else ctypes.c_void_p(v.data_ptr())  # noqa: E731
    stream = torch.cuda.current_stream(dev)
    tab = torch.from_numpy(np.ascontiguousarray(
        np.array([[s[0], s[1], *s[2]] for s in SETS]).T[:, np.arange(B) % len(SETS)])).to(dev)
    tr, cv = kf.empty(T, 6, B), kf.empty(T, 9, B)
    sx, sP, sl = kf.empty(T, 6, B), kf.empty(T, 9, B), kf.empty(T, B)
    st = torch.zeros(B, dtype=torch.int32, device=dev)
    six, siP = kf.empty(6, B), kf.empty(9, B)
    em = torch.empty(_lib.KF_EM_ROWS(3), B, dtype=torch.float64, device=dev)
    sc = torch.empty(_lib.KF_SCORE_ROWS, B, dtype=torch.float64, device=dev)
    kf.reset(x0)
    ix, iP = kf.state()
    iP = iP[kf._block_rows()].contiguous()

    def ok(rc):
        assert rc == _lib.KF_OK, (rc, _lib.last_error())

    def forward():
        ok(head.kf_reset(kf.handle, ptr(x0), kf._stream()))
        ok(head.kf_run_scores(kf.handle, T, dt, None, ptr(u), ptr(z), None, k, ptr(tab), None, ptr(sc), ptr(tr), ptr(cv),
                              None, kf._stream()))

    def params(lib):
        ok(lib.kf_smooth_run_params(kf.handle, T, dt, None, ptr(u), ptr(tr), ptr(cv), ptr(sx), ptr(sP), ptr(sl), ptr(st),
                                    ptr(tab), kf._stream()))

    def em_call(full):
        o = (sx, sP, sl, st, six, siP) if full else (None, None, None, st, None, None)
        ok(head.kf_smooth_run_em(kf.handle, T, dt, None, ptr(u), ptr(z), None, k, ptr(tr), ptr(cv), ptr(ix), ptr(iP),
                                 *[ptr(v) for v in o], ptr(tab), ptr(em), kf._stream()))

    def fit_iter():
        forward()
        em_call(False)
        kfmi.cv_em_update(em, tab, 'cv3')

    def timed(launch):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(stream)
        launch()
        e.record(stream)
        torch.cuda.synchronize(dev)
        return s.elapsed_time(e)

    zb = 24.0 / k
    yard_bytes = 144.0 + 120.0
    arms = [('params', yard_bytes, lambda: params(head)), ('em_full', 144.0 + zb + 120.0, lambda: em_call(True)),
            ('em_only', 144.0 + zb, lambda: em_call(False)), ('fit_iter', 24.0 + zb + 120.0 + 144.0 + zb, fit_iter)]
    forward()
    for _, _, launch in arms:        # warm: module load, first-launch costs, the allocator's blocks
        launch()
    params(yard_lib)
    torch.cuda.synchronize(dev)
    for name, nbytes, launch in arms:
        t_arm, t_yard = [], []
        for r in range(args.rounds):
            for side in ('arm', 'yard') if r % 2 == 0 else ('yard', 'arm'):
                (t_yard if side == 'yard' else t_arm).append(timed((lambda: params(yard_lib)) if side == 'yard' else launch))
        m, y = statistics.median(t_arm), statistics.median(t_yard)
        margin = (max(t_yard) - min(t_yard)) / y
        expected = y * nbytes / yard_bytes
        bad = int((st != 0).sum()) + int((kf.status() != 0).sum())
        print(json.dumps(dict(arm=name, yardstick=f'{yard_name} kf_smooth_run_params', update_every=k, B=B, T=T,
                              median_ms=round(m, 3), yardstick_ms=round(y, 3), ratio=round(m / y, 3),
                              bytes_per_filter_step=nbytes, TB_per_s=round(nbytes * B * T / m / 1e9, 3),
                              expected_ms=round(expected, 3), over_expected=round(m / expected - 1.0, 4),
                              yardstick_spread=round(margin, 4), within_margin=bool(m <= expected * (1.0 + margin)),
                              rounds_ms=[round(v, 3) for v in t_arm], yardstick_rounds_ms=[round(v, 3) for v in t_yard],
                              status_ok=bad == 0)), flush=True)
        assert bad == 0
    kf.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=1 << 20)
    ap.add_argument('--T', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--update-every', type=int, default=4)
    ap.add_argument('--parent', default=None)
    ap.add_argument('--limit', type=int, default=420, help="the child's time limit in seconds")
    ap.add_argument('--child', action='store_true')
    args = ap.parse_args()
    sys.exit(child(args) if args.child else driver(args))


if __name__ == '__main__':
    main()
