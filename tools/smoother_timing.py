"""What a smoothed sweep costs: the forward sweep with and without the filtered record, and the
RTS backward pass (kf_smooth_sweep) out of place and in place, over the 583k-event synthetic drive
log in f64, ungated, under the reference's constants, at B = 1, 8 and 64.

Every arm is timed against the parent commit's forward sweep (no records, no checkpoints) of the
same B, alternated with it in one process on the same buffers (HBM placement differs from process
to process): build the parent's library with tools/build_rev.sh REV parent and pass
it as --parent; it is loaded side by side (tools/ab_inproc.py's way) and only its kf_run_sweep is
called.  Without --parent the yardstick is this tree's own forward sweep.

  fwd0      kf_run_sweep, no records, ckpt_every = 0
  fwd1      kf_run_sweep, no records, ckpt_every = 1: writes the filtered record (336 B per event
            and filter)
  bwd_out   kf_smooth_sweep over that record into new sm_x / sm_P
  bwd_in    kf_smooth_sweep in place (the record is rewritten by an untimed forward sweep before
            every run)

Times are device events around one launch, ``--rounds`` rounds, the two sides in alternating
order; one JSON line per arm and B with the medians, the ratio to the yardstick and every round.
Last, the plain float64 NumPy smoother of tests/smoother_oracle.py (forward and backward) on a
``--numpy-T`` slice, one filter, wall clock.

    tools/build_rev.sh HEAD~1 parent
    python tools/smoother_timing.py --parent sensorfusion-kalmanfilter_amd/kfmi/libkfmi_parent.so
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'sensorfusion-kalmanfilter_amd'), os.path.join(ROOT, 'tests')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=583000)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 8, 64])
    ap.add_argument('--parent', default=None, help='libkfmi built from the parent commit (tools/build_rev.sh)')
    ap.add_argument('--numpy-T', type=int, default=20000)
    args = ap.parse_args()
    import numpy as np
    import torch
    import kfmi
    from kfmi import _lib, ref15
    from test_gpu_sweep import _stream
    T = args.T
    et, dt, pay, x0 = _stream(T, seed=11)
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    d_et, d_dt, d_pay = (torch.as_tensor(v, device=dev) for v in (et, dt, pay))
    head = _lib.lib()
    parent = head
    if args.parent:
        parent = ctypes.CDLL(os.path.abspath(args.parent))
        for name, (res, argt) in _lib.SIGNATURES.items():
            if hasattr(parent, name):  # an older build: entry points added since are not called
                fn = getattr(parent, name)
                fn.restype, fn.argtypes = res, argt
    stream = torch.cuda.current_stream(dev)

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(stream)
        fn()
        e.record(stream)
        torch.cuda.synchronize(dev)
        return s.elapsed_time(e)

    for B in args.batches:
        thr = torch.full((B,), -float('inf'), dtype=torch.float64, device=dev)
        x = torch.as_tensor(np.repeat(x0[:, None], B, 1), device=dev)
        P = torch.as_tensor(np.repeat(ref15.to_blocks(ref15.P0)[:, None], B, 1), device=dev)
        kf = kfmi.BatchedKF('ref15', B, 'f64')
        cx, cP = kf.empty(T, 15, B), kf.empty(T, 27, B)
        sx, sP = kf.empty(T, 15, B), kf.empty(T, 27, B)
        st = torch.zeros(B, dtype=torch.int32, device=dev)
        ptr = lambda v: ctypes.c_void_p(v.data_ptr())  # noqa: E731

        def forward(lib, every):
            kf.set_state(x, P)
            rc = lib.kf_run_sweep(kf.handle, T, ptr(d_et), ptr(d_dt), ptr(d_pay), ptr(thr), None, None, None, None,
                                  every, ptr(cx) if every else None, ptr(cP) if every else None, kf._stream())
            assert rc == _lib.KF_OK, rc

        def backward(inplace):
            rc = head.kf_smooth_sweep(kf.handle, T, ptr(d_et), ptr(d_dt), None, ptr(cx), ptr(cP),
                                      ptr(cx if inplace else sx), ptr(cP if inplace else sP), None, None, ptr(st),
                                      kf._stream())
            assert rc == _lib.KF_OK, _lib.last_error()

        arms = [('fwd0', lambda: forward(head, 0), None), ('fwd1', lambda: forward(head, 1), None),
                ('bwd_out', lambda: backward(False), None), ('bwd_in', lambda: backward(True), lambda: forward(head, 1))]
        yard = lambda: forward(parent, 0)  # noqa: E731
        yard()
        forward(head, 1)
        backward(False)  # warm: module load, first-launch costs
        torch.cuda.synchronize(dev)
        for name, fn, before in arms:
            t_arm, t_yard = [], []
            for r in range(args.rounds):
                for side in ('arm', 'yard') if r % 2 == 0 else ('yard', 'arm'):
                    if side == 'yard':
                        t_yard.append(timed(yard))
                    else:
                        if before:
                            before()
                        t_arm.append(timed(fn))
            ok = int((st != 0).sum()) == 0
            m, y = statistics.median(t_arm), statistics.median(t_yard)
            print(json.dumps(dict(arm=name, B=B, T=T, median_ms=round(m, 3), yardstick_ms=round(y, 3),
                                  ratio=round(m / y, 3), us_per_event=round(m * 1e3 / T, 4),
                                  rounds_ms=[round(v, 3) for v in t_arm], yardstick_rounds_ms=[round(v, 3) for v in t_yard],
                                  yardstick='parent' if args.parent else 'head', status_ok=ok,
                                  record_GB=round(T * 42 * B * 8 / 1e9, 2))), flush=True)
        kf.close()
        del cx, cP, sx, sP
        torch.cuda.empty_cache()

    if args.numpy_T > 0:
        import smoother_oracle as so
        n = args.numpy_T
        t0 = time.perf_counter()
        so.run('ref15', x0, ref15.P0, et[:n], dt[:n], pay[:n], arith='f64')
        s = time.perf_counter() - t0
        print(json.dumps(dict(arm='numpy_f64_forward_and_backward', B=1, T=n, wall_s=round(s, 3),
                              us_per_event=round(s * 1e6 / n, 2))), flush=True)


if __name__ == '__main__':
    main()
