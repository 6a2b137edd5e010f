"""What a smoothed constant-velocity track costs at bench.py's config-3 shape (cv3, f64, T = 256,
update_every = 1, B = 2^20; --B 262144 where the 32 GB record plus outputs does not fit): kf_run
(the yardstick), kf_run_rec, and kf_smooth_run out of place and in place.

Every arm is alternated with the yardstick in one process on the same buffers (HBM placement
differs from process to process); times are device events around one launch,
``--rounds`` rounds, the two sides in alternating order.  One JSON line per arm: the median ms,
the ratio to kf_run in the same rounds, and the arm's algorithmic bytes over its time next to
kf_run's own bytes/s in those rounds (the pattern's live rate).

  run         kf_run: reads u, z; writes traj, logdet                      104 B per filter-step
  run_rec     kf_run_rec: the same plus cov                                176 B
  smooth_out  kf_smooth_run into new sm_x / sm_P / sm_logdet: reads filt_x, filt_P, u; 272 B
  smooth_in   kf_smooth_run in place (an untimed kf_run_rec rewrites the record before every run)

``--depth-libs 2=PATH,8=PATH`` adds a smooth_out arm per library built with another input ring
(make EXTRA=-DKF_CV_SMOOTH_DEPTH=N OUT=... BDIR=...), loaded side by side (tools/ab_inproc.py's
way; KFMI_ALLOW_FOREIGN_LIB is not needed: only its kf_smooth_run is called, on this tree's handle).
``--parent PATH``: the yardstick is that library's kf_run (tools/build_rev.sh REV parent).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'sensorfusion-kalmanfilter_amd')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=1 << 20)
    ap.add_argument('--T', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent', default=None)
    ap.add_argument('--depth-libs', default='')
    args = ap.parse_args()
    import torch
    import kfmi
    from kfmi import _lib
    B, T, dt = args.B, args.T, 0.1
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    head = _lib.lib()

    def side_lib(path):
        h = ctypes.CDLL(os.path.abspath(path))
        for name, (res, argt) in _lib.SIGNATURES.items():
            if hasattr(h, name):
                fn = getattr(h, name)
                fn.restype, fn.argtypes = res, argt
        return h

    parent = side_lib(args.parent) if args.parent else head
    depth_libs = [(kv.split('=')[0], side_lib(kv.split('=', 1)[1])) for kv in args.depth_libs.split(',') if kv]
    free, total = torch.cuda.mem_get_info(dev)
    print(json.dumps(dict(B=B, T=T, free_GB=round(free / 1e9, 1), total_GB=round(total / 1e9, 1),
                          buffers_GB=round(B * T * 8 * (3 + 3 + 6 + 9 + 1 + 6 + 9 + 1) / 1e9, 1))), flush=True)
    kf = kfmi.BatchedKF('cv3', B, 'f64')
    x0, u, z = kf.synth(T=T, dt=dt, update_every=1, seed=1)
    tr, cv, ld = kf.empty(T, 6, B), kf.empty(T, 9, B), kf.empty(T, B)
    sx, sP, sl = kf.empty(T, 6, B), kf.empty(T, 9, B), kf.empty(T, B)
    st = torch.zeros(B, dtype=torch.int32, device=dev)
    ptr = lambda v: ctypes.c_void_p(v.data_ptr())  # noqa: E731
    stream = torch.cuda.current_stream(dev)

    def run(lib):
        kf.reset(x0)
        rc = lib.kf_run(kf.handle, T, dt, None, ptr(u), ptr(z), None, 1, ptr(tr), ptr(ld), kf._stream())
        assert rc == _lib.KF_OK, rc

    def run_rec():
        kf.reset(x0)
        rc = head.kf_run_rec(kf.handle, T, dt, None, ptr(u), ptr(z), None, 1, ptr(tr), ptr(cv), ptr(ld), kf._stream())
        assert rc == _lib.KF_OK, _lib.last_error()

    def smooth(lib, inplace):
        rc = lib.kf_smooth_run(kf.handle, T, dt, None, ptr(u), ptr(tr), ptr(cv), ptr(tr if inplace else sx),
                               ptr(cv if inplace else sP), ptr(sl), ptr(st), kf._stream())
        assert rc == _lib.KF_OK, rc

    def timed(fn, launch):
        fn()  # the untimed part (reset / rewriting the record), then the launch alone
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(stream)
        launch()
        e.record(stream)
        torch.cuda.synchronize(dev)
        return s.elapsed_time(e)

    def launch_run(lib):
        return lambda: lib.kf_run(kf.handle, T, dt, None, ptr(u), ptr(z), None, 1, ptr(tr), ptr(ld), kf._stream())

    reset = lambda: kf.reset(x0)  # noqa: E731
    arms = [('run', 104, reset, launch_run(head)),
            ('run_rec', 176, reset, lambda: head.kf_run_rec(kf.handle, T, dt, None, ptr(u), ptr(z), None, 1, ptr(tr),
                                                            ptr(cv), ptr(ld), kf._stream())),
            ('smooth_out', 272, lambda: None, lambda: smooth(head, False)),
            ('smooth_in', 272, run_rec, lambda: smooth(head, True))]
    arms += [(f'smooth_out_depth{d}', 272, lambda: None, (lambda lib: lambda: smooth(lib, False))(lib))
             for d, lib in depth_libs]
    run(parent)
    run_rec()
    smooth(head, False)
    for _, lib in depth_libs:
        smooth(lib, False)  # warm: module load, first-launch costs
    torch.cuda.synchronize(dev)
    run_rec()               # the record the out-of-place arms read
    for name, nbytes, before, launch in arms:
        t_arm, t_yard = [], []
        for r in range(args.rounds):
            for side in ('arm', 'yard') if r % 2 == 0 else ('yard', 'arm'):
                if side == 'yard':
                    t_yard.append(timed(reset, launch_run(parent)))
                else:
                    t_arm.append(timed(before, launch))
        if name in ('run', 'run_rec', 'smooth_in'):
            run_rec()       # the yardstick and these arms overwrite the record
        m, y = statistics.median(t_arm), statistics.median(t_yard)
        print(json.dumps(dict(arm=name, B=B, T=T, median_ms=round(m, 3), yardstick_ms=round(y, 3), ratio=round(m / y, 3),
                              bytes_per_filter_step=nbytes, TB_per_s=round(nbytes * B * T / m / 1e9, 3),
                              yardstick_TB_per_s=round(104 * B * T / y / 1e9, 3),
                              rounds_ms=[round(v, 3) for v in t_arm], yardstick_rounds_ms=[round(v, 3) for v in t_yard],
                              yardstick='parent' if args.parent else 'head',
                              status_ok=int((st != 0).sum()) == 0 and int((kf.status() != 0).sum()) == 0)), flush=True)
    kf.close()


if __name__ == '__main__':
    main()
