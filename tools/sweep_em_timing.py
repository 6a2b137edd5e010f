"""What the EM statistics cost on top of the reference models' smoother: kf_smooth_sweep_em over the
583k-event synthetic drive log, ref15 f64, ungated, under the reference's constants, at B = 64 (the
log and the batch README quotes for kf_smooth_sweep), against kf_smooth_sweep.

Without ``--child`` this is the driver: one child process under its own ``timeout``, its exit status
checked.  The child alternates every arm with the yardstick, kf_smooth_sweep into new sm_x / sm_P (the
parent commit's build with ``--parent PATH``, tools/build_rev.sh REV parent; else this tree's), in one
process on the same buffers (HBM placement differs from process to process); times are
device events around the arm, ``--rounds`` rounds, the two sides in alternating order.  One JSON line
per arm: the median ms, the ratio to the yardstick in the same rounds, every round, and the
yardstick's own spread (max - min over its rounds, over its median).

  smooth      this tree's kf_smooth_sweep into new sm_x / sm_P (the kernel is the parent's: the two
              must agree within the spread)
  em_full     kf_smooth_sweep_em, sm_x and sm_P out of place, status, em
  em_only     kf_smooth_sweep_em, em and status only
  em_iter     one whole EM iteration as ref15.fit_noise runs it: kf_set_state, kf_run_sweep_scores with
              ckpt_every = 1 and ``updated``, kf_smooth_sweep_em in place with em, the M-step in torch
  fwd_scores  that iteration's forward half alone

``--alt PATH`` (a build of this tree with another -DKF_REF_EM_DEPTH, e.g. make EXTRA=-DKF_REF_EM_DEPTH=2
BDIR=build_d2 OUT=kfmi/libkfmi_emd2.so) adds em_full and em_only of that build as arms of their own,
in the same process, so the two ring depths are compared on the same buffers.

    tools/build_rev.sh HEAD~1 parent
    python tools/sweep_em_timing.py --parent sensorfusion-kalmanfilter_amd/kfmi/libkfmi_parent.so
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'sensorfusion-kalmanfilter_amd'), os.path.join(ROOT, 'tests')]


def driver(args):
    cmd = ['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--child', '--B', str(args.B),
           '--T', str(args.T), '--rounds', str(args.rounds)]
    for k in ('parent', 'alt'):
        if getattr(args, k):
            cmd += [f'--{k}', getattr(args, k)]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(json.dumps(dict(failed='child', exit_status=rc)), flush=True)
    return rc


def child(args):
    import numpy as np
    import torch
    import kfmi
    from kfmi import _lib, engine, ref15
    from test_gpu_sweep import _stream
    B, T = args.B, args.T
    et, dt, pay, x0 = _stream(T, seed=11)
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    d_et, d_dt, d_pay = (torch.as_tensor(v, device=dev) for v in (et, dt, pay))
    head = _lib.lib()

    def load(path):
        lib = ctypes.CDLL(os.path.abspath(path))
        for name, (res, argt) in _lib.SIGNATURES.items():
            if hasattr(lib, name):  # an older build: entry points added since are not called
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, argt
        return lib
    yard_lib, yard_name = (load(args.parent), 'parent') if args.parent else (head, 'head')
    alt = load(args.alt) if args.alt else None
    stream = torch.cuda.current_stream(dev)
    ptr = lambda v: None if v is None else ctypes.c_void_p(v.data_ptr())  # noqa: E731
    x = torch.as_tensor(np.repeat(x0[:, None], B, 1), device=dev)
    P = torch.as_tensor(np.repeat(ref15.to_blocks(ref15.P0)[:, None], B, 1), device=dev)
    tab = torch.from_numpy(engine.consts_table('ref15', [ref15.ModelConsts('ref15')] * B)).to(dev)
    kf = kfmi.BatchedKF('ref15', B, 'f64')
    cx, cP = kf.empty(T, 15, B), kf.empty(T, 27, B)
    sx, sP = kf.empty(T, 15, B), kf.empty(T, 27, B)
    up = torch.empty(T, B, dtype=torch.uint8, device=dev)
    st = torch.zeros(B, dtype=torch.int32, device=dev)
    em = torch.empty(engine.em_rows('ref15'), B, dtype=torch.float64, device=dev)
    sc = torch.empty(_lib.KF_SCORE_ROWS, B, dtype=torch.float64, device=dev)

    def ok(rc):
        assert rc == _lib.KF_OK, (rc, _lib.last_error())

    def forward():
        kf.set_state(x, P)
        ok(head.kf_run_sweep_scores(kf.handle, T, ptr(d_et), ptr(d_dt), ptr(d_pay), None, ptr(tab), None, ptr(sc), None,
                                    None, ptr(up), None, 1, ptr(cx), ptr(cP), kf._stream()))

    def smooth(lib):
        ok(lib.kf_smooth_sweep(kf.handle, T, ptr(d_et), ptr(d_dt), None, ptr(cx), ptr(cP), ptr(sx), ptr(sP), None, None,
                               ptr(st), kf._stream()))

    def em_call(lib, ox, oP):
        ok(lib.kf_smooth_sweep_em(kf.handle, T, ptr(d_et), ptr(d_dt), ptr(d_pay), ptr(up), None, ptr(cx), ptr(cP), ptr(ox),
                                  ptr(oP), None, None, ptr(st), ptr(em), kf._stream()))

    def em_iter():
        forward()
        em_call(head, cx, cP)
        kfmi.ref_em_update(em, tab, 'ref15')

    def timed(launch):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(stream)
        launch()
        e.record(stream)
        torch.cuda.synchronize(dev)
        return s.elapsed_time(e)

    # (name, launch, untimed step before every timed run: em_iter rewrites the record itself)
    arms = [('smooth', lambda: smooth(head), None), ('em_full', lambda: em_call(head, sx, sP), None),
            ('em_only', lambda: em_call(head, None, None), None)]
    if alt is not None:
        arms += [('em_full_alt', lambda: em_call(alt, sx, sP), None), ('em_only_alt', lambda: em_call(alt, None, None), None)]
    arms += [('em_iter', em_iter, None), ('fwd_scores', forward, None)]
    forward()
    torch.cuda.synchronize(dev)
    first = None
    for name, launch, _ in arms[:-2]:   # warm: module load, first-launch costs; and the tables must agree
        launch()
        torch.cuda.synchronize(dev)
        if name.startswith('em_'):
            first = em.clone() if first is None else first
            assert torch.equal(em, first), f'{name}: another table'
    smooth(yard_lib)
    em_iter()
    forward()
    torch.cuda.synchronize(dev)
    for name, launch, before in arms:
        t_arm, t_yard = [], []
        for r in range(args.rounds):
            for side in ('arm', 'yard') if r % 2 == 0 else ('yard', 'arm'):
                if side == 'yard':
                    t_yard.append(timed(lambda: smooth(yard_lib)))
                else:
                    t_arm.append(timed(launch))
            if name == 'em_iter':
                forward()   # the yardstick and the later arms read a filtered record, not a smoothed one
        m, y = statistics.median(t_arm), statistics.median(t_yard)
        bad = int((st != 0).sum()) + int((kf.status() != 0).sum())
        print(json.dumps(dict(arm=name, yardstick=f'{yard_name} kf_smooth_sweep', B=B, T=T, median_ms=round(m, 3),
                              yardstick_ms=round(y, 3), ratio=round(m / y, 4), us_per_event=round(m * 1e3 / T, 4),
                              yardstick_spread=round((max(t_yard) - min(t_yard)) / y, 4),
                              rounds_ms=[round(v, 3) for v in t_arm], yardstick_rounds_ms=[round(v, 3) for v in t_yard],
                              alt=os.path.basename(args.alt) if args.alt and name.endswith('_alt') else None,
                              status_ok=bad == 0)), flush=True)
        assert bad == 0
    kf.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=64)
    ap.add_argument('--T', type=int, default=583000)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--parent', default=None, help='libkfmi built from the parent commit (tools/build_rev.sh)')
    ap.add_argument('--alt', default=None, help='a build of this tree with another KF_REF_EM_DEPTH')
    ap.add_argument('--limit', type=int, default=540, help="the child's time limit in seconds")
    ap.add_argument('--child', action='store_true')
    args = ap.parse_args()
    sys.exit(child(args) if args.child else driver(args))


if __name__ == '__main__':
    main()
