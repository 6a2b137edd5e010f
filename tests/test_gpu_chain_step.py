"""The 8-lanes-per-filter kernels share one event step (ChainLane::event in csrc/kf_ref_chainlane.h): on
the same short stream the chain kernel (scalar gate), the chain kernel with per-filter gates, the
sweep, a tail over the whole stream and the look-ahead kernel give the same bits — needs an
MI355X."""
import numpy as np
import pytest

import kfmi
from kfmi import ref15

pytestmark = pytest.mark.gpu
INF = float('inf')
LENGTHS = (1, 3, 19)  # 19 = 4 * 4 + 3: prologue, full rounds and remainder of ring depths 2 and 4
SCALE = np.array([20, 20, 20, 0.05, 0.05, 0.05, 0.5, 0.5, 0.5])


def _stream(T, with_none, seed):
    """GPS / IMU events (the first a GPS fix) with random dt and payloads; ``with_none``: about a
    quarter of the later events are NONE."""
    rng = np.random.default_rng(seed)
    kinds = [ref15.GPS, ref15.IMU, ref15.IMU] + ([ref15.NONE] if with_none else [])
    et = rng.choice(kinds, size=T).astype(np.uint8)
    et[0] = ref15.GPS
    if with_none and T > 1:
        et[T // 2] = ref15.NONE
    dt = rng.uniform(0.0, 0.05, T)
    pay = rng.normal(0, 1, (T, 9)) * SCALE
    return et, dt, pay


def _consts(model, seed):
    rng = np.random.default_rng(seed)
    n, g = (15, 3) if model == 'ref15' else (8, 2)
    return ref15.ModelConsts(model, q=rng.uniform(0.01, 8.0, n), r_imu=rng.uniform(0.02, 120.0, n),
                             r_gps=rng.uniform(0.5, 9.0, g), p0=rng.uniform(20.0, 2e4, n))


def _np(v):
    return None if v is None else v.cpu().numpy()


class _Runner:
    def __init__(self, model, dtype, params, et, dt, pay):
        self.model, self.dtype, self.params = model, dtype, params
        self.et, self.dt = et, dt
        self.pay = pay.astype(np.float64 if dtype == 'f64' else np.float32)

    def _run(self, B, kernel, fn):
        """fn(kf) -> records dict on a cold-started handle of B filters; adds x, P, status."""
        kf = kfmi.BatchedKF(self.model, B, self.dtype, params=self.params, options={'events_kernel': kernel})
        try:
            r = fn(kf)
            x, P = kf.state()
            r.update(x=_np(x), P=_np(P), status=_np(kf.status()))
            return r
        finally:
            kf.close()

    def _tiled(self, B):
        return (np.repeat(self.et[:, None], B, 1), np.repeat(self.dt[:, None], B, 1),
                np.repeat(self.pay[:, :, None], B, 2))

    def scalar(self, thr, kernel='chain'):
        def fn(kf):
            tr, ld, up, _ = kf.run_events(*self._tiled(1), updated=True, threshold=thr, sequential=True)
            return dict(traj=_np(tr), logdet=_np(ld), updated=_np(up))
        return self._run(1, kernel, fn)

    def gates(self, thr):
        def fn(kf):
            tr, ld, up, _ = kf.run_events_gates(*self._tiled(len(thr)), np.asarray(thr), updated=True)
            return dict(traj=_np(tr), logdet=_np(ld), updated=_np(up))
        return self._run(len(thr), 'chain', fn)

    def sweep(self, thr):
        def fn(kf):
            tr, ld, up, nu, _, _ = kf.run_sweep(self.et, self.dt, self.pay, np.asarray(thr), updated=True)
            return dict(traj=_np(tr), logdet=_np(ld), updated=_np(up), n_updated=_np(nu))
        return self._run(len(thr), 'chain', fn)

    def tails(self, thr):
        T, B = len(self.et), len(thr)
        def fn(kf):
            nu = kf.run_tails(self.et, self.dt, self.pay, [0] * B, [T] * B, np.asarray(thr), counts=True)
            return dict(n_updated=_np(nu))
        return self._run(B, 'chain', fn)


def _same(a, b, f, keys):
    """Column f of the B-filter run ``a`` equals the one-filter run ``b``, bit for bit."""
    for k in keys:
        np.testing.assert_array_equal(a[k][..., f:f + 1], b[k], err_msg=k)


@pytest.mark.parametrize('custom', [False, True])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('model', ['ref15', 'ref8'])
def test_chain_layout_kernels_share_the_event_step(model, dtype, custom):
    """Streams of 1, 3 and 19 events, GPS / IMU only and with NONE events mixed in, under an
    always-updating gate and one mid threshold (the ungated run's median log-det + 0.5): the
    chain kernel with per-filter gates, the sweep's column and the tail over [0, T) equal the
    chain kernel with the scalar gate bitwise in trajectory, log-det, flags, x, P and status (a
    tail has no records: x, P, status and its update count).  In f64 on the GPS / IMU-only stream
    the look-ahead kernel at threshold -1e9 (every gate opens, no look-ahead runs) joins,
    bitwise as well."""
    params = _consts(model, 7).params() if custom else None
    records = ('traj', 'logdet', 'updated', 'x', 'P', 'status')
    for T in LENGTHS:
        for with_none in (False, True):
            run = _Runner(model, dtype, params, *_stream(T, with_none, seed=100 + T))
            always = run.scalar(None)
            mid = float(np.median(always['logdet'])) + 0.5
            thr = [-INF, mid]
            one = [always, run.scalar(mid)]
            assert int(np.abs(always['status']).sum()) == 0
            assert always['updated'].sum() == np.sum(run.et != ref15.NONE)
            gates, sweep, tails = run.gates(thr), run.sweep(thr), run.tails(thr)
            for f in range(2):
                _same(gates, one[f], f, records)
                _same(sweep, one[f], f, records)
                _same(tails, one[f], f, ('x', 'P', 'status'))
                assert sweep['n_updated'][f] == tails['n_updated'][f] == one[f]['updated'].sum()
            if dtype == 'f64' and not with_none:
                look = run.scalar(-1e9, kernel='gated')
                _same(look, always, 0, records)
