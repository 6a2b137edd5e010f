"""Generate tests/golden/ref15_schedules.npz: the notebook's per-window schedule search
(KF_SensorFusion.ipynb, run_brute_force_kalman_filter scored by calculate_accuracy_metrics) on
small window sets, computed with the REFERENCE's own model code.

Run where the reference is available (it never travels with the tests):

    python tests/golden/make_golden_schedules.py

The notebook's cells are not executed (its first cell installs packages).  Its class is the
kf_workers module's KF_SensorFusion plus the search loop, so the loop is restated here over the
imported class's own getters, predict_covariance and calculate_kalman_gain, in the notebook's
operation order, and scored with scipy.interpolate.interp1d as the notebook scores, against the
stream's own fixes (its get_utm_data()).

One stream, synth_events(seed=SEED, out_of_order=False), and three cases:
  f050  50 Hz, the first 4 windows (a few hundred schedules)
  f120  120 Hz, the first 6 windows (queues of 1 and 2 candidates)
  f400  400 Hz, the first 5 windows: the sampling period is shorter than the IMU's, so every
        trigger meets an empty queue and is queued alone (one schedule)
  f030  30 Hz, the first 3 windows: the third holds the stream's second fix, so the winner is
        not the all-first-candidates schedule it is in the cases above
Per case: freq, end_idx (the slice [0, end_idx) holds exactly these windows), q_len, the
candidates' positions in the stream, every metric in itertools.product order, the winner's rank,
metric, trajectory [(t, x[:6])], final state and final covariance.
"""
import os
from itertools import product

import numpy as np
from scipy.interpolate import interp1d

import make_golden

SEED = 23
CASES = (('f050', 50.0, 4), ('f120', 120.0, 6), ('f400', 400.0, 5), ('f030', 30.0, 3))


def windows(events, freq):
    """[(queue, position of the closing trigger)] over the whole list, by the notebook's rule."""
    out, queue, last = [], [], None
    for pos, ev in enumerate(events):
        if last is None and ev[1] == 'GPS':
            last = ev[2]
        if last is None:
            continue
        if ev[2] - last < 1 / freq:
            queue.append(ev)
            continue
        if len(queue) == 0:
            queue.append(ev)
        out.append((queue, pos))
        queue, last = [], ev[2]
    return out


def run_schedule(sf, combo):
    """One schedule's filter: (trajectory rows (t, x[:6]), final x, final P)."""
    x = np.zeros(15)
    P = np.diag([1000] * 3 + [100] * 3 + [100] * 3 + [100] * 3 + [1000] * 3).astype(float)
    rows, before = [], None
    for _, stype, t, sdata in combo:
        dt = t - before if before is not None else 0
        F = sf.get_state_transition_matrix(dt)
        Q = sf.get_process_noise_covariance_matrix(dt)
        x = np.dot(F, x)
        P = sf.predict_covariance(P, F, Q)
        if stype == 'GPS':
            H = sf.get_gps_observation_matrix()
            R = sf.get_gps_measurement_noise_covariance_matrix()
            Z = [sdata['easting'], sdata['northing'], sdata['altitude']]
        else:
            ax, ay, az = sdata[7], sdata[8], sdata[9]
            vx, vy, vz = x[6] + ax * dt, x[7] + ay * dt, x[8] + az * dt
            Z = [x[0] + vx * dt, x[1] + vy * dt, x[2] + vz * dt, sdata[1], sdata[2], sdata[3], vx, vy, vz,
                 sdata[4], sdata[5], sdata[6], ax, ay, az]
            H = sf.get_imu_observation_matrix()
            R = sf.get_imu_measurement_noise_covariance_matrix()
        K = sf.calculate_kalman_gain(P, H, R)
        x = x + np.dot(K, np.array(Z) - np.dot(H, x))
        P = np.dot(np.eye(15) - np.dot(K, H), P)
        rows.append((t, *x[:6]))
        before = t
    return rows, x, P


def score(rows, fix_t, fix_p):
    """The notebook's calculate_accuracy_metrics: position RMSE against the interpolated fixes."""
    t = np.array([r[0] for r in rows])
    p = np.array([r[1:4] for r in rows])
    g = np.stack([interp1d(fix_t, fix_p[:, k], kind='linear', fill_value='extrapolate')(t) for k in range(3)], axis=1)
    return np.sqrt(np.mean(np.linalg.norm(p - g, axis=1) ** 2))


def main():
    kfw, _ = make_golden.import_reference()
    events = make_golden.synth_events(seed=SEED, out_of_order=False)
    sf = kfw.KF_SensorFusion('gps.csv', 'imu.csv')
    fix_t = np.array([e[2] for e in events if e[1] == 'GPS'])
    fix_p = np.array([[e[3]['easting'], e[3]['northing'], e[3]['altitude']] for e in events if e[1] == 'GPS'])
    out = make_golden.pack_events(events)
    for name, freq, n_win in CASES:
        win = windows(events, freq)[:n_win]
        assert len(win) == n_win
        queues = [q for q, _ in win]
        best, best_rank, best_run, metrics = float('inf'), -1, None, []
        for rank, combo in enumerate(product(*queues)):
            rows, x, P = run_schedule(sf, combo)
            m = score(rows, fix_t, fix_p)
            metrics.append(m)
            if m < best:
                best, best_rank, best_run = m, rank, (rows, x, P)
        out.update({f'{name}_freq': np.array(freq), f'{name}_end_idx': np.array(win[-1][1] + 1),
                    f'{name}_q_len': np.array([len(q) for q in queues]),
                    f'{name}_cand': np.array([e[0] for q in queues for e in q]),
                    f'{name}_metrics': np.array(metrics), f'{name}_best_rank': np.array(best_rank),
                    f'{name}_best_metric': np.array(best), f'{name}_traj': np.array(best_run[0]),
                    f'{name}_x': best_run[1], f'{name}_P': best_run[2]})
        print(name, 'q_len', [len(q) for q in queues], 'schedules', len(metrics), 'best', best_rank, best)
    np.savez_compressed(os.path.join(make_golden.OUT, 'ref15_schedules.npz'), **out)


if __name__ == '__main__':
    main()
