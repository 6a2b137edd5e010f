"""NumPy restatement of the notebook's per-window schedule search (KF_SensorFusion.ipynb,
run_brute_force_kalman_filter with calculate_accuracy_metrics) over oracle.ref_kf.step15: the
checker of kf_search_schedules and kfmi.ref15.search_schedules.  Shared by test_schedules_abi.py
and test_gpu_schedules.py; no GPU, no library.

Every schedule's filter is the reference's dense 15-state step, one pick per window; schedules
that share a prefix share its steps (the same numbers: a step depends on the prefix alone), which
keeps a few thousand schedules under a second.
"""
import numpy as np

from oracle import ref_kf

# the notebook's cold-start covariance
P0 = np.diag([1000.0] * 3 + [100.0] * 9 + [1000.0] * 3)


def queues(events, start_idx=0, end_idx=None, frequency=50.0):
    """The sampling windows of events[start_idx:end_idx]: nothing before the first fix; an event
    less than 1/frequency after the last trigger joins the open queue; any other event is a
    trigger, which closes the queue (joining it only if it is empty) and restarts the clock.
    The open queue at the end is dropped."""
    if end_idx is None:
        end_idx = len(events)
    out, cur, clock = [], [], None
    for ev in events[start_idx:end_idx]:
        stype, t = ev[1], ev[2]
        if clock is None:
            if stype != 'GPS':
                continue
            clock = t
        if t - clock < 1 / frequency:
            cur.append(ev)
        else:
            out.append(cur if cur else [ev])
            cur, clock = [], t
    return out


def track_positions(track_t, track_p, tq):
    """Piecewise-linear track through (track_t, track_p [G, 3]) at tq; outside the track the
    nearest end segment's line continues."""
    track_t = np.asarray(track_t, np.float64)
    track_p = np.asarray(track_p, np.float64)
    out = np.empty((len(tq), 3))
    for k, t in enumerate(np.asarray(tq, np.float64)):
        j = int(np.searchsorted(track_t, t, side='left'))
        j = min(max(j, 1), len(track_t) - 1)
        t0, t1 = track_t[j - 1], track_t[j]
        out[k] = (track_p[j] - track_p[j - 1]) / (t1 - t0) * (t - t0) + track_p[j - 1]
    return out


def fixes(events):
    """(times, positions [G, 3]) of an event list's fixes."""
    g = [(t, sd) for _, stype, t, sd in events if stype == 'GPS']
    return (np.array([t for t, _ in g]),
            np.array([[sd['easting'], sd['northing'], sd['altitude']] for _, sd in g]))


def metrics(qs, track_t, track_p, x0=None, P=None, prev_time=None, K=None, with_states=False):
    """Every schedule's position RMSE in itertools.product order (the last window fastest):
    metric = sqrt(sum over the picks of |x[:3] - track(t_pick)|^2 / W).  x0 / P / prev_time: the
    start (zeros, the notebook's P0, None = the first pick's dt is 0).  K: custom diagonal
    constants (ModelConsts.oracle()).  with_states: also the leaves' (trajectory [W, 7] rows
    (t, x[:6]), x, P) lists."""
    W = len(qs)
    x0 = np.zeros(15) if x0 is None else np.asarray(x0, np.float64)
    P = P0 if P is None else np.asarray(P, np.float64)
    refs = [track_positions(track_t, track_p, [ev[2] for ev in q]) for q in qs]
    out, states = [], []

    def walk(w, x, Pw, prev, sse, traj):
        if w == W:
            out.append(np.sqrt(sse / W))
            if with_states:
                states.append((np.array(traj), x, Pw))
            return
        for c, (_, stype, t, sdata) in enumerate(qs[w]):
            dt = t - prev if prev is not None else 0.0
            xn, Pn = ref_kf.step15(x, Pw, stype, sdata, dt, K)
            e = xn[:3] - refs[w][c]
            walk(w + 1, xn, Pn, t, sse + (e[0] * e[0] + e[1] * e[1] + e[2] * e[2]),
                 traj + [(t, *xn[:6])] if with_states else traj)

    with np.errstate(invalid='ignore'):
        walk(0, x0, P, prev_time, 0.0, [])
    m = np.array(out)
    return (m, states) if with_states else m


def winner(m):
    """(rank, metric) of the first strictly smallest finite metric, or (None, inf)."""
    best, rank = np.inf, None
    for r, v in enumerate(m):
        if v < best:
            best, rank = v, r
    return rank, best


def digits_of(rank, q_len):
    d = []
    for q in reversed(q_len):
        d.append(rank % q)
        rank //= q
    return tuple(reversed(d))
