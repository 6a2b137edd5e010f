"""kf_run_events_gates (a gate per filter on per-filter streams) and kf_search_windows (many
windows in one search) are part of the C ABI, and kfmi.ref15.window_arrays builds the windows'
[L][B] event arrays as the per-window drivers build them (no GPU needed)."""
import numpy as np
import pytest

from kfmi import _lib, ref15
from test_gpu_sweep import _stream

NAMES = {'kf_run_events_gates': 11, 'kf_search_windows': 14}


@pytest.mark.parametrize('name', sorted(NAMES))
def test_entry_point_is_declared_exported_and_bound(name):
    assert name in _lib.header_functions()
    assert name in _lib.SIGNATURES
    assert hasattr(_lib.lib(), name)
    assert len(_lib.SIGNATURES[name][1]) == NAMES[name]


def test_null_handles_are_einval():
    L = _lib.lib()
    assert L.kf_run_events_gates(None, 4, None, None, None, None, None, None, None, None, None) == _lib.KF_EINVAL
    assert 'null' in _lib.last_error()
    rc = L.kf_search_windows(None, 1, 4, None, None, None, None, None, None, 2, None, None, None, None)
    assert rc == _lib.KF_EINVAL
    assert 'null' in _lib.last_error()


# ---------------------------------------------------------------------------------------------
# the window-array helper against the list drivers' own stream builder
# ---------------------------------------------------------------------------------------------
T = 240


def _merged():
    """_stream's log as a merged stream with times, its one NONE event made what the drivers'
    dt < 0 rule is for: an event stamped before its predecessor.  Returns (t, etype, payload,
    the reference-layout event list, the out-of-order position)."""
    et, _, pay, _ = _stream(T, seed=3, skips=1)
    j = int(np.nonzero(et == ref15.NONE)[0][0])
    assert 30 < j < T - 30, j   # room for windows before, across and after it (a condition on the seed)
    et = et.copy()
    et[j] = ref15.IMU
    t = 100.0 + np.arange(T) * 0.005
    t[j] = t[j - 1] - 0.002
    events = []
    for i in range(T):
        if et[i] == ref15.GPS:
            sd = {'easting': pay[i, 0], 'northing': pay[i, 1], 'altitude': pay[i, 2]}
            events.append((i, 'GPS', float(t[i]), sd))
        else:
            events.append((i, 'IMU', float(t[i]), [repr(t[i]), *pay[i]]))
    return t, et, pay, events, j


def _windows(j):
    """(start, length) pairs: before the out-of-order event, across it (in the middle, as the
    first entry, as the last), ending at the stream's end; unequal lengths."""
    return [(5, 25), (j - 12, 25), (j, 7), (j - 9, 10), (j + 1, 3), (T - 40, 40), (T - 1, 1), (j - 1, 2)]


@pytest.mark.parametrize('rule', [_lib.KF_DT_FULL, _lib.KF_DT_MONOTONE])
def test_window_arrays_equal_the_drivers_streams(rule):
    t, et, pay, events, j = _merged()
    wins = _windows(j)
    starts = [s for s, _ in wins]
    lens = [n for _, n in wins]
    # each window's state time: just before its first event, or (window 3) after it, so that the
    # first entry itself is skipped
    prev = [float(t[s]) - 0.001 for s in starts]
    prev[3] = float(t[starts[3]]) + 0.0005
    e, d, p = ref15.window_arrays(t, et, pay, starts, lens, prev, rule)
    L = max(lens)
    assert e.shape == (L, len(wins)) and e.dtype == np.uint8
    assert d.shape == (L, len(wins)) and d.dtype == np.float64
    assert p.shape == (L, 9, len(wins)) and p.dtype == np.float64
    skipped_somewhere = False
    for w, (s, n) in enumerate(wins):
        stream, times, kept, _ = ref15._driver_stream(events[s:s + n], prev[w], rule)
        col = np.full(L, ref15.NONE, np.uint8)
        col[kept] = [ty for ty, _, _ in stream]
        assert np.array_equal(e[:, w], col), (w, e[:, w], col)
        assert np.array_equal(d[kept, w], np.array([dd for _, dd, _ in stream])), w   # bit for bit: t - prev
        assert np.array_equal(p[kept, :, w], np.array([pp for _, _, pp in stream]).reshape(len(kept), 9)), w
        assert np.array_equal(times, t[s:s + n][kept])
        skipped_somewhere |= len(kept) < n
        # the padding: KF_EVENT_NONE, zero dt and payload
        assert np.all(e[n:, w] == ref15.NONE) and np.all(d[n:, w] == 0) and np.all(p[n:, :, w] == 0)
    assert skipped_somewhere


def test_the_rules_differ_after_a_skipped_event():
    """The entry after the out-of-order one: KF_DT_FULL measures from the skipped event's time,
    KF_DT_MONOTONE from the latest time so far."""
    t, et, pay, _, j = _merged()
    args = (t, et, pay, [j - 2], [5], [float(t[j - 2]) - 0.001])
    ef, df, _ = ref15.window_arrays(*args, _lib.KF_DT_FULL)
    em, dm, _ = ref15.window_arrays(*args, _lib.KF_DT_MONOTONE)
    assert ef[2, 0] == em[2, 0] == ref15.NONE and ef[3, 0] != ref15.NONE
    assert df[3, 0] == t[j + 1] - t[j] and dm[3, 0] == t[j + 1] - t[j - 1]


def test_no_update_streams_are_predicts():
    _, _, _, events, j = _merged()
    stream, _, kept, _ = ref15._driver_stream(events[j - 3:j + 3], events[j - 3][2], _lib.KF_DT_MONOTONE,
                                              predict_only=True)
    assert len(kept) == 5 and all(ty == ref15.PREDICT and not any(pp) for ty, _, pp in stream)


def test_window_outside_the_stream_is_refused():
    t, et, pay, _, _ = _merged()
    with pytest.raises(ValueError):
        ref15.window_arrays(t, et, pay, [T - 3], [5], [0.0], _lib.KF_DT_FULL)
