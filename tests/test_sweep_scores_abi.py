"""kf_run_sweep_scores (a parameter sweep scored on the device) and its KF_SCORE_* row constants
are part of the C ABI: declared in include/kf.h, exported by libkfmi.so and bound in kfmi/_lib.py
(no GPU needed)."""
import ctypes
import re

from kfmi import _lib, engine

ROWS = ('GPS_N', 'GPS_NIS', 'GPS_LOGDET_S', 'IMU_N', 'IMU_NIS', 'IMU_LOGDET_S', 'POS_N', 'POS_SSE')


def test_run_sweep_scores_is_exported_and_bound():
    assert 'kf_run_sweep_scores' in _lib.header_functions()
    assert 'kf_run_sweep_scores' in _lib.SIGNATURES
    assert hasattr(_lib.lib(), 'kf_run_sweep_scores')
    # kf_run_sweep_params' arguments plus track and scores, which follow consts
    params, scores = _lib.SIGNATURES['kf_run_sweep_params'], _lib.SIGNATURES['kf_run_sweep_scores']
    assert scores[0] is params[0] is ctypes.c_int
    assert len(scores[1]) == 17
    assert scores[1][:7] + scores[1][9:] == params[1]
    assert scores[1][7] is ctypes.c_void_p and scores[1][8] is ctypes.c_void_p


def test_score_row_constants():
    """The header's KF_SCORE_* are 0..7 in the documented order, KF_SCORE_ROWS == 8, and _lib and
    engine.SCORE_ROWS carry the same values."""
    text = open(_lib.HEADER).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define\s+KF_SCORE_(\w+)\s+(\d+)', text)}
    assert defs == {**{name: i for i, name in enumerate(ROWS)}, 'ROWS': 8}
    assert _lib.KF_SCORE_ROWS == 8
    for i, name in enumerate(ROWS):
        assert getattr(_lib, 'KF_SCORE_' + name) == i
        assert engine.SCORE_ROWS[name.lower()] == i
    assert len(engine.SCORE_ROWS) == 8


def test_run_sweep_scores_null_handle_is_einval():
    L = _lib.lib()
    table = (ctypes.c_double * 33)()
    out = (ctypes.c_double * 8)()
    rc = L.kf_run_sweep_scores(None, 4, None, None, None, None, ctypes.cast(table, ctypes.c_void_p), None,
                               ctypes.cast(out, ctypes.c_void_p), None, None, None, None, 0, None, None, None)
    assert rc == _lib.KF_EINVAL
    assert 'null' in _lib.last_error()
    assert list(out) == [0.0] * 8
