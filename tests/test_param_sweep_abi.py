"""kf_run_sweep_params (one event stream under B constant sets and gates) and kf_consts_rows are
part of the C ABI: declared in include/kf.h, exported by libkfmi.so and bound in kfmi/_lib.py (no
GPU needed)."""
import ctypes

from kfmi import _lib, engine


def test_run_sweep_params_is_exported_and_bound():
    for name in ('kf_run_sweep_params', 'kf_consts_rows'):
        assert name in _lib.header_functions()
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)
    # kf_run_sweep's arguments plus consts, which follows thresholds
    sweep, params = _lib.SIGNATURES['kf_run_sweep'], _lib.SIGNATURES['kf_run_sweep_params']
    assert params[0] is sweep[0] is ctypes.c_int
    assert len(params[1]) == 15
    assert params[1][:6] + params[1][7:] == sweep[1] and params[1][6] is ctypes.c_void_p
    assert _lib.SIGNATURES['kf_consts_rows'][1] == [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]


def test_consts_rows_for_both_models():
    """q and r_imu per state, r_gps per axis, in kf_params order with the model's lengths."""
    L = _lib.lib()
    rows = ctypes.c_int(-1)
    assert L.kf_consts_rows(_lib.KF_MODEL_REF15, ctypes.byref(rows)) == _lib.KF_OK and rows.value == 15 + 15 + 3
    assert L.kf_consts_rows(_lib.KF_MODEL_REF8, ctypes.byref(rows)) == _lib.KF_OK and rows.value == 8 + 8 + 2
    assert engine.consts_rows('ref15') == 33 and engine.consts_rows('ref8') == 18
    p = _lib.kf_params()
    assert rows.value <= len(p.ref_q) + len(p.ref_r_imu) + len(p.ref_r_gps) == 33


def test_consts_rows_errors():
    L = _lib.lib()
    rows = ctypes.c_int(-1)
    for model in (_lib.KF_MODEL_CV3, _lib.KF_MODEL_CV2, 99):
        assert L.kf_consts_rows(model, ctypes.byref(rows)) == _lib.KF_EINVAL
        assert f'kf_consts_rows: model {model} has no per-filter constants' in _lib.last_error()
    assert rows.value == -1
    assert L.kf_consts_rows(_lib.KF_MODEL_REF15, None) == _lib.KF_EINVAL
    assert 'kf_consts_rows: null rows' in _lib.last_error()


def test_run_sweep_params_null_handle_is_einval():
    """With and without a table (consts = NULL is kf_run_sweep itself)."""
    L = _lib.lib()
    table = (ctypes.c_double * 33)()
    for consts in (None, ctypes.cast(table, ctypes.c_void_p)):
        rc = L.kf_run_sweep_params(None, 4, None, None, None, None, consts, None, None, None, None, 0, None, None,
                                   None)
        assert rc == _lib.KF_EINVAL
        assert 'null' in _lib.last_error()


def test_consts_table_layout():
    """engine.consts_table: column f is set f's q, r_imu, r_gps; a set of the other model is
    KF_EINVAL."""
    import numpy as np
    import pytest
    from kfmi import ref15
    a = ref15.ModelConsts('ref8', q=np.arange(1.0, 9.0), r_imu=np.arange(11.0, 19.0), r_gps=[21.0, 22.0])
    b = ref15.ModelConsts('ref8')
    tab = engine.consts_table('ref8', [a, b])
    assert tab.shape == (18, 2) and tab.dtype == np.float64
    np.testing.assert_array_equal(tab[:, 0], list(range(1, 9)) + list(range(11, 19)) + [21, 22])
    d = engine.default_params('ref8')
    np.testing.assert_array_equal(tab[:, 1], list(d.ref_q)[:8] + list(d.ref_r_imu)[:8] + list(d.ref_r_gps)[:2])
    with pytest.raises(_lib.KFError) as e:
        engine.consts_table('ref15', [a])
    assert e.value.code == _lib.KF_EINVAL and 'ref8' in str(e.value)
