"""kf_run_sweep (one event stream under B adaptive thresholds) is part of the C ABI: declared in
include/kf.h, exported by libkfmi.so and bound in kfmi/_lib.py (no GPU needed)."""
from kfmi import _lib


def test_run_sweep_is_exported_and_bound():
    assert 'kf_run_sweep' in _lib.header_functions()
    assert 'kf_run_sweep' in _lib.SIGNATURES
    L = _lib.lib()
    assert hasattr(L, 'kf_run_sweep')
    assert len(_lib.SIGNATURES['kf_run_sweep'][1]) == 14


def test_run_sweep_null_handle_is_einval():
    L = _lib.lib()
    rc = L.kf_run_sweep(None, 4, None, None, None, None, None, None, None, None, 0, None, None, None)
    assert rc == _lib.KF_EINVAL
    assert 'null' in _lib.last_error()
