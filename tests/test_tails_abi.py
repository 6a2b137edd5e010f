"""kf_run_tails (ragged tails of one event stream in one launch) is part of the C ABI: declared in
include/kf.h, exported by libkfmi.so and bound in kfmi/_lib.py (no GPU needed)."""
from kfmi import _lib


def test_run_tails_is_exported_and_bound():
    assert 'kf_run_tails' in _lib.header_functions()
    assert 'kf_run_tails' in _lib.SIGNATURES
    L = _lib.lib()
    assert hasattr(L, 'kf_run_tails')
    assert len(_lib.SIGNATURES['kf_run_tails'][1]) == 16


def test_run_tails_null_handle_is_einval():
    L = _lib.lib()
    rc = L.kf_run_tails(None, 4, None, None, None, None, None, None, None, None, 0, 0, None, None, None, None)
    assert rc == _lib.KF_EINVAL
    assert 'null' in _lib.last_error()
