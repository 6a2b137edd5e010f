"""kf_smooth_sweep (the RTS backward pass over a sweep's filtered record) is part of the C ABI:
declared in include/kf.h, exported by libkfmi.so and bound in kfmi/_lib.py (no GPU needed)."""
import ctypes
import re

from kfmi import _lib


def test_smooth_sweep_is_declared_exported_and_bound():
    assert 'kf_smooth_sweep' in _lib.header_functions()
    assert 'kf_smooth_sweep' in _lib.SIGNATURES
    assert hasattr(_lib.lib(), 'kf_smooth_sweep')
    res, args = _lib.SIGNATURES['kf_smooth_sweep']
    assert res is ctypes.c_int
    assert len(args) == 13
    assert args[0] is ctypes.c_void_p and args[1] is ctypes.c_int and all(a is ctypes.c_void_p for a in args[2:])
    # the header's prototype: handle, T, etype, dt, consts, the record, the five outputs, stream
    text = re.sub(r'/\*.*?\*/', '', open(_lib.HEADER).read(), flags=re.S)
    params = re.search(r'\bkf_smooth_sweep\s*\(([^;{]*?)\)\s*;', text).group(1)
    names = [p.split()[-1].lstrip('*') for p in params.split(',')]
    assert names == ['handle', 'T', 'etype', 'dt', 'consts', 'filt_x', 'filt_P', 'sm_x', 'sm_P', 'sm_traj',
                     'sm_logdet', 'sm_status', 'stream']


def test_smooth_sweep_null_handle_is_einval():
    L = _lib.lib()
    status = (ctypes.c_int32 * 1)(7)
    rc = L.kf_smooth_sweep(None, 4, None, None, None, None, None, None, None, None, None,
                           ctypes.cast(status, ctypes.c_void_p), None)
    assert rc == _lib.KF_EINVAL
    assert 'null' in _lib.last_error()
    assert status[0] == 7
