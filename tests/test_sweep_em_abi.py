"""kf_smooth_sweep_em / kf_em_rows: exported, bound with the header's arity and argument names, the
row macros equal the header's, a NULL handle is KF_EINVAL with a message that names the function,
and the engine's host-side pieces (ref_em_update on CPU tensors and arrays, the methods'
signatures) work (no GPU needed)."""
import ctypes
import inspect
import re

import numpy as np
import pytest
import torch

from kfmi import _lib

ARITY = {'kf_smooth_sweep_em': 16, 'kf_em_rows': 2}


def _prototypes():
    text = re.sub(r'/\*.*?\*/', '', open(_lib.HEADER).read(), flags=re.S)
    return dict(re.findall(r'\b(kf_\w+)\s*\(([^;{]*?)\)\s*;', text))


def test_symbols_exported_and_bound_with_header_arity():
    protos = _prototypes()
    L = _lib.lib()
    for name, arity in ARITY.items():
        assert name in protos, f'{name} not declared in include/kf.h'
        assert name in _lib.header_functions()
        assert hasattr(L, name), f'{name} not exported'
        params = ' '.join(protos[name].split())
        assert len(_lib.SIGNATURES[name][1]) == params.count(',') + 1 == arity, (name, params)
    names = [p.split()[-1].lstrip('*') for p in protos['kf_smooth_sweep_em'].split(',')]
    assert names == ['handle', 'T', 'etype', 'dt', 'payload', 'updated', 'consts', 'filt_x', 'filt_P', 'sm_x', 'sm_P',
                     'sm_traj', 'sm_logdet', 'sm_status', 'em', 'stream']
    res, args = _lib.SIGNATURES['kf_smooth_sweep_em']
    assert res is ctypes.c_int and args[0] is ctypes.c_void_p and args[1] is ctypes.c_int
    assert all(a is ctypes.c_void_p for a in args[2:])
    assert _lib.SIGNATURES['kf_em_rows'][1] == [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]


def test_null_handle_is_einval_and_names_the_function():
    L = _lib.lib()
    status = (ctypes.c_int32 * 1)(7)
    args = [None] * 14
    args[11] = ctypes.cast(status, ctypes.c_void_p)
    assert L.kf_smooth_sweep_em(None, 4, *args) == _lib.KF_EINVAL
    assert 'kf_smooth_sweep_em' in _lib.last_error() and 'null' in _lib.last_error()
    assert status[0] == 7


def test_row_macros_match_the_header():
    text = open(_lib.HEADER).read()

    def macro(name, args):
        m = re.search(rf'^#define\s+{name}{re.escape(args)}\s+(.*?)\s*(?:/\*.*)?$', text, flags=re.M)
        assert m, name
        return m.group(1)
    assert macro('KF_REF_EM_N_TRANS', '') == '0' and _lib.KF_REF_EM_N_TRANS == 0
    assert macro('KF_REF_EM_Q', '') == '1' and _lib.KF_REF_EM_Q == 1
    for name in ('KF_REF_EM_N_IMU', 'KF_REF_EM_R_IMU', 'KF_REF_EM_N_GPS', 'KF_REF_EM_R_GPS'):
        body = macro(name, '(n)')
        for n in (15, 8):
            assert eval(body, {'n': n}) == getattr(_lib, name)(n), name
    body = macro('KF_REF_EM_ROWS', '(n, m)')
    for n, m, want in ((15, 3, 36), (8, 2, 21)):
        assert eval(body, {'n': n, 'm': m}) == _lib.KF_REF_EM_ROWS(n, m) == want
    # a count before each block, the blocks in the constants table's order
    for n, m in ((15, 3), (8, 2)):
        assert _lib.KF_REF_EM_N_IMU(n) == _lib.KF_REF_EM_Q + n
        assert _lib.KF_REF_EM_R_IMU(n) == _lib.KF_REF_EM_N_IMU(n) + 1
        assert _lib.KF_REF_EM_N_GPS(n) == _lib.KF_REF_EM_R_IMU(n) + n
        assert _lib.KF_REF_EM_R_GPS(n) == _lib.KF_REF_EM_N_GPS(n) + 1
        assert _lib.KF_REF_EM_ROWS(n, m) == _lib.KF_REF_EM_R_GPS(n) + m


def test_em_rows():
    L = _lib.lib()
    rows = ctypes.c_int(0)
    assert L.kf_em_rows(_lib.KF_MODEL_REF15, ctypes.byref(rows)) == _lib.KF_OK and rows.value == 36
    assert L.kf_em_rows(_lib.KF_MODEL_REF8, ctypes.byref(rows)) == _lib.KF_OK and rows.value == 21
    rows = ctypes.c_int(-1)
    for model in (_lib.KF_MODEL_CV2, _lib.KF_MODEL_CV3, 99):
        assert L.kf_em_rows(model, ctypes.byref(rows)) == _lib.KF_EINVAL
        assert 'kf_em_rows' in _lib.last_error()
    assert rows.value == -1
    assert L.kf_em_rows(_lib.KF_MODEL_REF15, None) == _lib.KF_EINVAL
    assert 'kf_em_rows: null rows' in _lib.last_error()


def test_engine_has_the_methods():
    import kfmi
    from kfmi import engine, ref15
    assert kfmi.ref_em_update is engine.ref_em_update and kfmi.ref_em_rows is engine.ref_em_rows
    assert engine.SmoothedSweepEm._fields == ('x', 'P', 'traj', 'logdet', 'status', 'em')
    assert engine.ref_em_rows('ref15') == {'n_trans': 0, 'q': 1, 'n_imu': 16, 'r_imu': 17, 'n_gps': 32, 'r_gps': 33,
                                           'rows': 36}
    assert engine.ref_em_rows('ref8') == {'n_trans': 0, 'q': 1, 'n_imu': 9, 'r_imu': 10, 'n_gps': 18, 'r_gps': 19,
                                          'rows': 21}
    assert engine.em_rows('ref15') == 36 and engine.em_rows('ref8') == 21
    sig = inspect.signature(engine.BatchedKF.smooth_sweep_em).parameters
    assert list(sig)[:7] == ['self', 'etype', 'dt', 'payload', 'updated', 'filt_x', 'filt_P']
    assert [sig[k].default for k in ('consts', 'status', 'em', 'inplace')] == [None, True, True, False]
    sig = inspect.signature(ref15.fit_noise).parameters
    assert list(sig)[:5] == ['events', 'consts_list', 'thresholds', 'iters', 'imu_rows']
    assert [sig[k].default for k in ('consts_list', 'thresholds', 'iters', 'imu_rows')] == [None, None, 10, 'measured']
    assert 'em' in inspect.signature(ref15.AdaptiveSweep.__init__).parameters
    assert 'em' in inspect.signature(ref15.ParameterSweep.__init__).parameters
    assert 'monotonic' in ref15.fit_noise.__doc__


@pytest.mark.parametrize('kind', ['tensor', 'array'])
def test_ref_em_update(kind):
    """q_i = Q_i / N_TRANS, r = R / N; a zero count keeps the old block (column 1: no transition;
    column 2: no IMU update and no fix); a q whose old value is 0 stays 0; imu_rows picks the R_imu
    rows; NaN rows pass through."""
    from kfmi import KFError, engine, ref_em_update
    n, m = 8, 2
    r = engine.ref_em_rows('ref8')
    B = 3
    em = np.zeros((r['rows'], B))
    em[r['n_trans']] = [4.0, 0.0, 5.0]
    em[r['n_imu']] = [2.0, 3.0, 0.0]
    em[r['n_gps']] = [8.0, 1.0, 0.0]
    em[r['q']:r['q'] + n] = np.arange(1, n + 1)[:, None] * np.array([4.0, 7.0, 10.0])
    em[r['r_imu']:r['r_imu'] + n] = np.arange(1, n + 1)[:, None] * np.array([2.0, 6.0, 9.0])
    em[r['r_gps']:r['r_gps'] + m] = np.array([[16.0, 3.0, 5.0], [4.0, 0.5, 5.0]])
    tab = 100.0 + np.arange((2 * n + m) * B, dtype=np.float64).reshape(2 * n + m, B)
    tab[3, 0] = 0.0                                        # a state without process noise
    old = tab.copy()
    arg = (torch.from_numpy(em), torch.from_numpy(tab)) if kind == 'tensor' else (em, tab)
    new = ref_em_update(*arg, 'ref8')
    if kind == 'tensor':
        assert torch.is_tensor(new) and new.dtype == torch.float64 and new.device.type == 'cpu'
        new = new.numpy()
    else:
        assert isinstance(new, np.ndarray)
    assert np.array_equal(tab, old)                        # a new table: the old one is not written
    want = old.copy()
    want[:n, 0] = np.arange(1, n + 1) * 4.0 / 4.0
    want[3, 0] = 0.0
    want[:n, 2] = np.arange(1, n + 1) * 10.0 / 5.0
    meas = list(engine.IMU_MEASURED['ref8'])
    assert meas == [2, 5, 6, 7]
    for f, cnt, scale in ((0, 2.0, 2.0), (1, 3.0, 6.0)):
        want[[n + i for i in meas], f] = np.array([i + 1 for i in meas]) * scale / cnt
    want[2 * n:, 0] = [2.0, 0.5]
    want[2 * n:, 1] = [3.0, 0.5]
    assert np.array_equal(new, want)
    every = np.asarray(ref_em_update(em, tab, 'ref8', imu_rows='all'))
    assert np.array_equal(every[n:2 * n, 0], np.arange(1, n + 1) * 2.0 / 2.0)
    assert np.array_equal(every[n:2 * n, 2], old[n:2 * n, 2])
    none = np.asarray(ref_em_update(em, tab, 'ref8', imu_rows='none'))
    assert np.array_equal(none[n:2 * n], old[n:2 * n]) and np.array_equal(none[:n], want[:n])
    nan = em.copy()
    nan[r['q'] + 1, 0] = np.nan
    assert np.isnan(np.asarray(ref_em_update(nan, tab, 'ref8'))[1, 0])
    for bad in ((em[:-1], tab, 'ref8'), (em, tab[:, :2], 'ref8'), (em, tab, 'cv3'), (em, tab, 'ref15')):
        with pytest.raises(KFError) as e:
            ref_em_update(*bad)
        assert e.value.code == _lib.KF_EINVAL and 'ref_em_update' in str(e.value)
    with pytest.raises(KFError):
        ref_em_update(em, tab, 'ref8', imu_rows='some')
