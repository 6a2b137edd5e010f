"""kf_smooth_run_em: exported, bound with the header's arity, its row constants equal the header's, a
NULL handle is KF_EINVAL with a message that names the function, and the engine's host-side pieces
(cv_em_update on CPU tensors and arrays, the methods' signatures) work (no GPU needed)."""
import inspect
import re

import numpy as np
import pytest
import torch

from kfmi import _lib

ARITY = {'kf_smooth_run_em': 21}


def _prototypes():
    text = re.sub(r'/\*.*?\*/', '', open(_lib.HEADER).read(), flags=re.S)
    return dict(re.findall(r'\b(kf_\w+)\s*\(([^;{]*?)\)\s*;', text))


def test_symbol_exported_and_bound_with_header_arity():
    protos = _prototypes()
    L = _lib.lib()
    for name, arity in ARITY.items():
        assert name in protos, f'{name} not declared in include/kf.h'
        assert hasattr(L, name), f'{name} not exported'
        params = ' '.join(protos[name].split())
        assert len(_lib.SIGNATURES[name][1]) == params.count(',') + 1 == arity, (name, params)


def test_null_handle_is_einval_and_names_the_function():
    L = _lib.lib()
    assert L.kf_smooth_run_em(None, 4, 0.1, None, None, None, None, 1, *([None] * 13)) == _lib.KF_EINVAL
    assert 'kf_smooth_run_em' in _lib.last_error() and 'null' in _lib.last_error()


def test_constants_match_the_header():
    text = open(_lib.HEADER).read()
    names = ('KF_EM_N_TRANS', 'KF_EM_Q_POS', 'KF_EM_Q_VEL', 'KF_EM_N_FIX', 'KF_EM_R')
    for want, name in enumerate(names):
        assert int(re.search(rf'#define\s+{name}\s+(\d+)', text).group(1)) == getattr(_lib, name) == want
    assert re.search(r'#define\s+KF_EM_ROWS\(d\)\s+\(4 \+ \(d\)\)', text)
    assert _lib.KF_EM_ROWS(2) == 6 and _lib.KF_EM_ROWS(3) == 7


def test_engine_has_the_methods():
    import kfmi
    from kfmi import engine
    assert kfmi.cv_em_update is engine.cv_em_update
    assert engine.SmoothedEm._fields == ('x', 'P', 'logdet', 'status', 'init_x', 'init_P', 'em')
    assert engine.NoiseFit._fields == ('consts', 'history', 'nll', 'status')
    assert engine.EM_ROWS == {'n_trans': 0, 'q_pos': 1, 'q_vel': 2, 'n_fix': 3, 'r': 4}
    sig = inspect.signature(engine.BatchedKF.smooth_run_em).parameters
    assert list(sig)[:4] == ['self', 'filt_x', 'filt_P', 'z']
    assert [sig[k].default for k in ('init', 'consts', 'x', 'P', 'em', 'update_every', 'mask')] == \
        [None, None, False, False, True, 1, None]
    sig = inspect.signature(engine.BatchedKF.fit_noise).parameters
    assert list(sig)[:3] == ['self', 'u', 'z']
    assert [sig[k].default for k in ('x0', 'consts', 'iters', 'update_every', 'mask')] == [None, None, 10, 1, None]


@pytest.mark.parametrize('kind', ['tensor', 'array'])
def test_cv_em_update(kind):
    """q = row / (d N_TRANS), r_i = row / N_FIX; a zero count keeps the old value (column 1: no
    transition; column 2: no fix)."""
    from kfmi import KFError, cv_em_update
    em = np.array([[4.0, 0.0, 5.0], [24.0, 1.0, 30.0], [6.0, 1.0, 15.0], [2.0, 3.0, 0.0], [8.0, 9.0, 1.0],
                   [3.0, 1.5, 1.0], [1.0, 6.0, 1.0]])
    tab = np.array([[9.0, 9.25, 9.5], [7.0, 7.25, 7.5], [5.0, 5.25, 5.5], [4.0, 4.25, 4.5], [3.0, 3.25, 3.5]])
    want = np.array([[2.0, 9.25, 2.0], [0.5, 7.25, 1.0], [4.0, 3.0, 5.5], [1.5, 0.5, 4.5], [0.5, 2.0, 3.5]])
    if kind == 'tensor':
        new = cv_em_update(torch.from_numpy(em), torch.from_numpy(tab), 'cv3')
        assert torch.is_tensor(new) and new.dtype == torch.float64 and new.device.type == 'cpu'
        new = new.numpy()
    else:
        new = cv_em_update(em, tab, 'cv3')
        assert isinstance(new, np.ndarray)
    assert np.array_equal(new, want)
    assert np.array_equal(tab[0], [9.0, 9.25, 9.5])                     # a new table: the old one is not written
    new2 = cv_em_update(em[:6, :2], tab[:4, :2], 'cv2')
    assert np.array_equal(np.asarray(new2), np.array([[3.0, 9.25], [0.75, 7.25], [4.0, 3.0], [1.5, 0.5]]))
    nan = em.copy()
    nan[1, 0] = np.nan                                                   # a failed filter's NaN row passes through
    assert np.isnan(np.asarray(cv_em_update(nan, tab, 'cv3'))[0, 0])
    for bad in ((em[:6], tab, 'cv3'), (em, tab[:, :2], 'cv3'), (em, tab, 'ref15')):
        with pytest.raises(KFError) as e:
            cv_em_update(*bad)
        assert e.value.code == _lib.KF_EINVAL and 'cv_em_update' in str(e.value)
