"""kf_run_scores / kf_smooth_run_params: exported, bound with the header's arity, a NULL handle is
KF_EINVAL with a message that names the function, and the engine's host-side pieces
(cv_consts_table, innovation_nll for the CV models) work (no GPU needed)."""
import math
import re

import numpy as np
import pytest

from kfmi import _lib

ARITY = {'kf_run_scores': 15, 'kf_smooth_run_params': 13}


def _prototypes():
    text = re.sub(r'/\*.*?\*/', '', open(_lib.HEADER).read(), flags=re.S)
    return dict(re.findall(r'\b(kf_\w+)\s*\(([^;{]*?)\)\s*;', text))


def test_symbols_exported_and_bound_with_header_arity():
    protos = _prototypes()
    L = _lib.lib()
    for name, arity in ARITY.items():
        assert name in protos, f'{name} not declared in include/kf.h'
        assert hasattr(L, name), f'{name} not exported'
        params = ' '.join(protos[name].split())
        assert len(_lib.SIGNATURES[name][1]) == params.count(',') + 1 == arity, (name, params)


def test_null_handle_is_einval_and_names_the_function():
    L = _lib.lib()
    assert L.kf_run_scores(None, 4, 0.1, None, None, None, None, 1, None, None, None, None, None, None,
                           None) == _lib.KF_EINVAL
    assert 'kf_run_scores' in _lib.last_error() and 'null' in _lib.last_error()
    assert L.kf_smooth_run_params(None, 4, 0.1, None, None, None, None, None, None, None, None, None,
                                  None) == _lib.KF_EINVAL
    assert 'kf_smooth_run_params' in _lib.last_error() and 'null' in _lib.last_error()


def test_constants_match_the_header():
    text = open(_lib.HEADER).read()
    for name in ('KF_CV_CONST_Q_POS', 'KF_CV_CONST_Q_VEL', 'KF_CV_CONST_R'):
        assert int(re.search(rf'#define\s+{name}\s+(\d+)', text).group(1)) == getattr(_lib, name)
    assert re.search(r'#define\s+KF_CV_CONST_ROWS\(d\)\s+\(2 \+ \(d\)\)', text)
    assert _lib.KF_CV_CONST_ROWS(2) == 4 and _lib.KF_CV_CONST_ROWS(3) == 5


def test_engine_has_the_methods():
    import inspect

    import kfmi
    from kfmi import engine
    assert callable(engine.BatchedKF.run_scores)
    assert engine.ScoredRun._fields == ('scores', 'traj', 'cov', 'logdet')
    for m in ('smooth_run', 'run_smoothed'):
        assert inspect.signature(getattr(engine.BatchedKF, m)).parameters['consts'].default is None
    sig = inspect.signature(engine.BatchedKF.run_scores).parameters
    assert [sig[k].default for k in ('consts', 'track', 'update_every', 'scores', 'traj', 'cov', 'logdet')] == \
        [None, None, 1, True, False, False, False]
    assert kfmi.cv_consts_table is engine.cv_consts_table


def test_cv_consts_table():
    from kfmi import KFError, engine
    t3 = engine.cv_consts_table('cv3', [(0.1, 0.2, (1.0, 2.0, 3.0)), dict(q_pos=0.3, q_vel=0.4, r=5.0)])
    assert t3.shape == (5, 2) and t3.dtype == np.float64
    assert np.array_equal(t3, np.array([[0.1, 0.3], [0.2, 0.4], [1.0, 5.0], [2.0, 5.0], [3.0, 5.0]]))
    t2 = engine.cv_consts_table('cv2', [(0.1, 0.2, [1.0, 2.0])] * 7)
    assert t2.shape == (4, 7)
    for model, sets in (('cv3', [(0.1, 0.2, (1.0, 2.0))]),        # r of the wrong length
                        ('cv2', [(0.1, 0.2)]),                     # no r
                        ('cv2', [dict(q_pos=0.1, r=1.0)]),         # a key missing
                        ('cv3', [(0.1, 'x', 1.0)]),                # not a number
                        ('ref15', [(0.1, 0.2, 1.0)])):             # not a CV model
        with pytest.raises(KFError) as e:
            engine.cv_consts_table(model, sets)
        assert e.value.code == _lib.KF_EINVAL and 'cv_consts_table' in str(e.value)


def test_innovation_nll_for_the_cv_models():
    from kfmi import engine
    sc = np.zeros((8, 2))
    sc[engine.SCORE_ROWS['gps_n']] = [4, 0]
    sc[engine.SCORE_ROWS['gps_nis']] = [10.0, 0.0]
    sc[engine.SCORE_ROWS['gps_logdet_s']] = [6.0, 0.0]
    for model, m in (('cv2', 2), ('cv3', 3)):
        nll = engine.innovation_nll(sc, model, 'gps')
        assert nll[0] == 0.5 * (16.0 + 4 * m * math.log(2 * math.pi)) and nll[1] == 0.0
    with pytest.raises(ValueError):
        engine.innovation_nll(sc, 'cv3', 'imu')
    assert engine.innovation_nll(sc, 'ref15', 'gps')[0] == 0.5 * (16.0 + 12 * math.log(2 * math.pi))
