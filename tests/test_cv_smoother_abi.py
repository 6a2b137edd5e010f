"""kf_run_rec / kf_smooth_run: exported, bound with the header's arity, and a NULL handle is
KF_EINVAL with a message that names the function (no GPU needed)."""
import re

from kfmi import _lib

NAMES = ('kf_run_rec', 'kf_smooth_run')


def _prototypes():
    text = re.sub(r'/\*.*?\*/', '', open(_lib.HEADER).read(), flags=re.S)
    return dict(re.findall(r'\b(kf_\w+)\s*\(([^;{]*?)\)\s*;', text))


def test_symbols_exported_and_bound_with_header_arity():
    protos = _prototypes()
    L = _lib.lib()
    for name in NAMES:
        assert name in protos, f'{name} not declared in include/kf.h'
        assert hasattr(L, name), f'{name} not exported'
        params = ' '.join(protos[name].split())
        assert len(_lib.SIGNATURES[name][1]) == params.count(',') + 1 == 12, (name, params)


def test_null_handle_is_einval_and_names_the_function():
    L = _lib.lib()
    assert L.kf_run_rec(None, 4, 0.1, None, None, None, None, 1, None, None, None, None) == _lib.KF_EINVAL
    assert 'kf_run_rec' in _lib.last_error() and 'null' in _lib.last_error()
    assert L.kf_smooth_run(None, 4, 0.1, None, None, None, None, None, None, None, None, None) == _lib.KF_EINVAL
    assert 'kf_smooth_run' in _lib.last_error() and 'null' in _lib.last_error()


def test_engine_has_the_three_methods():
    from kfmi import engine
    for m in ('run_rec', 'smooth_run', 'run_smoothed'):
        assert callable(getattr(engine.BatchedKF, m))
    assert engine.SmoothedRun._fields == ('x', 'P', 'logdet', 'status')
