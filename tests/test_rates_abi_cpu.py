"""nemo_score_rates / nemo_score_rates_dev without a GPU: the symbols, the
bindings, the refusals that need no device, and a loud failure (no CPU
fall-back) of everything built on them when no device is visible."""
import ctypes

import numpy as np
import pytest

NAMES = ("nemo_score_rates", "nemo_score_rates_dev")


@pytest.fixture(scope="module")
def lib():
    from nemo import _lib, build
    build.build()
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    from nemo import _lib
    bound = {name: args for name, _, args in _lib.SIGNATURES}
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in bound
    # (ctx, batch, pos, w01, rates, cap, ll, drates, grad[, stream])
    assert len(bound["nemo_score_rates"]) == 9 and len(bound["nemo_score_rates_dev"]) == 10


def test_engine_and_modules_expose_the_feature():
    from nemo import autograd, rates
    from nemo.engine import Engine
    assert callable(Engine.score_rates) and callable(Engine.score_rates_dev)
    assert callable(autograd.order_score_rates)
    assert callable(rates.fit_error_rates) and callable(rates.absolute_ll)


def test_null_context_is_refused(lib):
    from nemo import _lib
    buf = np.zeros(8)
    a = _lib.addr(buf)
    assert lib.nemo_score_rates(None, 1, a, a, a, 0, a, a, a) == _lib.NEMO_ERR_ARG
    assert b"null context" in lib.nemo_last_error()
    assert lib.nemo_score_rates_dev(None, 1, a, a, a, 0, a, a, a, None) == _lib.NEMO_ERR_ARG
    assert b"null context" in lib.nemo_last_error()
    assert not buf.any()


def test_no_device_means_loud_failure(lib):
    """Without a device nothing falls back to the CPU: the engine cannot be made, so neither
    the score nor the fit runs.  (With a device the same calls are tests/test_gpu_score_rates.py's.)"""
    from nemo import _lib
    from nemo.engine import Engine
    from nemo.rates import fit_error_rates
    d = np.array([[1, 0, 1, 1], [0, 0, 1, 0], [1, 1, 0, 0]], dtype=np.uint8)
    if _lib.device_count() == 0:
        with pytest.raises(_lib.NemoError, match="no HIP device"):
            Engine.from_knockdown(d, -1.0, -2.0)
        with pytest.raises(_lib.NemoError, match="no HIP device"):
            fit_error_rates(d, [0, 1, 2])
        ctx = ctypes.c_void_p()
        assert lib.nemo_ctx_create(0, 3, 4, _lib.NEMO_F64, ctypes.byref(ctx)) == _lib.NEMO_ERR_HIP
        assert not ctx.value


def test_fit_argument_checks_come_before_any_device_work():
    from nemo.rates import fit_error_rates
    d = np.zeros((3, 4), dtype=np.uint8)
    with pytest.raises(ValueError, match="permutation"):
        fit_error_rates(d, [0, 1, 1])
    with pytest.raises(ValueError, match="bounds"):
        fit_error_rates(d, [0, 1, 2], bounds=(0.5, 0.1))
    with pytest.raises(ValueError, match="errors0"):
        fit_error_rates(d, [0, 1, 2], errors0=(0.7, 0.2))
    with pytest.raises(ValueError, match="weights"):
        fit_error_rates(d, [0, 1, 2], weights=np.zeros((2, 2)))
