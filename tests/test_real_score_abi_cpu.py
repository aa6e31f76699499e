"""The true-graph score surface without a GPU: ``nemo_real_sweep`` is exported
and bound, the product calls fail loudly where no device is visible (there is
no host fallback), and constructing a ``NEM`` still does no GPU work."""
import ctypes
import os

import numpy as np
import pytest
from conftest import GOLDEN, REPO

SIX = ("real_order_ll", "real_ll", "real_parent_order", "obs_order_ll", "obs_ll", "obs_parent_order")


@pytest.fixture(scope="module")
def lib():
    from nemo import _lib, build
    build.build()
    return _lib.load()


def net2_model():
    from nemo import NEM, utils
    adj, end, err, s, e = utils.read_csv_to_adj(os.path.join(GOLDEN, "network2.csv"))
    return NEM(adj, end, err, s, e)


def test_real_sweep_is_declared_exported_and_bound(lib):
    from nemo import _lib
    header = open(os.path.join(REPO, "include", "nemo.h")).read()
    assert "int nemo_real_sweep(nemo_ctx* ctx, int nprob, const int32_t* pos, const double* w, double* w_out," in header
    sig = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    res, args = sig["nemo_real_sweep"]
    assert res is ctypes.c_int and len(args) == 7
    getattr(ctypes.CDLL(lib._name), "nemo_real_sweep")   # plain C in the dynamic table
    assert lib.nemo_real_sweep.argtypes == args


def test_constructor_leaves_the_six_attributes_unset():
    m = net2_model()
    assert all(getattr(m, k) is None for k in SIX)
    assert "_nemo_engines" not in m.__dict__   # no engine was staged


def test_real_sweep_needs_a_context(lib):
    """The C entry refuses a null context whatever the machine."""
    from nemo import _lib
    pos = np.arange(3, dtype=np.int32)
    w = np.zeros((3, 3))
    out, ll = np.empty((3, 3)), np.empty(1)
    rc = lib.nemo_real_sweep(None, 1, _lib.ptr(pos, _lib._i32p), _lib.ptr(w), _lib.ptr(out), _lib.ptr(ll), None)
    assert rc == _lib.NEMO_ERR_ARG and b"null context" in lib.nemo_last_error()


def test_product_calls_raise_without_a_device(lib):
    from nemo import _lib
    from nemo.engine import Engine
    m = net2_model()
    if _lib.device_count() > 0:
        # a GPU is visible: the same calls must then work (tests/test_gpu_real_score.py holds their values)
        m.real_scores()
        assert all(getattr(m, k) is not None for k in SIX)
        return
    with pytest.raises(_lib.NemoError, match="no HIP device"):
        m.real_scores()
    assert all(getattr(m, k) is None for k in SIX)
    with pytest.raises(_lib.NemoError, match="no HIP device"):
        Engine.for_nem(m).real_sweep(np.arange(m.num_s), np.zeros((m.num_s, m.num_s)))
