"""``real_score_ref`` (the numpy / scipy statement of the true-graph fit)
against the sweeps recorded from the reference programme
(``tests/golden/real_score_<name>.npz``): every sweep's ll and weights bit
for bit, the solves' iteration counts and initial gradients, and the three
outputs.  That makes it the CPU reference for inputs the reference programme
cannot take (``test_gpu_real_score.py``: a generic table, other shapes).

The small fixtures run the whole fit of both calls; the large ones
(network17, network13, 65x70) one recorded sweep per call -- the last, which starts from
recorded weights -- so the file stays at seconds.
"""
import os
import sys

import numpy as np
import pytest
from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import real_score_inputs as ri  # noqa: E402
import real_score_ref as rr  # noqa: E402

WHOLE = ["2x1", "3x5200", "net2", "network5"]
ONE_SWEEP = ["network17", "network13", "65x70"]


def pair_values(order, mat):
    return np.array([mat[i, j] for i, j in rr.pair_list(order)])


@pytest.mark.parametrize("name", WHOLE)
def test_whole_fit_equals_the_reference(name):
    g = golden(f"real_score_{name}.npz")
    nem = ri.build_nem(name)
    for call in ("real", "obs"):
        U, T = ri.call_tables(nem, call)
        order_ll, real_ll, order, f = rr.real_score(U, T, np.array(nem.adj_matrix))
        assert np.array_equal(order, g[f"{call}_parent_order"])
        assert np.array_equal(f["ll"], g[f"{call}_ll"])
        assert np.array_equal(f["w"], g[f"{call}_w"])
        assert np.array_equal(f["nit"], g[f"{call}_nit"])
        assert np.array_equal(f["g0"], g[f"{call}_g0"])
        assert order_ll == float(g[f"{call}_order_ll"])
        assert real_ll == float(g[f"{call}_real_ll"])


@pytest.mark.parametrize("name", ONE_SWEEP)
def test_one_sweep_equals_the_reference(name):
    g = golden(f"real_score_{name}.npz")
    nem = ri.build_nem(name)
    for call in ("real", "obs"):
        U, T = ri.call_tables(nem, call)
        order = g[f"{call}_parent_order"]
        assert np.array_equal(rr.parent_order_of(np.array(nem.adj_matrix)), order)
        k = len(g[f"{call}_ll"]) - 1
        assert k >= 1
        ll, w, nit, g0, _ = rr.sweep(U, T, order, g[f"{call}_w"][k - 1])
        assert ll == g[f"{call}_ll"][k]
        assert np.array_equal(w, g[f"{call}_w"][k])
        assert np.array_equal(nit, g[f"{call}_nit"][k])
        assert np.array_equal(g0, g[f"{call}_g0"][k])


def test_net2_outputs_are_the_recorded_constructor_values():
    """The four numbers make_goldens.py recorded from the reference's
    constructor for net2."""
    g = golden("real_score_net2.npz")
    t = golden("net2_tables.npz")
    assert float(g["real_order_ll"]) == float(t["real_order_ll"])
    assert float(g["real_real_ll"]) == float(t["real_ll"])
    assert float(g["obs_order_ll"]) == float(t["obs_order_ll"])
    assert float(g["obs_real_ll"]) == float(t["obs_ll"])


@pytest.mark.parametrize("name", list(ri.FIXTURES))
def test_fixture_margins(name):
    """The conditions that keep a GPU run's decisions the reference's, from
    the recorded data: the loop's test 100 ll tolerances from 1e-4, the last
    sweep's moved weights 10 weight tolerances from 0.5, every initial |g|
    100 d_g from 0.1."""
    g = golden(f"real_score_{name}.npz")
    ll_tol = max(10 * float(g["d_ll"]), 1e-6)
    w_tol = max(10 * float(g["d_w"]), 1e-6)
    for call in ("real", "obs"):
        assert np.all(np.abs(np.diff(g[f"{call}_ll"]) - 1e-4) > 100 * ll_tol)
        order = g[f"{call}_parent_order"]
        last = pair_values(order, g[f"{call}_w"][-1])
        moved = g[f"{call}_nit"][-1] > 0
        assert np.all(np.abs(last[moved] - 0.5) > 10 * w_tol)
        assert np.all(np.abs(np.abs(g[f"{call}_g0"]) - 0.1) > 100 * float(g["d_g"]))
        assert np.all(g[f"{call}_w"][:, rr.start_weights(order) == 0.0] == 0.0)
