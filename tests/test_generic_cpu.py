"""CPU: real-valued (generic) score tables, option exact_generic.  The oracle
replays the reference's recorded steps and trajectories on such tables
(tests/golden/make_generic_goldens.py) to the bit -- so the GPU tests
(test_gpu_exact_generic.py) may check against either -- and the limits table
and ``TableModel`` say what the option covers."""
import os
import random
import sys

import numpy as np
import pytest
from conftest import GOLDEN, golden

import nemo_oracle as no
from nemo import limits
from nemo.nem import TableModel

sys.path.insert(0, GOLDEN)
from generic_tables import KINDS, generic_tables, step_inputs, table_sha256  # noqa: E402


def fixture_tables(z, kind, prefix=None):
    """The fixture's tables, regenerated from its seed; the hash is checked."""
    p = f"{kind}_" if prefix is None else prefix
    seed = int(z[f"{p}seed"] if prefix is None else z["table_seed"])
    u, t = generic_tables(kind, int(z["S"]), int(z["E"]), seed)
    assert table_sha256(u, t) == str(z[f"{p}sha256"])
    return u, t


@pytest.mark.parametrize("name,cap", [("6x130", 0), ("9x300", 0), ("12x1000", 0), ("9x300_cap3", 3)])
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_equals_reference_generic_step(name, cap, kind):
    z = golden(f"generic_step_{name}.npz")
    assert int(z["cap"]) == cap
    u, t = fixture_tables(z, kind)
    perm, w = z[f"{kind}_perm"], z[f"{kind}_W"]
    if not cap:   # the inputs are step_inputs' (the GPU tests make them the same way)
        p2, w2 = step_inputs(int(z["S"]), int(z[f"{kind}_seed"]))
        assert np.array_equal(perm, p2) and np.array_equal(w, w2)
    ora = no.OracleSampler(u, t, perm, cap=cap)
    ora.w = w.copy()
    dag_ll = ora.optimal_weights()
    assert ora.ll1 == float(z[f"{kind}_ll1"])
    assert np.array_equal(ora.ow, z[f"{kind}_ow"])
    assert np.array_equal(ora.w, z[f"{kind}_W_new"])
    assert dag_ll == float(z[f"{kind}_dag_ll"])


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_equals_reference_generic_trajectory(kind):
    z = golden(f"generic_traj_9x300_{kind}.npz")
    u, t = fixture_tables(z, kind, prefix="")
    state = random.getstate()
    try:
        random.seed(int(z["seed"]))
        smp = no.OracleSampler(u, t, z["order0"])
        best = smp.method(swap_prob=float(z["swap_prob"]), gamma=float(z["gamma"]), n_iterations=int(z["n_iter"]))
        end = np.array(random.getstate()[1])
    finally:
        random.setstate(state)
    assert np.array_equal(np.array(smp.traj["perm"]), z["perm"])
    assert np.array_equal(np.array(smp.traj["i1"]), z["i1"]) and np.array_equal(np.array(smp.traj["i2"]), z["i2"])
    assert np.array_equal(np.array(smp.traj["acc"]), z["acc"])
    assert np.array_equal(np.array(smp.all_scores), z["all_scores"])
    assert best == float(z["best_score"]) and np.array_equal(smp.best_order, z["best_order"])
    assert np.array_equal(smp.w, z["final_W"])
    assert np.array_equal(end, z["rng_state_after"])


def test_generic_meta_records_versions():
    import json
    with open(os.path.join(GOLDEN, "generic_meta.json")) as fh:
        meta = json.load(fh)
    assert {"numpy", "scipy", "python"} <= set(meta)


def _status(**kw):
    a = dict(S=9, E=300, factored=False, cap=0, host_blas="SkylakeX", exact_option=True)
    a.update(kw)
    return limits.exact_status_from(limits.exact_limits(**a))


def test_exact_generic_limit_on_both_sides():
    assert _status(exact_generic=True) == (True, "")
    assert _status(E=8192, exact_generic=True) == (True, "")
    ok, why = _status(E=8193, exact_generic=True)
    assert not ok and why.startswith("table form") and "8192" in why and "700" in why
    assert _status(E=8193, factored=True, exact_generic=True) == (True, "")   # the factored kernels, any E
    assert _status(E=300, cap=3, exact_generic=True) == (True, "")
    ok, why = _status(exact_generic=True, exact_option=False)
    assert not ok and why.startswith("option exact")
    row = {r.name: r for r in limits.exact_limits(9, 300, False, exact_generic=True)}["table form"]
    assert row.covered and "8192" in row.outside and "700" in row.outside
    md = limits.limits_table_markdown(limits.exact_limits(9, 300, False, exact_generic=True))
    assert "exact_generic" in md and "8192" in md


def test_limits_without_the_option_are_unchanged():
    """exact_generic=False (the default): today's rows, whatever the table."""
    for fact in (True, False):
        for e in (300, 8192, 8193, 64 * 8192 + 1):
            assert limits.exact_limits(64, e, fact) == limits.exact_limits(64, e, fact, exact_generic=False)
    rows = limits.exact_limits(64, 2000, False)
    form = {r.name: r for r in rows}["table form"]
    assert not form.covered and form.value == "generic"
    assert form.bound == ("factored: every off-diagonal row T[.][j] shared by all children, two-valued "
                          "(every table nem.py builds)")
    assert form.outside == "ExactArithmeticWarning (strict=True: RuntimeError); the fast kernels"
    assert [r.name for r in rows] == ["option exact", "table form", "E (effects)", "parent cap",
                                      "S (S-genes), ancestor_x on the device"]
    ok, why = limits.exact_status_from(rows)
    assert not ok and why.startswith("table form")
    with pytest.raises(TypeError):   # keyword-only
        limits.exact_limits(64, 2000, False, 0, "SkylakeX", True, True)


def test_table_model_from_log_ratios():
    rng = np.random.default_rng(5)
    r = rng.normal(0, 1, (5, 37))
    m = TableModel.from_log_ratios(r)
    assert (m.num_s, m.num_e) == (5, 37) and m.observed_knockdown_mat is None
    assert m.U.shape == (6, 37) and np.array_equal(m.U[:5], r) and not m.U[5].any()
    t = m.get_score_tables(None)
    assert t is m.get_score_tables(m.observed_knockdown_mat) and t.shape == (5, 5, 37)
    for i in range(5):
        for j in range(5):
            assert np.array_equal(t[i][j], r[j])
    u, tt = generic_tables("shared", 5, 37, 5)   # the fixtures' "shared" kind is this model
    m2 = TableModel.from_log_ratios(u[:5])
    assert np.array_equal(m2.U, u) and np.array_equal(m2.T, tt)
    with pytest.raises(ValueError):
        TableModel(np.zeros((5, 37)), np.zeros((5, 5, 37)))
    with pytest.raises(ValueError):
        TableModel.from_log_ratios(np.zeros(7))
