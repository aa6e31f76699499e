"""CPU: row-shared real-valued tables (per-effect log ratios, T[i][j] = R[j];
option exact_generic) past one numpy buffer.  The oracle replays the
reference's recorded steps and trajectory at E = 9000 and 16500
(tests/golden/make_shared_goldens.py) to the bit, so the GPU tests
(test_gpu_exact_shared.py) may check against either; the limits table covers
such a table over the factored model's range of E; ``TableModel`` builds its
S*S*E tables only when they are read; and the host side of the staging
(csrc/nemo_host.h) is checked by a stand-alone program."""
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest
from conftest import GOLDEN, REPO, golden

import nemo_oracle as no
from nemo import limits
from nemo.nem import TableModel

sys.path.insert(0, GOLDEN)
from generic_tables import generic_tables, step_inputs, table_sha256  # noqa: E402


@pytest.mark.parametrize("name,parts", [("4x9000", [8192, 808]), ("3x16500", [8192, 8192, 116])])
def test_oracle_equals_reference_shared_step(name, parts):
    z = golden(f"shared_step_{name}.npz")
    s, e, seed = int(z["S"]), int(z["E"]), int(z["seed"])
    assert limits.pairwise_parts(e) == parts
    u, t = generic_tables("shared", s, e, seed)
    assert table_sha256(u, t) == str(z["sha256"])
    perm, w = step_inputs(s, seed)
    assert np.array_equal(z["perm"], perm) and np.array_equal(z["W"], w)
    ora = no.OracleSampler(u, t, perm)
    ora.w = w.copy()
    dag_ll = ora.optimal_weights()
    assert ora.ll1 == float(z["ll1"]) and dag_ll == float(z["dag_ll"])
    assert np.array_equal(ora.w, z["W_new"])
    _ow, ll, cs = no.calculate_ll(no.cell_ratios(u, t, no.parents_of(perm, 0), no.expit(w)))
    assert ll == float(z["ll1"]) and np.array_equal(cs, z["cs"])


def test_oracle_equals_reference_shared_trajectory():
    z = golden("shared_traj_5x9000.npz")
    u, t = generic_tables("shared", int(z["S"]), int(z["E"]), int(z["table_seed"]))
    assert table_sha256(u, t) == str(z["sha256"])
    state = random.getstate()
    try:
        random.seed(int(z["seed"]))
        smp = no.OracleSampler(u, t, z["order0"])
        best = smp.method(swap_prob=float(z["swap_prob"]), gamma=float(z["gamma"]), n_iterations=int(z["n_iter"]))
        end = np.array(random.getstate()[1])
    finally:
        random.setstate(state)
    assert np.array_equal(np.array(smp.traj["perm"]), z["perm"])
    assert np.array_equal(np.array(smp.traj["acc"]), z["acc"])
    assert np.array_equal(np.array(smp.all_scores), z["all_scores"])
    assert best == float(z["best_score"]) and np.array_equal(smp.best_order, z["best_order"])
    assert np.array_equal(smp.w, z["final_W"])
    assert np.array_equal(end, z["rng_state_after"])


def _status(**kw):
    a = dict(S=9, E=300, factored=False, cap=0, host_blas="SkylakeX", exact_option=True, exact_generic=True)
    a.update(kw)
    return limits.exact_status_from(limits.exact_limits(**a))


def test_row_shared_limit_on_both_sides():
    for e in (300, 8192, 8193, 9000, 64 * 8192):
        assert _status(E=e, row_shared=True) == (True, ""), e
        row = {r.name: r for r in limits.exact_limits(9, e, False, exact_generic=True, row_shared=True)}["table form"]
        assert row.covered and row.value == f"generic, rows shared, E={e}"
    ok, why = _status(E=64 * 8192 + 1, row_shared=True)
    assert not ok and why.startswith("table form") and "524288" in why and "700" in why
    assert _status(E=64 * 8192 + 1, row_shared=True, factored=True)[1].startswith("E (effects)")
    ok, why = _status(E=9000, row_shared=True, exact_option=False)
    assert not ok and why.startswith("option exact")
    # without the engine's option the flag changes nothing
    assert (limits.exact_limits(9, 9000, False, row_shared=True) == limits.exact_limits(9, 9000, False))
    with pytest.raises(TypeError):   # keyword-only
        limits.exact_limits(9, 9000, False, 0, "SkylakeX", True, True, True)


def test_limits_of_a_table_with_its_own_rows_are_unchanged():
    for fact in (True, False):
        for e in (300, 8192, 8193, 9000, 64 * 8192 + 1):
            for gen in (True, False):
                assert (limits.exact_limits(64, e, fact, exact_generic=gen, row_shared=False)
                        == limits.exact_limits(64, e, fact, exact_generic=gen))
    ok, why = _status(E=8193)
    assert not ok and why.startswith("table form") and "8192" in why
    assert _status(E=8192) == (True, "")


def test_table_model_builds_its_tables_lazily():
    rng = np.random.default_rng(6)
    r = rng.normal(0, 1, (5, 37))
    m = TableModel.from_log_ratios(r)
    assert m.tables_built is False and np.array_equal(m.R, r)
    assert (m.num_s, m.num_e) == (5, 37) and m.U.shape == (6, 37)
    assert m.tables_built is False
    t = m.T
    assert m.tables_built is True
    assert t.shape == (5, 5, 37) and np.array_equal(t, np.broadcast_to(r[None], (5, 5, 37)))
    assert m.T is t and m.get_score_tables(None) is t
    m2 = TableModel.from_log_ratios(r)
    assert m2.get_score_tables(None) is m2.T and m2.tables_built
    full = TableModel(m.U, t)   # a model given by its tables holds them from the start
    assert full.tables_built is True and full.R is None and full.T is not None


def test_shared_rows_host_check(tmp_path):
    """tests/host/shared_rows_check.cpp: the plan-ordered lv - 1 rows,
    row-shared detection and factored detection on R, for E in {130, 8192,
    8193, 8200, 16500}."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "shared_rows_check")
    subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-pthread",
                    f"-I{os.path.join(REPO, 'nem-mcmc-optimization_amd', 'csrc')}",
                    os.path.join(REPO, "tests", "host", "shared_rows_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert [ln.split(":")[0] for ln in r.stdout.splitlines()] == ["E=130", "E=8192", "E=8193", "E=8200", "E=16500"]
