"""``nemo_real_sweep`` (csrc/nemo_realscore.hip) and ``NEM.real_scores``
against the sweeps recorded from the reference programme
(``tests/golden/real_score_<name>.npz``) and, where that programme cannot run
(a generic table, other shapes), against its numpy / scipy statement
``real_score_ref`` (held to the recordings bit for bit on the CPU,
``test_real_score_cpu.py``).

Tolerances.  A fixture records the reference's own spread: ll, weights and
initial gradients under three other summations of its objective (long
double, reversed, log1p): d_ll, d_w, d_g.  The device differs in the log and
the algebra as well as in the order of the sum, so a sweep may differ by ten
times that spread, with the score kernels' 1e-6 as the floor:
ll within max(10 d_ll, 1e-6), weights within max(10 d_w, 1e-6).  Against
``real_score_ref`` (no recorded spread) the floor alone, 1e-6.  The final
scores are order scores at 0/1 weights: 1e-6, the score kernels' tolerance.
The fixtures keep every decision (the loop's test, the rounding at 0.5, the
nit = 0 exits) further from its threshold than these tolerances reach
(``test_real_score_cpu.py::test_fixture_margins``).
"""
import functools
import os
import sys

import numpy as np
import pytest
from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import real_score_inputs as ri  # noqa: E402
import real_score_ref as rr  # noqa: E402
from nemo import NEM, _lib, generator  # noqa: E402
from nemo.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = list(ri.FIXTURES)


@functools.lru_cache(maxsize=None)
def fixture_nem(name):
    return ri.build_nem(name)


def stacked_inputs(g, call):
    """Every recorded sweep's input weights: 0.5 on the pairs, then the
    weights after the sweep before."""
    order = g[f"{call}_parent_order"]
    w_after = g[f"{call}_w"]
    return order, np.concatenate([rr.start_weights(order)[None], w_after[:-1]])


@pytest.mark.parametrize("name", NAMES)
def test_sweep_parity(name):
    g = golden(f"real_score_{name}.npz")
    nem = fixture_nem(name)
    ll_tol = max(10 * float(g["d_ll"]), 1e-6)
    w_tol = max(10 * float(g["d_w"]), 1e-6)
    for call in ("real", "obs"):
        U, T = ri.call_tables(nem, call)
        eng = Engine(U, T)
        order, w_in = stacked_inputs(g, call)
        n = len(w_in)
        pos = np.tile(rr.positions(order), (n, 1))
        w_out, ll, info = eng.real_sweep(pos, w_in)
        pairs = rr.pair_list(order)
        ii, jj = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
        dev_ll = np.abs(ll - g[f"{call}_ll"]).max()
        dev_w = np.abs(w_out - g[f"{call}_w"]).max()
        nit = (info[:, ii, jj] >> 4) & 0xfff
        nfev = info[:, ii, jj] >> 16
        print(f"{name}/{call}: |dll| {dev_ll:.3g} (tol {ll_tol:.3g})  |dw| {dev_w:.3g} (tol {w_tol:.3g})  "
              f"nit differs at {(nit != g[f'{call}_nit']).sum()} of {nit.size}  f-evals per solve {nfev.mean():.2f}")
        assert dev_ll <= ll_tol
        assert dev_w <= w_tol
        still = g[f"{call}_nit"] == 0
        assert np.all(w_out[:, ii, jj][still] == 0.5)
        assert np.all(nit[still] == 0)
        off = rr.start_weights(order) == 0.0
        assert np.all(info[:, off] == -1) and np.all(w_out[:, off] == 0.0)
        eng.close()


@pytest.mark.parametrize("name", NAMES)
def test_real_scores_end_to_end(name):
    g = golden(f"real_score_{name}.npz")
    nem = ri.build_nem(name)   # a fresh model: real_scores fills its attributes
    assert nem.obs_ll is None
    nem.real_scores()
    for call, trace in (("real", nem.real_trace), ("obs", nem.obs_trace)):
        assert trace["sweeps"] == len(g[f"{call}_ll"])
        assert np.array_equal(trace["rounded"], 1.0 * (g[f"{call}_w"][-1] > 0.5))
    assert np.array_equal(nem.real_parent_order, g["real_parent_order"])
    assert np.array_equal(nem.obs_parent_order, g["obs_parent_order"])
    got = np.array([nem.real_order_ll, nem.real_ll, nem.obs_order_ll, nem.obs_ll])
    want = np.array([float(g[k]) for k in ("real_order_ll", "real_real_ll", "obs_order_ll", "obs_real_ll")])
    print(f"{name}: |d score| {np.abs(got - want).max():.3g}")
    assert np.abs(got - want).max() <= 1e-6
    if name == "net2":
        t = golden("net2_tables.npz")
        rec = np.array([float(t[k]) for k in ("real_order_ll", "real_ll", "obs_order_ll", "obs_ll")])
        assert np.abs(got - rec).max() <= 1e-6


def perturbed_net2():
    """net2's observed tables with one child's row made real-valued: staging
    finds no factored structure, so the generic instantiation runs."""
    nem = fixture_nem("net2")
    U, T = ri.call_tables(nem, "obs")
    T = T.copy()
    T[4, 7] += 0.05 * np.sin(np.arange(T.shape[2]))
    return nem, U, T


def test_generic_instantiation():
    nem, U, T = perturbed_net2()
    eng = Engine(U, T)
    assert not eng.factored
    order = rr.parent_order_of(np.array(nem.adj_matrix))
    rng = np.random.default_rng(5)
    starts = [rr.start_weights(order), np.where(rr.start_weights(order) > 0, rng.random(T.shape[:2]), 0.0)]
    for w0 in starts:
        ll_ref, w_ref, nit_ref, _, _ = rr.sweep(U, T, order, w0)
        w_out, ll, info = eng.real_sweep(rr.positions(order), w0)
        print(f"generic: |dll| {abs(ll[0] - ll_ref):.3g}  |dw| {np.abs(w_out[0] - w_ref).max():.3g}")
        assert abs(ll[0] - ll_ref) <= 1e-6
        assert np.abs(w_out[0] - w_ref).max() <= 1e-6
    eng.close()


@pytest.mark.parametrize("generic", [False, True])
def test_bits_do_not_depend_on_the_batch_or_the_run(generic):
    if generic:
        _, U, T = perturbed_net2()
    else:
        U, T = ri.call_tables(fixture_nem("net2"), "obs")
    s = T.shape[0]
    eng = Engine(U, T)
    rng = np.random.default_rng(11)
    orders = [rng.permutation(s) for _ in range(3)]
    pos = np.array([rr.positions(o) for o in orders])
    w = np.array([np.where(rr.start_weights(o) > 0, rng.random((s, s)), 0.0) for o in orders])
    w3, ll3, info3 = eng.real_sweep(pos, w)
    for k in (2, 0, 1):
        w1, ll1, info1 = eng.real_sweep(pos[k], w[k])
        assert np.array_equal(w1[0], w3[k]) and ll1[0] == ll3[k] and np.array_equal(info1[0], info3[k])
    again = eng.real_sweep(pos, w)
    assert np.array_equal(again[0], w3) and np.array_equal(again[1], ll3) and np.array_equal(again[2], info3)
    eng.close()


@pytest.mark.parametrize("e", [1, 63, 64, 65, 257])
def test_effect_counts_around_the_wave_and_the_block(e):
    nem = generator.synthetic_nem(3, e, 2, edge_p=0.6)
    U, T = ri.call_tables(nem, "obs")
    order = rr.parent_order_of(np.array(nem.adj_matrix))
    w0 = rr.start_weights(order)
    ll_ref, w_ref, _, _, _ = rr.sweep(U, T, order, w0)
    eng = Engine(U, T)
    w_out, ll, _ = eng.real_sweep(rr.positions(order), w0)
    print(f"E={e}: |dll| {abs(ll[0] - ll_ref):.3g}  |dw| {np.abs(w_out[0] - w_ref).max():.3g}")
    assert abs(ll[0] - ll_ref) <= 1e-6
    assert np.abs(w_out[0] - w_ref).max() <= 1e-6
    eng.close()


def test_run_network_reports_the_observed_score():
    from nemo.main import run_network
    r = run_network(os.path.join(GOLDEN, "network2.csv"), real_score=True)
    t = golden("net2_tables.npz")
    assert abs(r["observed_score"] - float(t["obs_ll"])) <= 1e-6
    assert abs(r["observed_order_score"] - float(t["obs_order_ll"])) <= 1e-6


def test_backward_edge_raises():
    # 0 -> 1 with 1 -> 2, 1 -> 3: node 1 has the larger row sum, so the edge
    # 0 -> 1 points backwards in parent_order (not a closure)
    adj = np.zeros((4, 4), dtype=int)
    adj[0, 1] = adj[1, 2] = adj[1, 3] = 1
    nem = NEM(adj, np.arange(8) % 4, (0.05, 0.1), 4, 8)
    with pytest.raises(ValueError, match="0->1"):
        nem.real_scores()
    assert nem.obs_ll is None


def test_fp32_context_is_refused():
    U, T = ri.call_tables(fixture_nem("net2"), "obs")
    eng = Engine(U, T, dtype="f32")
    order = np.arange(T.shape[0])
    with pytest.raises(_lib.NemoError, match="fp64 only") as ei:
        eng.real_sweep(rr.positions(order), rr.start_weights(order))
    assert ei.value.code == _lib.NEMO_ERR_ARG
    eng.close()
