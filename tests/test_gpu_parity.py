"""GPU parity: the HIP kernels (through the C-ABI) against the reference's
golden vectors and the pinned oracle.  Tolerances (north_star): log-scores
within 1e-6 absolute in fp64; the fp32 table path (C5) within 1e-6 relative;
accepted-move indices of the sampler identical under the reference's seed."""
import os
import random

import numpy as np
import pytest
from conftest import golden
from scipy.special import expit

import nemo_oracle as no
from nemo import NEM, _lib, generator, utils
from nemo.engine import Engine, lse_full

pytestmark = pytest.mark.gpu

LL_TOL = 1e-6


def _pos(perm):
    perm = np.asarray(perm)
    pos = np.empty(len(perm), dtype=np.int32)
    pos[perm] = np.arange(len(perm))
    return pos


def _unpack_d(z):
    s, e = int(z["S"]), int(z["E"])
    return np.unpackbits(z["D_packed"])[: s * e].reshape(s, e).astype(np.float64)


@pytest.fixture(scope="module")
def net2_engine():
    z = golden("net2_tables.npz")
    return Engine(z["U"], z["T"]), z


@pytest.fixture(scope="module")
def c3_model():
    m = generator.synthetic_nem(64, 2000, 0)
    return m, Engine.for_nem(m)


def _golden_batch(z):
    pos = np.array([_pos(p) for p in z["perm"]])
    return pos, expit(z["W"])


def test_score_net2_golden(net2_engine):
    eng, t = net2_engine
    z = golden("eval_net2.npz")
    pos, w01 = _golden_batch(z)
    out = eng.score(pos, w01, want_cs=True, want_cells=True, want_ow=True)
    assert np.max(np.abs(out["ll"] - z["ll"])) <= 1e-9
    assert np.max(np.abs(out["cs"] - z["cs"])) <= 1e-11
    assert np.max(np.abs(out["ow"][0] - z["ow0"])) <= 1e-12
    for c in range(len(pos)):
        cell = no.cell_ratios(t["U"], t["T"], no.parents_of(z["perm"][c]), w01[c])
        assert np.max(np.abs(out["cells"][c] - cell)) <= 1e-11
    # ll-only calls (the pipelined kernel) agree with the full-output kernel,
    # and single-eval calls give the same bits as the batch
    ll = eng.score(pos, w01)
    assert np.max(np.abs(ll - out["ll"])) <= 1e-9
    for c in (0, 5):
        assert eng.score(pos[c:c + 1], w01[c:c + 1])[0] == ll[c]


@pytest.mark.parametrize("name,s,e", [("C2", 16, 500), ("C3", 64, 2000)])
def test_score_synthetic_golden(name, s, e):
    z = golden(f"eval_{name}.npz")
    m = generator.synthetic_nem(s, e, 0)
    assert np.array_equal(m.observed_knockdown_mat, _unpack_d(z))
    eng = Engine.for_nem(m)
    pos, w01 = _golden_batch(z)
    # the fast kernels (option exact 0; the default exact arithmetic gives the
    # goldens' bits: test_gpu_exact.py)
    eng.set_option("exact", 0)
    try:
        out = eng.score(pos, w01, want_cs=True, want_ow=True)
        assert np.max(np.abs(out["ll"] - z["ll"])) <= LL_TOL
        # ll-only calls take the int8 log2 offset kernel (U folded into the
        # contraction): fact_kernel 10, within its own error bound
        assert eng.get_option("i8o") == 2
        fk, bound = eng.score_kernel(0, True)
        assert fk == 10 and bound <= 1e-7
        assert np.max(np.abs(eng.score(pos, w01) - z["ll"])) <= min(LL_TOL, bound)
        assert np.max(np.abs(out["cs"] - z["cs"])) <= 1e-9
        assert np.max(np.abs(out["ow"][0] - z["ow0"])) <= 1e-11
        np.testing.assert_allclose(out["ow"].sum(axis=1), 1.0, atol=1e-12)
    finally:
        eng.set_option("exact", 1)


def test_score_c5_cap6_f64_and_f32():
    z = golden("eval_C5cap.npz")
    m = generator.synthetic_nem(128, 5000, 0)
    assert np.array_equal(m.observed_knockdown_mat, _unpack_d(z))
    pos, w01 = _golden_batch(z)
    e64 = Engine.for_nem(m, dtype="f64")
    ll64 = e64.score(pos, w01, cap=6)
    assert np.max(np.abs(ll64 - z["ll"])) <= LL_TOL
    e64.close()
    e32 = Engine.for_nem(m, dtype="f32")
    ll32 = e32.score(pos, w01, cap=6)
    # fp32 storage and products, fp64 logs / LSE / effect sum
    assert np.max(np.abs(ll32 - z["ll"]) / np.abs(z["ll"])) <= 1e-6
    e32.close()


def test_full_size_properties_c3(c3_model):
    m, eng = c3_model
    s = m.num_s
    b = 48
    rng = np.random.default_rng(9)
    pos = np.array([rng.permutation(s) for _ in range(b)], dtype=np.int32)
    w01 = expit(rng.uniform(-3, 3, (b, s, s)))
    ll = eng.score(pos, w01)
    # deterministic, batch-position invariant
    assert np.array_equal(eng.score(pos, w01), ll)
    assert np.array_equal(eng.score(pos[::-1], w01[::-1]), ll[::-1])
    # zero weights: every cell is U, ll = sum_e logsumexp(U[:, e])
    ll0 = eng.score(pos[:2], np.zeros((2, s, s)))
    ref0 = sum(np.logaddexp.reduce(m.U, axis=0))
    assert np.max(np.abs(ll0 - ref0)) <= 1e-9
    # oracle on a few of them
    t = m.get_score_tensor()
    for c in (0, 17):
        perm = np.argsort(pos[c])
        ref = no.order_score(m.U, t, perm, w01[c])
        assert abs(ll[c] - ref) <= LL_TOL


def test_group_kernel_matches_stream(c3_model):
    import torch
    m, eng = c3_model
    s = m.num_s
    b = 40
    rng = np.random.default_rng(4)
    pos = np.array([rng.permutation(s) for _ in range(b)], dtype=np.int32)
    w01 = expit(rng.uniform(-3, 3, (b, s, s)))
    ref = eng.score(pos, w01)
    eng.reserve(b)
    dpos = torch.from_numpy(pos).cuda()
    dw = torch.from_numpy(w01).cuda()
    for g in (1, 4, 8, 16):
        dll = torch.zeros(b, dtype=torch.float64, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        eng.score_dev(b, dpos.data_ptr(), dw.data_ptr(), dll.data_ptr(), stream=st, group=g)
        torch.cuda.synchronize()
        got = dll.cpu().numpy()
        assert np.max(np.abs(got - ref) / np.abs(ref)) <= 1e-13, g


def test_lse_kernel_matches_numpy():
    rng = np.random.default_rng(2)
    cells = rng.normal(-50, 20, (33, 300))
    cells[3, 7] = -np.inf
    ll, cs, ow = lse_full(cells)
    ref_cs = np.logaddexp.reduce(cells, axis=0)
    assert np.max(np.abs(cs - ref_cs)) <= 1e-12
    assert abs(ll - sum(ref_cs)) <= 1e-9
    assert np.max(np.abs(ow - np.exp(cells - ref_cs))) <= 1e-12
    assert abs(utils.compute_ll(cells) - sum(ref_cs)) <= 1e-9


@pytest.mark.parametrize("name", ["net2_200", "C2_20"])
@pytest.mark.parametrize("prod", [1, 0])
def test_local_opt_vs_scipy_records(name, prod):
    """prod 1: the objective's sum of logs as one log of a product per lane
    (the default); 0: a log per element."""
    z = golden(f"localopt_{name}.npz")
    e = z["c"].shape[1]
    eng = Engine(np.zeros((3, e)), np.zeros((2, 2, e)))
    eng.set_option("exact", 0)   # the fast objective (test_gpu_exact.py: the exact one, bit for bit)
    eng.set_option("local_prod", prod)
    xs, fs, nit, nfev, st = eng.local_opt(z["c"], z["anc"], z["x0"])
    assert np.all(st <= 1)
    same = (nit == z["nit"]) & (nfev == z["nfev"])
    # every recorded problem follows scipy's iteration path
    assert same.all(), f"{int((~same).sum())} of {same.size} problems left scipy's (nit, nfev) path"
    rel = np.abs(xs - z["xstar"]) / np.maximum(1, np.abs(z["xstar"]))
    assert np.max(rel[same]) <= 1e-3
    assert np.array_equal(np.sign(xs), np.sign(z["xstar"]))
    # f* at an x* that differs by forward-difference noise (~1e-5 rel.)
    np.testing.assert_allclose(fs[same], z["fun"][same], rtol=1e-6, atol=1e-6)


def _oracle_step_inputs(u, t, perm, w_raw):
    smp = no.OracleSampler(u, t, perm)
    smp.w = w_raw.copy()
    return smp


def test_fused_step_vs_oracle_c3(c3_model):
    """One get_optimal_weights at 64x2000 (2016 local optima) vs the oracle,
    with the fast kernels (option exact = 0; the default exact arithmetic:
    test_gpu_exact.py, every weight to the bit)."""
    from nemo.nem_order_mcmc import NEMOrderMCMC
    m, eng = c3_model
    eng.set_option("exact", 0)
    try:
        t = m.get_score_tensor()
        rng = np.random.default_rng(12)
        perm = rng.permutation(m.num_s)
        smp = NEMOrderMCMC(m, perm, engine=eng)
        w_raw = rng.uniform(-3, 3, (m.num_s, m.num_s))
        smp.parent_weights = w_raw.copy()
        ora = _oracle_step_inputs(m.U, t, perm, w_raw)
        ref_dag = ora.optimal_weights()
        got_dag = smp.get_optimal_weights(init=True)
        assert abs(smp.ll - ora.ll1) <= LL_TOL
        mask = smp._mask
        assert np.array_equal(smp.parent_weights[~mask], ora.w[~mask])
        dw = np.abs(smp.parent_weights[mask] - ora.w[mask])
        # 16 of the 2016 optima differ from scipy's by more than 1e-6 (max
        # 8.5e-3, tools/parity_stats.py): the order weights differ from
        # numpy's in the last bits and the forward-difference gradient (h =
        # 1e-8) amplifies that into another line-search path; every binarised
        # weight is the same
        assert int((dw > 1e-6).sum()) <= 16 and dw.max() <= 1e-2
        assert np.array_equal(smp.parent_weights[mask] > 0.5, ora.w[mask] > 0.5)
        assert abs(got_dag - ref_dag) <= LL_TOL
    finally:
        eng.set_option("exact", 1)


def _run_sampler(m, order, gamma, swap_prob, n, state):
    from nemo.nem_order_mcmc import NEMOrderMCMC
    random.setstate(state)
    smp = NEMOrderMCMC(m, order)
    best, _ = smp.method(n_iterations=n, gamma=gamma, swap_prob=swap_prob, verbose=False)
    return smp, best


def test_trajectory_net2_200(net2):
    """C1: 200 MCMC steps on network2 with the reference's seed: identical
    accepted moves, scores within 1e-6."""
    m, state = net2
    z = golden("traj_net2_200.npz")
    smp, best = _run_sampler(m, z["order0"], float(z["gamma"]), float(z["swap_prob"]),
                             int(z["n_iter"]), state)
    assert np.array_equal(np.array(smp.accepted), z["acc"])
    scores = np.array(smp.all_score_list)
    # the reference's arithmetic (option exact, the default): every score,
    # the best score and the final weights to the bit
    assert np.array_equal(scores, z["all_scores"])
    assert best == float(z["best_score"])
    assert np.array_equal(smp.best_order, z["best_order"])
    assert np.array_equal(np.array(random.getstate()[1]), z["rng_state_after"])
    assert np.array_equal(smp.parent_weights, z["final_W"])


def test_trajectory_net2_use_nem_50(net2):
    """method(use_nem=True): the transitive-closure DAG scores eval #2 and
    the accept step (nem_order_mcmc.py:203-204, 283-284; utils.py:37-54).
    50 steps on network2 with the reference's seed (make_goldens.py
    --only-traj-nem): identical proposals and accepted moves, scores within
    1e-6, the same best score, order and (closure) DAG, the same random
    state after the run."""
    m, state = net2
    z = golden("traj_net2_nem_50.npz")
    assert bool(z["use_nem"])
    from nemo.nem_order_mcmc import NEMOrderMCMC
    random.setstate(state)
    smp = NEMOrderMCMC(m, z["order0"])
    best, best_dag = smp.method(n_iterations=int(z["n_iter"]), gamma=float(z["gamma"]),
                                swap_prob=float(z["swap_prob"]), verbose=False, use_nem=True)
    assert np.array_equal(np.array(smp.accepted), z["acc"])
    assert np.array_equal(np.array(smp.all_score_list), z["all_scores"])
    assert best == float(z["best_score"])
    assert np.array_equal(smp.best_order, z["best_order"])
    assert np.array_equal(np.asarray(best_dag), z["best_dag"])
    assert np.array_equal(np.array(random.getstate()[1]), z["rng_state_after"])
    assert np.array_equal(smp.parent_weights, z["final_W"])


def test_trajectory_c2_20():
    z = golden("traj_C2_20.npz")
    m = generator.synthetic_nem(16, 500, 0)
    state = random.getstate()
    smp, best = _run_sampler(m, z["order0"], float(z["gamma"]), float(z["swap_prob"]),
                             int(z["n_iter"]), state)
    assert np.array_equal(np.array(smp.accepted), z["acc"])
    assert np.array_equal(np.array(smp.all_score_list), z["all_scores"])
    assert np.array_equal(smp.parent_weights, z["final_W"])


@pytest.mark.parametrize("n", [20, 100])
def test_trajectory_c3(n):
    """C3, the headline model (64 x 2000): n steps of the reference's method()
    with its seed (tests/golden/make_goldens.py --only-traj-c3 n), in the
    reference's own arithmetic (option exact, the default): identical
    proposals and accepted moves, and every score, the best score and order,
    the final random state and the final weights (every step's 2016 local
    optima carried into the next) equal to the reference's to the bit."""
    z = golden(f"traj_C3_{n}.npz")
    m = generator.synthetic_nem(64, 2000, 0)
    state = random.getstate()
    smp, best = _run_sampler(m, z["order0"], float(z["gamma"]), float(z["swap_prob"]),
                             int(z["n_iter"]), state)
    assert np.array_equal(np.array(smp.accepted), z["acc"])
    d = np.array(smp.all_score_list) != z["all_scores"]
    assert not d.any(), np.where(d)[0].tolist()
    assert best == float(z["best_score"])
    assert np.array_equal(smp.best_order, z["best_order"])
    assert np.array_equal(np.array(random.getstate()[1]), z["rng_state_after"])
    assert np.array_equal(smp.parent_weights, z["final_W"])


def _record_sampler(smp):
    """Per-step proposals, accepts and scores of a mirror sampler, kept even
    when method() raises (the reference's golden keeps them the same way)."""
    rec = {"perm": [], "acc": [], "scores": []}
    new, acc, gow = smp.get_new_order, smp.accepting, smp.get_optimal_weights

    def get_new_order(curr, swap_prob=0.95):
        r = new(curr, swap_prob=swap_prob)
        rec["perm"].append(np.array(r[0]))
        return r

    def accepting(*a):
        r = acc(*a)
        rec["acc"].append(bool(r[0]))
        return r

    def get_optimal_weights(*a, **k):
        r = gow(*a, **k)
        rec["scores"].append(r)
        return r

    smp.get_new_order, smp.accepting, smp.get_optimal_weights = get_new_order, accepting, get_optimal_weights
    return rec


def test_trajectory_c3_until_the_reference_raises():
    """C3 with the reference's default n_iterations = 500: the reference's own
    run ends in step 128, when one of that step's local optimisations
    terminates abnormally and method() raises (nem_order_mcmc.py:168-169;
    make_goldens.py --only-traj-c3 500).  The mirror makes the same 128
    proposals and 127 accept decisions, scores every completed step to the
    bit, and raises in the same step with the same weights."""
    from nemo.nem_order_mcmc import NEMOrderMCMC
    z = golden("traj_C3_500.npz")
    m = generator.synthetic_nem(64, 2000, 0)
    smp = NEMOrderMCMC(m, z["order0"])
    rec = _record_sampler(smp)
    with pytest.raises(Exception, match="Minimization not successful"):
        smp.method(n_iterations=int(z["n_iter"]), gamma=float(z["gamma"]), swap_prob=float(z["swap_prob"]),
                   verbose=False)
    assert len(rec["perm"]) == int(z["raised_in_step"])
    assert np.array_equal(np.array(rec["perm"]), z["perm"])
    assert np.array_equal(np.array(rec["acc"]), z["acc"])
    got = np.array(rec["scores"][1:1 + int(z["steps_completed"])])
    off = np.where(got != z["step_scores"])[0].tolist()
    print("C3 steps whose score differs from the reference's:", off)
    assert not off, off
    assert np.array_equal(smp.parent_weights, z["W_at_raise"])


def test_edge_cases():
    # smallest model, E not a multiple of the 64-effect tile, E = 1
    for s, e in ((2, 1), (3, 65), (5, 130)):
        m = generator.synthetic_nem(s, e, 1)
        t = m.get_score_tensor()
        eng = Engine(m.U, t)
        rng = np.random.default_rng(s * e)
        perms = [rng.permutation(s) for _ in range(3)]
        w01 = expit(rng.uniform(-3, 3, (3, s, s)))
        ll = eng.score(np.array([_pos(p) for p in perms]), w01)
        for c in range(3):
            assert abs(ll[c] - no.order_score(m.U, t, perms[c], w01[c])) <= 1e-9
        # a cap at least S-1 is no cap
        assert np.array_equal(eng.score(np.array([_pos(p) for p in perms]), w01, cap=s), ll)
        eng.close()
    m = generator.synthetic_nem(4, 10, 0)
    eng = Engine(m.U, m.get_score_tensor())
    assert eng.score(np.zeros((0, 4), dtype=np.int32), np.zeros((0, 4, 4))).shape == (0,)
    with pytest.raises(RuntimeError, match="permutation"):
        eng.score(np.array([[0, 0, 1, 2]]), np.zeros((1, 4, 4)))


def test_chain_batch_equals_single_chains():
    """Lock-step batching (one fused call for all chains) reproduces each
    chain's single-chain run driven by the same random stream, bit for bit."""
    from nemo.chains import ChainBatch
    from nemo.nem_order_mcmc import NEMOrderMCMC
    m = generator.synthetic_nem(16, 500, 0)
    nc = 7
    orders = [np.random.default_rng(k).permutation(16) for k in range(nc)]
    seeds = [11 + k for k in range(nc)]
    cb = ChainBatch(m, orders, seeds, swap_prob=0.95)
    best, best_orders = cb.run(8)
    for k in range(nc):
        single = NEMOrderMCMC(m, orders[k], engine=cb.engine)
        single.rng = random.Random(seeds[k])
        b, _ = single.method(n_iterations=8, gamma=cb.gamma, swap_prob=0.95, verbose=False)
        assert np.array_equal(np.array(single.accepted), cb.accepted[:, k])
        assert b == best[k]
        assert np.array_equal(single.best_order, best_orders[k])
        c = cb.chains[k]
        assert np.array_equal(single.best_dag, c.best_dag) and single.best_dag.dtype == c.best_dag.dtype
        assert single.all_score_list == c.all_score_list and single.curr_score_list == c.curr_score_list
        assert single.best_score_list == c.best_score_list
        assert all(np.array_equal(x, y) for x, y in zip(single.parents_list, c.parents_list))
        assert np.array_equal(single.parent_weights, c.parent_weights)
    # three pipeline groups, one group: the same trajectories
    for g in (3, 1):
        cbg = ChainBatch(m, orders, seeds, swap_prob=0.95, engine=cb.engine, groups=g)
        bg, bog = cbg.run(8)
        assert np.array_equal(bg, best) and np.array_equal(bog, best_orders)
        assert np.array_equal(cbg.accepted, cb.accepted)
    # ancestor_x inversions in worker processes: the same trajectories
    from nemo.invpool import InvPool
    pool = InvPool(16, nc, n_workers=2)
    try:
        cbp = ChainBatch(m, orders, seeds, swap_prob=0.95, engine=cb.engine, inv_pool=pool)
        bp, bop = cbp.run(8)
    finally:
        pool.close()
    assert np.array_equal(bp, best) and np.array_equal(bop, best_orders)
    assert np.array_equal(cbp.accepted, cb.accepted)


def test_pipelined_chain_groups_equal_one_batch():
    """48 chains in three pipelined groups of 16: each group's fused step is
    queued on the library thread (two steps in flight, staging slots 1 and 2);
    the trajectories equal one synchronous batch of all 48."""
    from nemo.chains import ChainBatch
    m = generator.synthetic_nem(16, 500, 3)
    nc = 48
    orders = [np.random.default_rng(100 + k).permutation(16) for k in range(nc)]
    seeds = [500 + k for k in range(nc)]
    one = ChainBatch(m, orders, seeds, swap_prob=0.9, groups=1, on_fail="continue")
    b1, o1 = one.run(6)
    grp = ChainBatch(m, orders, seeds, swap_prob=0.9, groups=3, engine=one.engine, on_fail="continue")
    b3, o3 = grp.run(6)
    assert np.array_equal(b1, b3) and np.array_equal(o1, o3)
    assert np.array_equal(one.accepted, grp.accepted)
    for c1, c3 in zip(one.chains, grp.chains):
        assert np.array_equal(c1.parent_weights, c3.parent_weights)
        assert c1.all_score_list == c3.all_score_list


@pytest.mark.parametrize("name,s,e,cap", [("net2", 11, 184, 0), ("C2", 16, 500, 0), ("C3", 64, 2000, 0),
                                          ("C5cap", 128, 5000, 6)])
def test_factored_mfma_path_vs_golden_and_stream(name, s, e, cap):
    """The factored MFMA kernel (score_path=2) against the reference goldens
    and against the streaming kernel (score_path=1) on the same inputs."""
    z = golden(f"eval_{name}.npz")
    if name == "net2":
        t = golden("net2_tables.npz")
        eng = Engine(t["U"], t["T"])
    else:
        m = generator.synthetic_nem(s, e, 0)
        eng = Engine(m.U, m.get_score_tensor())
    assert eng.factored
    pos, w01 = _golden_batch(z)
    eng.set_option("score_path", 2)
    f = eng.score(pos, w01, cap=cap, want_cs=True, want_cells=True, want_ow=True)
    eng.set_option("score_path", 1)
    st = eng.score(pos, w01, cap=cap, want_cs=True, want_cells=True, want_ow=True)
    assert np.max(np.abs(f["ll"] - z["ll"])) <= LL_TOL
    assert np.max(np.abs(f["cs"] - z["cs"])) <= 1e-9
    assert np.max(np.abs(f["cells"] - st["cells"])) <= 1e-10
    assert np.max(np.abs(f["ow"] - st["ow"])) <= 1e-12
    if "ow0" in z.files:
        assert np.max(np.abs(f["ow"][0] - z["ow0"])) <= 1e-11
    eng.close()


def test_factored_detection_rejects_generic_tables():
    rng = np.random.default_rng(8)
    s, e = 6, 70
    t = rng.normal(0, 1, (s, s, e))
    u = rng.normal(-5, 1, (s + 1, e))
    eng = Engine(u, t)
    assert not eng.factored
    eng.set_option("score_path", 2)
    with pytest.raises(RuntimeError, match="not factorable"):
        eng.score(np.arange(s, dtype=np.int32)[None], np.full((1, s, s), 0.5))
    eng.set_option("score_path", 0)  # auto -> stream
    perm = rng.permutation(s)
    w01 = rng.random((s, s))
    ll = eng.score(_pos(perm)[None], w01[None])[0]
    assert abs(ll - no.order_score(u, t, perm, w01)) <= 1e-9


@pytest.mark.parametrize("s,e", [(2, 1), (11, 184), (16, 500), (33, 17), (40, 333), (64, 2000)])
def test_factored_kernel_variants_agree(s, e):
    """Chunked (fact_kernel=1), f64 pipelined (2: 4 waves, 3: 8 waves) and
    int8 fixed-point (4: 4 digit pairs, 5: 5 pairs, 6: 4 pairs x 8 waves,
    7 / 8: offset log-sum-exp with 4 / 8 waves, 10 / 11: the same in log2
    fixed point with 8 / 4 waves) factored kernels against the streaming kernel and the oracle: padding rows
    (S % 16 != 0), ragged last tile (E % 16 != 0), tiny E; the pipelined
    kernel's bits do not depend on the batch size."""
    m = generator.synthetic_nem(s, e, 3)
    t = m.get_score_tensor()
    eng = Engine(m.U, t)
    assert eng.factored
    rng = np.random.default_rng(s + e)
    b = 37
    perms = [rng.permutation(s) for _ in range(b)]
    pos = np.array([_pos(p) for p in perms])
    w01 = expit(rng.uniform(-4, 4, (b, s, s)))
    variants = ((1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (7, 1), (8, 1),
                (10, 0), (11, 0), (12, 0), (13, 0), (14, 0), (16, 0))
    for cap in (0, 5):
        eng.set_option("score_path", 1)
        ref = eng.score(pos, w01, cap=cap)
        eng.set_option("score_path", 2)
        # nem.py's U: U - U[S] is two-valued per row, so the offset kernels
        # fold it into the contraction (i8o 2); i8o_nodiag keeps its loads
        assert eng.get_option("i8o") == (2 if s <= 64 else 0)
        assert eng.get_option("i8l") == (1 if s <= 64 else 0)
        for fk, nodiag in variants:
            eng.set_option("fact_kernel", fk)
            eng.set_option("i8o_nodiag", nodiag)
            ll = eng.score(pos, w01, cap=cap)
            # 10 / 11 carry the fraction of each entry to 2^-38 / ln 2 (7 slices;
            # DESIGN.md 3.1e): ~1e-9 at 64 x 2000, the others ~1e-11
            tol = 1e-8 if fk >= 10 else 1e-9
            assert np.max(np.abs(ll - ref)) <= tol, (fk, cap)
            for c in (0, 11, 36):
                assert eng.score(pos[c:c + 1], w01[c:c + 1], cap=cap)[0] == ll[c], (fk, cap)
        eng.set_option("i8o_nodiag", 0)
    ll = eng.score(pos, w01)   # fact_kernel 11 (log2 fixed point)
    for c in (0, 1):
        assert abs(ll[c] - no.order_score(m.U, t, perms[c], w01[c])) <= 1e-8
    # zero and one weights (G, Delta at their extremes)
    # (what L-BFGS-B's bounds hand the kernels): every variant, each within its tolerance above
    for w in (0.0, 1.0):
        wz = np.full((2, s, s), w)
        eng.set_option("score_path", 1)
        ref = eng.score(pos[:2], wz)
        eng.set_option("score_path", 2)
        for fk, nodiag in variants:
            eng.set_option("fact_kernel", fk)
            eng.set_option("i8o_nodiag", nodiag)
            a = eng.score(pos[:2], wz)
            assert np.max(np.abs(a - ref)) <= (1e-8 if fk >= 10 else 1e-9), (fk, nodiag, w)
        eng.set_option("i8o_nodiag", 0)
    eng.close()


def test_offset_kernel_with_generic_u():
    """A U whose U - U[S] is not two-valued per row (perturbed; T keeps the
    NEM structure) takes the offset kernel that reads U - U[S] per cell
    (i8o 1); a U far from any bound falls back to the max-offset kernel."""
    m = generator.synthetic_nem(40, 333, 5)
    t = m.get_score_tensor()
    rng = np.random.default_rng(8)
    u = m.U + rng.uniform(-0.5, 0.5, m.U.shape)
    eng = Engine(u, t)
    assert eng.factored and eng.get_option("i8o") == 1
    perms = [rng.permutation(40) for _ in range(9)]
    pos = np.array([_pos(p) for p in perms])
    w01 = expit(rng.uniform(-3, 3, (9, 40, 40)))
    ll = eng.score(pos, w01)
    eng.set_option("score_path", 1)
    assert np.max(np.abs(ll - eng.score(pos, w01))) <= 1e-9
    eng.close()
    for c in (0, 4):
        assert abs(ll[c] - no.order_score(u, t, perms[c], w01[c])) <= 1e-9
    far = m.U.copy()
    far[3] -= 2000.0  # exp(U - U[S]) would underflow: no offset kernel
    eng = Engine(far, t)
    assert eng.factored and eng.get_option("i8o") == 0
    ll = eng.score(pos, w01)
    assert abs(ll[0] - no.order_score(far, t, perms[0], w01[0])) <= 1e-9
    eng.close()


def test_int8_kernel_bits_independent_of_split(c3_model):
    """The int8 kernel splits an evaluation over more blocks for small batches
    (and sums its partials in-kernel when one block owns it); ll bits must not
    depend on the batch size."""
    m, eng = c3_model
    try:
        _split_checks(m, eng)
    finally:
        # the module's engine back to its defaults, whatever failed
        eng.set_option("fact_kernel", 0)
        eng.set_option("score_path", 0)
        eng.set_option("exact", 1)


def _split_checks(m, eng):
    s = m.num_s
    rng = np.random.default_rng(21)
    b = 300
    pos = np.array([rng.permutation(s) for _ in range(b)], dtype=np.int32)
    w01 = expit(rng.uniform(-3, 3, (b, s, s)))
    eng.set_option("fact_kernel", 0)
    eng.set_option("exact", 0)   # the fixed-point kernels (the exact path: test_gpu_exact.py)
    big = eng.score(pos, w01)
    for n in (1, 5, 64):
        assert np.array_equal(eng.score(pos[:n], w01[:n]), big[:n])
    # auto is the log2 fixed-point offset kernel walking two effect tiles per
    # iteration (10; 17 is the same walk in persistent blocks): the two tiles'
    # column products are kept by different lanes, so its bits differ in the
    # last places from the one-tile walks -- 4 / 8 waves per block, 16 waves,
    # 6 waves per SIMD (11 / 16 / 12 / 14), which give one another's bits; the
    # natural-scale offset kernel's (7 / 8) and the max-offset kernel's (4 / 6)
    # likewise
    assert eng.get_option("i8o") == 2 and eng.get_option("i8l") == 1
    for fk in (10, 17):
        eng.set_option("fact_kernel", fk)
        assert np.array_equal(eng.score(pos, w01), big)
        assert np.array_equal(eng.score(pos[:7], w01[:7]), big[:7])
    eng.set_option("fact_kernel", 16)
    one = eng.score(pos, w01)
    assert np.max(np.abs(one - big)) <= 1e-9
    for fk in (11, 12, 14):
        eng.set_option("fact_kernel", fk)
        assert np.array_equal(eng.score(pos, w01), one)
        assert np.array_equal(eng.score(pos[:7], w01[:7]), one[:7])
    # the register-stationary kernel: its own bits (per-set sums in another
    # order), independent of the batch too
    eng.set_option("fact_kernel", 13)
    st13 = eng.score(pos, w01)
    assert np.max(np.abs(st13 - big)) <= 1e-8
    for n in (1, 7, 64):
        assert np.array_equal(eng.score(pos[:n], w01[:n]), st13[:n])
    eng.set_option("fact_kernel", 8)
    nat = eng.score(pos, w01)
    assert np.max(np.abs(nat - big)) <= 1e-8
    eng.set_option("fact_kernel", 7)
    assert np.array_equal(eng.score(pos, w01), nat)
    assert np.array_equal(eng.score(pos[:7], w01[:7]), nat[:7])
    eng.set_option("fact_kernel", 4)
    other = eng.score(pos, w01)
    assert np.max(np.abs(other - nat)) <= 1e-9
    eng.set_option("fact_kernel", 6)
    assert np.array_equal(eng.score(pos, w01), other)
    assert np.array_equal(eng.score(pos[:7], w01[:7]), other[:7])
    eng.set_option("fact_kernel", 0)
    eng.set_option("score_path", 1)
    assert np.max(np.abs(eng.score(pos[:8], w01[:8]) - big[:8])) <= 1e-8
    eng.set_option("score_path", 0)
    eng.set_option("exact", 1)
    # the exact arithmetic: batch-independent too, within 1e-6 of the kernels
    ex = eng.score(pos, w01)
    assert np.array_equal(eng.score(pos[:5], w01[:5]), ex[:5])
    assert np.max(np.abs(ex - big)) <= 1e-6


def test_replica_exchange_net2_golden(net2):
    """replica_exchange_method (nem_order_mcmc.py:344-363) on net2: 10
    replicas, 3 rounds of 4 steps, global stream seeded 2024.  The batched
    version (all replicas in one fused call per step) and the sequential
    mirror both reproduce the reference's per-round scores, exchanges, final
    best and random state."""
    from nemo import nem_order_mcmc as mc
    from nemo.replicas import ReplicaExchange
    z = golden("replica_net2.npz")
    m, _ = net2
    order = utils.initial_order_guess(m.observed_knockdown_mat)
    assert np.array_equal(order, z["order0"])
    n_ex, n_it = int(z["n_exchange"]), int(z["n_iter"])
    random.seed(int(z["seed"]))
    rx = ReplicaExchange(m, order)
    for k in range(n_ex):
        best, best_obj, nx = rx.step(n_it, k % 2 == 0)
        assert np.max(np.abs(rx.scores - z["round_scores"][k])) <= LL_TOL
        assert nx == int(z["round_nex"][k])
        assert abs(best - float(z["round_best"][k])) <= LL_TOL
    assert np.array_equal(np.array(random.getstate()[1]), z["rng_state_after"])
    win = rx.objs[best_obj]
    assert np.array_equal(win.best_order, z["best_order"]) and np.array_equal(win.best_dag, z["best_dag"])
    # the sequential mirror of the reference function
    random.seed(int(z["seed"]))
    best2, nem2 = mc.replica_exchange_method(m, n_ex, n_it, order)
    assert abs(best2 - float(z["best_score"])) <= LL_TOL
    assert np.array_equal(nem2.best_order, z["best_order"])
    assert np.array_equal(np.array(random.getstate()[1]), z["rng_state_after"])


def test_replica_exchange_c3_golden():
    """replica_exchange_method at the headline model (C3, 64 x 2000; make_goldens.py
    --only-c3-extra): 10 replicas, 2 exchange rounds of 3 steps, global stream
    seeded 2025.  The batched version and the sequential mirror reproduce the
    reference's per-round scores and exchanges, the final best score, order and
    DAG and the random state -- to the bit (option exact, the default)."""
    from nemo import nem_order_mcmc as mc
    from nemo.replicas import ReplicaExchange
    z = golden("replica_C3.npz")
    m = generator.synthetic_nem(64, 2000, 0)
    order = utils.initial_order_guess(m.observed_knockdown_mat)
    assert np.array_equal(order, z["order0"])
    n_ex, n_it = int(z["n_exchange"]), int(z["n_iter"])
    random.seed(int(z["seed"]))
    rx = ReplicaExchange(m, order)
    for k in range(n_ex):
        best, best_obj, nx = rx.step(n_it, k % 2 == 0)
        assert np.array_equal(rx.scores, z["round_scores"][k]), k
        assert nx == int(z["round_nex"][k])
        assert best == float(z["round_best"][k])
        assert np.array_equal(np.array([np.asarray(rx.objs[r].best_order) for r in rx.obj_at_pos]),
                              z["round_best_orders"][k])
    assert np.array_equal(np.array(random.getstate()[1]), z["rng_state_after"])
    win = rx.objs[best_obj]
    assert np.array_equal(win.best_order, z["best_order"]) and np.array_equal(win.best_dag, z["best_dag"])
    random.seed(int(z["seed"]))
    best2, nem2 = mc.replica_exchange_method(m, n_ex, n_it, order)
    assert best2 == float(z["best_score"])
    assert np.array_equal(nem2.best_order, z["best_order"]) and np.array_equal(nem2.best_dag, z["best_dag"])
    assert np.array_equal(np.array(random.getstate()[1]), z["rng_state_after"])


def test_trajectory_c3_use_nem_20():
    """method(use_nem=True) at the headline model (C3; make_goldens.py
    --only-c3-extra, global stream seeded 77): the transitive-closure DAG of
    eval #2 and the accept step, 20 steps -- identical proposals and accepts,
    every score, the best score, order and (closure) DAG, the final weights
    and the random state, to the bit."""
    from nemo.nem_order_mcmc import NEMOrderMCMC
    z = golden("traj_C3_nem_20.npz")
    assert bool(z["use_nem"])
    m = generator.synthetic_nem(64, 2000, 0)
    random.seed(77)
    smp = NEMOrderMCMC(m, z["order0"])
    best, best_dag = smp.method(n_iterations=int(z["n_iter"]), gamma=float(z["gamma"]),
                                swap_prob=float(z["swap_prob"]), verbose=False, use_nem=True)
    assert np.array_equal(np.array(smp.accepted), z["acc"])
    assert np.array_equal(np.array(smp.all_score_list), z["all_scores"])
    assert best == float(z["best_score"])
    assert np.array_equal(smp.best_order, z["best_order"])
    assert np.array_equal(np.asarray(best_dag), z["best_dag"])
    assert np.array_equal(np.array(random.getstate()[1]), z["rng_state_after"])
    assert np.array_equal(smp.parent_weights, z["final_W"])


def test_integration_stub_binds_the_library(net2):
    """INTEGRATION.md's ctypes stub (the binding a maintainer would add next to
    the reference) drives libnemo.so for a sampler object with the reference's
    attributes and gives the mirror's results."""
    import re

    from nemo import _lib
    from nemo.nem_order_mcmc import NEMOrderMCMC
    text = open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "INTEGRATION.md")).read()
    code = re.search(r"```python\n(# nemo_binding\.py.*?)```", text, re.S).group(1)
    code = code.replace('"/path/to/nem-mcmc-optimization_amd/nemo/libnemo.so"', repr(_lib.lib_path()))
    ns = {}
    exec(compile(code, "nemo_binding.py", "exec"), ns)
    m, _ = net2
    order = utils.initial_order_guess(m.observed_knockdown_mat)
    ref = NEMOrderMCMC(m, order)
    smp = NEMOrderMCMC(m, order, engine=ref.engine)
    scorer = ns["Scorer"](smp)
    want = ref.get_optimal_weights(init=True)
    got = scorer.optimal_weights(smp)
    assert got == want and np.array_equal(smp.parent_weights, ref.parent_weights)  # same kernels, same bits
    assert np.array_equal(smp.ancestor_x, ref.ancestor_x)
    _ow, ll = scorer.order_score(smp)
    assert abs(ll - float(ref.engine.score(ref._pos[None], expit(ref.parent_weights)[None])[0])) <= 1e-9


@pytest.mark.parametrize("s,e,dtype,cap", [(11, 184, "f64", 0), (16, 500, "f64", 0), (64, 2000, "f64", 0),
                                           (128, 700, "f32", 6)])
def test_stage_knockdown_equals_stage_tables(s, e, dtype, cap):
    """Staging from D on the device (nemo_stage_knockdown, nem.py:25-64)
    stages bit for bit what the host tables stage: the same cells and ll on
    every kernel, the same fused optimal-weights step, and U itself (cells of
    an evaluation with all weights 0)."""
    m = generator.synthetic_nem(s, e, 3)
    ref = Engine(m.U, m.get_score_tensor(), dtype=dtype)
    dev = Engine.from_knockdown(m.observed_knockdown_mat, m.A, m.B, dtype=dtype)
    assert dev.factored == ref.factored
    rng = np.random.default_rng(s + e)
    pos = np.array([rng.permutation(s) for _ in range(6)], dtype=np.int32)
    w01 = expit(rng.uniform(-3, 3, (6, s, s)))
    zero = dev.score(pos[:1], np.zeros((1, s, s)), cap=cap, want_cells=True)["cells"][0]
    assert np.array_equal(zero, ref.score(pos[:1], np.zeros((1, s, s)), cap=cap, want_cells=True)["cells"][0])
    if dtype == "f64":
        assert np.array_equal(zero, m.U)
    for path, fks in ((1, (0,)), (2, (0, 1, 2, 4, 6, 7) if s <= 64 else (0, 1))):
        for fk in fks:
            for eng in (ref, dev):
                eng.set_option("score_path", path)
                eng.set_option("fact_kernel", fk)
            a = ref.score(pos, w01, cap=cap, want_cells=True)
            b = dev.score(pos, w01, cap=cap, want_cells=True)
            assert np.array_equal(a["ll"], b["ll"]), (path, fk)
            assert np.array_equal(a["cells"], b["cells"]), (path, fk)
            assert np.array_equal(ref.score(pos, w01, cap=cap), dev.score(pos, w01, cap=cap)), (path, fk)
    for eng in (ref, dev):
        eng.set_option("score_path", 0)
        eng.set_option("fact_kernel", 0)
    from nemo.nem_order_mcmc import SIG0, SIG1
    wr = rng.uniform(-3, 3, (2, s, s))
    anc = np.clip(rng.random((2, s, s)) - 0.5, 0, 1)
    ra = ref.optimal_weights(pos[:2], expit(wr), anc, wr, SIG0, SIG1, cap=cap, raise_on_fail=False)
    rb = dev.optimal_weights(pos[:2], expit(wr), anc, wr, SIG0, SIG1, cap=cap, raise_on_fail=False)
    for x, y in zip(ra, rb):
        assert np.array_equal(x, y)
    ref.close()
    dev.close()


def test_stage_knockdown_rejects_bad_input():
    m = generator.synthetic_nem(4, 10, 0)
    with pytest.raises(ValueError, match="0 and 1"):
        Engine.from_knockdown(m.observed_knockdown_mat * 0.5, m.A, m.B)
    with pytest.raises(RuntimeError, match="finite"):
        Engine.from_knockdown(m.observed_knockdown_mat, float("-inf"), m.B)
    with pytest.raises(RuntimeError, match="product range"):
        Engine.from_knockdown(m.observed_knockdown_mat, m.A, 30.0, dtype="f32")


def test_staging_while_the_gpu_is_busy():
    """Staging from D zero-fills U's padding before the knockdown kernels write
    U, on the context's (non-blocking) stream: a null-stream fill is not
    ordered before them and landed after them when another process shared
    the GPU (garbage scores in the N = 2 rehearsal).  Stage C2 engines while a
    128-chain C3 step runs on another context: every one scores the golden
    bits."""
    from nemo.nem_order_mcmc import SIG0, SIG1
    m3 = generator.config_nem("C3")
    busy = Engine.for_nem(m3)
    rng = np.random.default_rng(5)
    n = 128
    pos3 = np.array([np.argsort(rng.permutation(64)) for _ in range(n)], dtype=np.int32)
    call = busy.bind_optimal_weights_w(pos3, rng.uniform(-3, 3, (n, 64, 64)), SIG0, SIG1, want_prep=False)
    m2 = generator.config_nem("C2")
    perm = rng.permutation(16)
    pos = np.argsort(perm)[None].astype(np.int32)
    w01 = expit(rng.uniform(-3, 3, (1, 16, 16)))
    ref = no.order_score(m2.U, m2.get_score_tensor(), perm, w01[0])
    try:
        for _ in range(3):
            call.ended = False
            call.begin()
            engs = [Engine.from_knockdown(m2.observed_knockdown_mat, m2.A, m2.B) for _ in range(4)]
            call.end()
            for e in engs:
                assert abs(e.score(pos, w01)[0] - ref) <= 1e-9
                e.close()
    finally:
        call.end()
        busy.close()


def test_staging_while_another_engine_captures():
    """Staging takes no process-wide lock (its copies run on the context's own
    stream): stage C2 engines on this thread while a busy C3
    engine's step thread captures a new graph for every call (a new sig0 per
    call misses the graph cache), with the library lock out of the staging
    path.  Every staged engine scores the golden bits, every step returns
    NEMO_OK, and no HIP error is left behind."""
    from nemo.nem_order_mcmc import SIG0, SIG1
    m3 = generator.config_nem("C3")
    busy = Engine.for_nem(m3)
    rng = np.random.default_rng(6)
    n = 8
    pos3 = np.array([np.argsort(rng.permutation(64)) for _ in range(n)], dtype=np.int32)
    w3 = rng.uniform(-3, 3, (n, 64, 64))
    m2 = generator.config_nem("C2")
    perm = rng.permutation(16)
    pos = np.argsort(perm)[None].astype(np.int32)
    w01 = expit(rng.uniform(-3, 3, (1, 16, 16)))
    ref = no.order_score(m2.U, m2.get_score_tensor(), perm, w01[0])
    assert busy.get_option("graphs") == 1
    try:
        for k in range(12):
            call = busy.bind_optimal_weights_w(pos3, w3, SIG0 + 1e-6 * (k + 1), SIG1, want_prep=False)
            call.begin()
            engs = [Engine.from_knockdown(m2.observed_knockdown_mat, m2.A, m2.B) for _ in range(2)]
            call.end()
            assert call.rc in (0, _lib.NEMO_ERR_OPT), _lib.load().nemo_last_error()
            for e in engs:
                assert abs(e.score(pos, w01)[0] - ref) <= 1e-9
                e.close()
        assert busy.get_option("graphs") == 1   # no capture failed (a failure turns graphs off)
    finally:
        busy.close()


def test_order_weights_per_sampler_on_shared_engine():
    """order_weights / calculate_local_optimum read THIS sampler's eval #1
    (nem_order_mcmc.py:181-182, 160-170), also when other samplers share the
    engine and after method()'s opt_weights pass-through scored on it."""
    from nemo.nem_order_mcmc import NEMOrderMCMC
    m = generator.synthetic_nem(16, 500, 0)
    t = m.get_score_tensor()
    eng = Engine.for_nem(m)
    rng = np.random.default_rng(21)
    pa, pb = rng.permutation(16), rng.permutation(16)
    a = NEMOrderMCMC(m, pa, engine=eng)
    b = NEMOrderMCMC(m, pb, engine=eng)
    with pytest.raises(AttributeError):
        a.order_weights
    a.get_optimal_weights(init=True)
    w_a, anc_a = a.parent_weights.copy(), a.ancestor_x.copy()
    ora = no.OracleSampler(m.U, t, pa)
    ora.optimal_weights()
    b.get_optimal_weights(init=True)   # the engine's last fused call is b's
    b.opt_weights()
    assert np.max(np.abs(a.order_weights - ora.ow)) <= 1e-11
    for i, k in ((int(pa[5]), int(pa[2])), (int(pa[15]), int(pa[0]))):
        c = no.local_c(t[i][k], ora.ow[k], w_a[i][k])
        res = no.local_optimum(c, anc_a[i][k], expit(w_a[i][k]))
        got = a.calculate_local_optimum(i, k)
        assert abs(got[0] - expit(res.x[0])) <= 1e-6
    # method() on a shared engine leaves a usable order_weights
    random.seed(5)
    a.method(n_iterations=3, gamma=0.05, verbose=False)
    pos, w01, _ = a._eval1
    ref = no.calculate_ll(no.cell_ratios(m.U, t, no.parents_of(np.argsort(pos)), w01))[0]
    assert np.max(np.abs(a.order_weights - ref)) <= 1e-11


def test_init_false_reoptimises_only_pairs_touching_i1_i2():
    """get_optimal_weights(init=False, i1, i2) (nem_order_mcmc.py:190-194):
    pairs away from i1 / i2 keep their weights; the others get the same
    optimum as a full pass."""
    from nemo.nem_order_mcmc import NEMOrderMCMC
    m = generator.synthetic_nem(16, 500, 0)
    eng = Engine.for_nem(m)
    perm = np.random.default_rng(3).permutation(16)
    full = NEMOrderMCMC(m, perm, engine=eng)
    part = NEMOrderMCMC(m, perm, engine=eng)
    w0 = full.parent_weights.copy()
    full.get_optimal_weights(init=True)
    i1, i2 = int(perm[3]), int(perm[9])
    part.get_optimal_weights(init=False, i1=i1, i2=i2)
    mask = part._mask
    touch = np.zeros_like(mask)
    touch[[i1, i2], :] = True
    touch[:, [i1, i2]] = True
    redo = mask & touch
    assert redo.any() and (mask & ~touch).any()
    assert np.array_equal(part.parent_weights[mask & ~touch], w0[mask & ~touch])
    assert np.array_equal(part.parent_weights[redo], full.parent_weights[redo])


def test_queued_fused_step_equals_direct_call():
    """nemo_optimal_weights_begin / _end (the library's step thread): two
    queued calls give the direct call's outputs and result codes, in order;
    an _end with nothing queued is NEMO_ERR_STATE."""
    from nemo import _lib
    from nemo.nem_order_mcmc import SIG0, SIG1
    m = generator.synthetic_nem(64, 2000, 3)
    eng = Engine.for_nem(m)
    rng = np.random.default_rng(21)
    calls, direct, w_orig = [], [], []
    for n in (3, 5):
        pos = np.array([rng.permutation(64) for _ in range(n)], dtype=np.int32)
        w = rng.uniform(-3, 3, (n, 64, 64))
        w_orig.append(w)
        anc = np.clip(rng.random((n, 64, 64)) - 0.5, 0, 1)
        direct.append(eng.optimal_weights(pos, expit(w), anc, w, SIG0, SIG1, raise_on_fail=False))
        calls.append(eng.bind_optimal_weights(pos, expit(w), anc, w, SIG0, SIG1))
    for c in calls:
        c.begin()
    for c, d in zip(calls, direct):
        c.end()
        assert c.rc in (0, _lib.NEMO_ERR_OPT)
        for x, y in zip(c.result(raise_on_fail=False), d):
            assert np.array_equal(x, y)
    assert _lib.load().nemo_optimal_weights_end(eng._ctx) == _lib.NEMO_ERR_STATE
    # calls still queued when the engine closes run to completion first: their
    # output buffers hold the direct call's results although no _end collects them
    again = []
    for c, w in zip(calls, w_orig):
        pos, w01, anc = c._keep
        a = eng.bind_optimal_weights(pos, w01, anc, w, SIG0, SIG1)
        a.ll1[:] = np.nan
        a.lld[:] = np.nan
        a.begin()
        again.append(a)
    eng.close()
    for a, d in zip(again, direct):
        assert np.array_equal(a.w_new, d[0]) and np.array_equal(a.ll1, d[1]) and np.array_equal(a.lld, d[2])


@pytest.mark.parametrize("n", [1, 3])
def test_split_local_optima_same_bits(n):
    """The fused step's local optima on 4-wave and 2-wave blocks (local_split 2
    and 3) give exactly the one-wave kernel's results."""
    from nemo.nem_order_mcmc import SIG0, SIG1
    m = generator.synthetic_nem(64, 2000, 0)
    eng = Engine.for_nem(m)
    rng = np.random.default_rng(40 + n)
    pos = np.array([rng.permutation(64) for _ in range(n)], dtype=np.int32)
    w = rng.uniform(-3, 3, (n, 64, 64))
    anc = np.clip(rng.random((n, 64, 64)) - 0.5, 0, 1)
    out = {}
    for mode in (1, 2, 3, 0):
        eng.set_option("local_split", mode)
        out[mode] = eng.optimal_weights(pos, expit(w), anc, w, SIG0, SIG1, raise_on_fail=False)
    for mode in (2, 3, 0):
        for x, y in zip(out[mode], out[1]):
            assert np.array_equal(x, y), mode
    eng.set_option("local_split", 0)


def test_fused_step_graph_replay_equals_direct_launches():
    """nemo_optimal_weights replays its device work as a hipGraph per
    (nchains, cap) (option "graphs", default 1): the same outputs as direct
    launches, for several chain counts, a cap, and after an option change
    (which must not replay a stale graph)."""
    from nemo.nem_order_mcmc import SIG0, SIG1
    m = generator.synthetic_nem(64, 2000, 0)
    eng = Engine.for_nem(m)
    rng = np.random.default_rng(77)
    cases = []
    for n, cap in ((1, 0), (3, 0), (2, 5), (1, 0)):
        pos = np.array([rng.permutation(64) for _ in range(n)], dtype=np.int32)
        w = rng.uniform(-3, 3, (n, 64, 64))
        anc = np.clip(rng.random((n, 64, 64)) - 0.5, 0, 1)
        cases.append((pos, w, anc, cap))
    def run_all():
        return [eng.optimal_weights(p, expit(w), a, w, SIG0, SIG1, cap=cap, raise_on_fail=False)
                for p, w, a, cap in cases]
    eng.set_option("graphs", 1)
    g1 = run_all()
    g2 = run_all()            # replays
    assert eng.get_option("graphs") == 1, "the fused step could not be captured"
    eng.set_option("graphs", 0)
    d = run_all()
    for a, b, c in zip(g1, g2, d):
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x, z) and np.array_equal(y, z)
    # an option change between replays takes effect (fp64 eval #2 instead of
    # int8, on the fast kernels: the exact path takes no fact_kernel)
    try:
        eng.set_option("exact", 0)
        d = run_all()                 # graphs 0, int8
        eng.set_option("graphs", 1)
        run_all()
        eng.set_option("fact_kernel", 1)
        f1 = run_all()
        eng.set_option("graphs", 0)
        f0 = run_all()
        for a, c in zip(f1, f0):
            for x, z in zip(a, c):
                assert np.array_equal(x, z)
        assert any(not np.array_equal(a[2], b[2]) for a, b in zip(f0, d))  # ll_dag moved: other kernel
    finally:
        eng.set_option("fact_kernel", 0)
        eng.set_option("exact", 1)
        eng.set_option("graphs", 1)


def test_chain_checkpoint_resume_equals_one_run(tmp_path):
    """ChainBatch.save_checkpoint / from_checkpoint + run(n, resume=True):
    3 + 4 steps with a checkpoint in between give exactly the 7-step run
    (accepts, scores, best orders, every chain's random stream)."""
    from nemo.chains import ChainBatch
    m = generator.synthetic_nem(16, 500, 0)
    orders = [np.random.default_rng(k).permutation(16) for k in range(4)]
    seeds = [21, 22, 23, 24]
    one = ChainBatch(m, orders, seeds, swap_prob=0.9)
    b1, o1 = one.run(7)
    part = ChainBatch(m, orders, seeds, swap_prob=0.9, engine=one.engine)
    part.run(3)
    path = str(tmp_path / "chains.npz")
    part.save_checkpoint(path)
    back = ChainBatch.from_checkpoint(path, m, engine=one.engine)
    b2, o2 = back.run(4, resume=True)
    assert np.array_equal(b1, b2) and np.array_equal(o1, o2)
    assert np.array_equal(back.accepted, one.accepted)
    for c1, c2 in zip(one.chains, back.chains):
        assert c1.rng.getstate() == c2.rng.getstate()
        assert np.array_equal(c1.parent_weights, c2.parent_weights)
        assert c1.all_score_list == c2.all_score_list
    # resuming the in-memory batch is the same as resuming the checkpoint
    b3, _ = part.run(4, resume=True)
    assert np.array_equal(b3, b1)
    with pytest.raises(ValueError, match="resume"):
        ChainBatch(m, orders, seeds, engine=one.engine).run(1, resume=True)


@pytest.mark.parametrize("n,cap", [(1, 0), (3, 0), (2, 5), (600, 0)])
def test_fused_step_host_summed_ll_dag_equals_device_sum(n, cap):
    """The staged fused step (nemo_optimal_weights) copies eval #2's partials
    out with its other outputs and sums them on the host (sum_partials_host,
    nemo_host.h) instead of in a finalize launch; nemo_optimal_weights_dev
    keeps the device's sum.  Same bits: one chain (16 blocks, partials per set),
    a ragged group, a capped call (the lookup-table kernel's per-word
    partials) and a batch past the split (the kernel sums in-kernel)."""
    import ctypes as C
    import torch
    from nemo import _lib
    from nemo.nem_order_mcmc import SIG0, SIG1
    m = generator.synthetic_nem(64, 2000, 0)
    eng = Engine.for_nem(m)
    rng = np.random.default_rng(90 + n)
    pos = np.array([rng.permutation(64) for _ in range(n)], dtype=np.int32)
    w = rng.uniform(-3, 3, (n, 64, 64))
    anc = np.clip(rng.random((n, 64, 64)) - 0.5, 0, 1)
    w_new, ll1, lld, info = eng.optimal_weights(pos, expit(w), anc, w, SIG0, SIG1, cap=cap, raise_on_fail=False)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dp, dw, da = dev(pos), dev(expit(w)), dev(anc)
    dn = torch.zeros((n, 64, 64), dtype=torch.float64, device="cuda")
    d1 = torch.zeros(n, dtype=torch.float64, device="cuda")
    d2 = torch.zeros(n, dtype=torch.float64, device="cuda")
    di = torch.zeros((n, 64, 64), dtype=torch.int32, device="cuda")
    rc = _lib.load().nemo_optimal_weights_dev(eng._ctx, n, C.c_void_p(dp.data_ptr()), C.c_void_p(dw.data_ptr()),
                                             C.c_void_p(da.data_ptr()), SIG0, SIG1, cap, C.c_void_p(dn.data_ptr()),
                                             C.c_void_p(d1.data_ptr()), C.c_void_p(d2.data_ptr()),
                                             C.c_void_p(di.data_ptr()), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(d2.cpu().numpy(), lld)
    assert np.array_equal(d1.cpu().numpy(), ll1)
    eng.close()


@pytest.mark.parametrize("capture", [False, True])
def test_fused_step_dev_first_call_on_a_side_stream(capture):
    """nemo_optimal_weights_dev as the first step call of a fresh engine, on a
    non-null stream: nemo_reserve covers the exact step's buffers (zero-filled
    and finished on the context's stream before it returns), so the call only
    enqueues -- it may even be captured into the caller's graph -- and gives
    the host path's bits (the fills used to race the step)."""
    import ctypes as C
    import torch
    from nemo import _lib
    from nemo.nem_order_mcmc import SIG0, SIG1
    m = generator.synthetic_nem(64, 2000, 0)
    n = 3
    rng = np.random.default_rng(7)
    pos = np.array([rng.permutation(64) for _ in range(n)], dtype=np.int32)
    w = rng.uniform(-3, 3, (n, 64, 64))
    anc = np.clip(rng.random((n, 64, 64)) - 0.5, 0, 1)
    host = Engine.from_knockdown(m.observed_knockdown_mat, m.A, m.B)
    w_new, ll1, lld, info = host.optimal_weights(pos, expit(w), anc, w, SIG0, SIG1, raise_on_fail=False)
    host.close()
    eng = Engine.from_knockdown(m.observed_knockdown_mat, m.A, m.B)
    eng.reserve(n, n)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        dp, dw, da = dev(pos), dev(expit(w)), dev(anc)
        dn = torch.zeros((n, 64, 64), dtype=torch.float64, device="cuda")
        d1 = torch.zeros(n, dtype=torch.float64, device="cuda")
        d2 = torch.zeros(n, dtype=torch.float64, device="cuda")
        di = torch.zeros((n, 64, 64), dtype=torch.int32, device="cuda")
    side.synchronize()
    args = (eng._ctx, n, C.c_void_p(dp.data_ptr()), C.c_void_p(dw.data_ptr()), C.c_void_p(da.data_ptr()),
            SIG0, SIG1, 0, C.c_void_p(dn.data_ptr()), C.c_void_p(d1.data_ptr()), C.c_void_p(d2.data_ptr()),
            C.c_void_p(di.data_ptr()))
    lib = _lib.load()
    if capture:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            rc = lib.nemo_optimal_weights_dev(*args, C.c_void_p(side.cuda_stream))
        assert rc == 0, lib.nemo_last_error()
        g.replay()
    else:
        rc = lib.nemo_optimal_weights_dev(*args, C.c_void_p(side.cuda_stream))
        assert rc == 0, lib.nemo_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(d1.cpu().numpy(), ll1)
    assert np.array_equal(d2.cpu().numpy(), lld)
    mask = info != -1
    assert np.array_equal(di.cpu().numpy(), info)
    assert np.array_equal(dn.cpu().numpy()[mask], w_new[mask])
    eng.close()
