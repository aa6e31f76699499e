"""GPU: the reference's own arithmetic on real-valued (generic) score tables,
option exact_generic (csrc/nemo_exact.hip: exact_cells_generic_kernel, the
stored c rows of a generic table) -- bit for bit, no tolerance, against the
oracle (numpy / scipy) and the reference's recorded steps and trajectories
(tests/golden/make_generic_goldens.py; test_generic_cpu.py pins the oracle to
the same fixtures)."""
import random
import sys
import warnings

import numpy as np
import pytest
from conftest import GOLDEN, golden
from scipy.linalg import inv
from scipy.special import expit

import nemo_oracle as no
from nemo import _lib
from nemo.engine import Engine, ExactArithmeticWarning
from nemo.nem import TableModel

sys.path.insert(0, GOLDEN)
from generic_tables import KINDS, generic_tables, table_sha256  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _engine(u, t, **kw):
    eng = Engine(u, t, exact_generic=True, **kw)
    assert eng.get_option("exact_generic") == 1 and not eng.factored
    return eng


def _oracle_eval(u, t, perm, w01, cap=0):
    cells = no.cell_ratios(u, t, no.parents_of(perm, cap), w01)
    ow, ll, cs = no.calculate_ll(cells)
    return ll, cs, cells, ow


def _inputs(rng, s, b):
    perms = [rng.permutation(s) for _ in range(b)]
    pos = np.array([np.argsort(p) for p in perms], dtype=np.int32)
    return perms, pos, expit(rng.uniform(-4, 4, (b, s, s)))


# (6, 100): one pairwise leaf; (6, 130): past the 128 boundary, a lane tail and
# an 8-element tail; (9, 300): several leaves, a tile tail; (17, 1000): several
# tiles of 256, more parents than one load group; (5, 8192): the largest plan
@pytest.mark.parametrize("s,e,cap", [(6, 100, 0), (6, 130, 0), (9, 300, 0), (9, 300, 3), (17, 1000, 0), (5, 8192, 0)])
@pytest.mark.parametrize("kind", KINDS)
def test_generic_scores_equal_oracle(s, e, cap, kind):
    """ll, cs, the cells and the order weights of a batch of 3."""
    u, t = generic_tables(kind, s, e, 7)
    eng = _engine(u, t)
    assert eng.get_option("exact_ok") == 1 and eng.exact_status(cap) == (True, "")
    perms, pos, w01 = _inputs(np.random.default_rng(100 * s + e), s, 3)
    r = eng.score(pos, w01, cap=cap, want_cs=True, want_cells=True, want_ow=True)
    ll_only = eng.score(pos, w01, cap=cap)
    for b in range(3):
        ll, cs, cells, ow = _oracle_eval(u, t, perms[b], w01[b], cap)
        assert r["ll"][b] == ll and ll_only[b] == ll, b
        assert _bits_equal(r["cs"][b], cs) and _bits_equal(r["cells"][b], cells) and _bits_equal(r["ow"][b], ow), b
    eng.close()


@pytest.mark.parametrize("kind", KINDS)
def test_generic_score_dev_equals_host_path_at_any_batch_position(kind):
    """nemo_score_dev with exact_dev 1: the oracle's bits wherever an
    evaluation sits in the batch."""
    import torch
    s, e = 9, 300
    u, t = generic_tables(kind, s, e, 7)
    eng = _engine(u, t)
    eng.set_option("exact_dev", 1)
    perms, pos, w01 = _inputs(np.random.default_rng(5), s, 3)
    order = [2, 0, 1, 1, 2, 0, 0]
    b = len(order)
    eng.reserve(b)
    dpos, dw = torch.from_numpy(pos[order]).cuda(), torch.from_numpy(w01[order]).cuda()
    dll = torch.zeros(b, dtype=torch.float64, device="cuda")
    dcs = torch.zeros((b, e), dtype=torch.float64, device="cuda")
    dow = torch.zeros((b, s + 1, e), dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().nemo_score_dev(eng._ctx, b, dpos.data_ptr(), dw.data_ptr(), 0, dll.data_ptr(),
                                          dcs.data_ptr(), None, dow.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    ref = [_oracle_eval(u, t, perms[k], w01[k]) for k in range(3)]
    for q, k in enumerate(order):
        assert dll[q].item() == ref[k][0], q
        assert _bits_equal(dcs[q].cpu().numpy(), ref[k][1]) and _bits_equal(dow[q].cpu().numpy(), ref[k][3]), q
    eng.close()


def _host_prep(pos, w, cap=0):
    """W~ and ancestor_x as the sampler's host path makes them."""
    gap = pos[:, None] - pos[None, :]
    mask = (gap > 0) & ((gap <= cap) if cap else True)
    mapped = w.copy()
    mapped[mask] = expit(w[mask])
    eye = np.identity(len(pos))
    return expit(w), np.clip(inv(eye - mapped) - eye, 0, 1)


def _check_step(eng, perm, w, cap, ll1, w_new, dag_ll, ow=None):
    """One fused step from host inputs and from W, with graphs on and off."""
    from nemo.nem_order_mcmc import SIG0, SIG1
    pos = np.argsort(perm).astype(np.int32)
    w01, anc = _host_prep(pos, w, cap)
    try:
        for graphs in (1, 0):
            eng.set_option("graphs", graphs)
            for rep in range(2):   # (graphs 1: captured, then replayed)
                got = eng.optimal_weights(pos[None], w01[None], anc[None], w[None], SIG0, SIG1, cap=cap)
                assert got[1][0] == ll1 and got[2][0] == dag_ll, (graphs, rep)
                assert _bits_equal(got[0][0], w_new), (graphs, rep)
                if ow is not None:
                    assert _bits_equal(eng.order_weights(0), ow), (graphs, rep)
                gw = eng.optimal_weights_w(pos[None], w[None], SIG0, SIG1, cap=cap)
                assert _bits_equal(gw[1][0], anc), (graphs, rep)
                assert gw[3][0] == ll1 and gw[4][0] == dag_ll and _bits_equal(gw[2][0], w_new), (graphs, rep)
            # queued on the library's step thread (_begin / _end), two calls in flight
            for from_w in (False, True):
                calls = [eng.bind_optimal_weights_w(pos[None], w[None], SIG0, SIG1, cap=cap) if from_w else
                         eng.bind_optimal_weights(pos[None], w01[None], anc[None], w[None], SIG0, SIG1, cap=cap)
                         for _ in range(2)]
                for c in calls:
                    c.begin()
                for c in calls:
                    c.end()
                    wn, l1, ld, _info = c.result()
                    assert l1[0] == ll1 and ld[0] == dag_ll and _bits_equal(wn[0], w_new), (graphs, from_w)
    finally:
        eng.set_option("graphs", 1)


@pytest.mark.parametrize("name", ["6x130", "9x300", "12x1000", "9x300_cap3"])
@pytest.mark.parametrize("kind", KINDS)
def test_generic_fused_step_equals_reference_capture(name, kind):
    z = golden(f"generic_step_{name}.npz")
    u, t = generic_tables(kind, int(z["S"]), int(z["E"]), int(z[f"{kind}_seed"]))
    assert table_sha256(u, t) == str(z[f"{kind}_sha256"])
    eng = _engine(u, t)
    _check_step(eng, z[f"{kind}_perm"], z[f"{kind}_W"], int(z["cap"]), float(z[f"{kind}_ll1"]), z[f"{kind}_W_new"],
                float(z[f"{kind}_dag_ll"]), z[f"{kind}_ow"])
    eng.close()


def test_generic_fused_step_equals_oracle_largest_plan():
    """(4, 8192): 64 leaf blocks, 8 slots."""
    s, e = 4, 8192
    u, t = generic_tables("own", s, e, 7)
    rng = np.random.default_rng(8)
    perm = rng.permutation(s)
    pos = np.argsort(perm)
    w = np.where(pos[:, None] > pos[None, :], rng.uniform(-3, 3, (s, s)), 0.0)
    ora = no.OracleSampler(u, t, perm)
    ora.w = w.copy()
    dag_ll = ora.optimal_weights()
    eng = _engine(u, t)
    assert eng.get_option("exact_ok") == 1
    _check_step(eng, perm, w, 0, ora.ll1, ora.w, dag_ll, ora.ow)
    eng.close()


@pytest.mark.parametrize("kind", KINDS)
def test_generic_kernel_forms_give_the_same_bits(kind):
    """exact_form 0 (auto), 1 (latency), 2 (throughput) and 7 (slot: needs the
    recompute rows, so it runs as the throughput form), the work queue and the
    schedule on and off: the step fixture's bits, for one chain and for three."""
    from nemo.nem_order_mcmc import SIG0, SIG1
    z = golden("generic_step_9x300.npz")
    s, e = 9, 300
    u, t = generic_tables(kind, s, e, int(z[f"{kind}_seed"]))
    eng = _engine(u, t)
    perm, w = z[f"{kind}_perm"], z[f"{kind}_W"]
    pos = np.argsort(perm).astype(np.int32)
    w01, anc = _host_prep(pos, w)
    p3, w3, w013, anc3 = (np.repeat(x[None], 3, axis=0) for x in (pos, w, w01, anc))
    try:
        for form in (0, 1, 2, 7):
            for persist, sched in ((1, 1), (1, 0), (0, 0)):
                eng.set_option("exact_form", form)
                eng.set_option("exact_persist", persist)
                eng.set_option("exact_sched", sched)
                for rep in range(2):   # (the schedule reads the previous step's counts)
                    got = eng.optimal_weights(p3, w013, anc3, w3, SIG0, SIG1)
                    for c in range(3):
                        assert got[1][c] == float(z[f"{kind}_ll1"]) and got[2][c] == float(z[f"{kind}_dag_ll"])
                        assert _bits_equal(got[0][c], z[f"{kind}_W_new"]), (form, persist, sched, rep, c)
        eng.set_option("exact_trace", 1)   # the timeline is recorded and changes nothing
        got = eng.optimal_weights(pos[None], w01[None], anc[None], w[None], SIG0, SIG1)
        assert _bits_equal(got[0][0], z[f"{kind}_W_new"])
    finally:
        for name, v in (("exact_form", 0), ("exact_persist", 1), ("exact_sched", 1), ("exact_trace", 0)):
            eng.set_option(name, v)
        eng.close()


def _run_traj(z, kind, **kw):
    from nemo.nem_order_mcmc import NEMOrderMCMC
    u, t = generic_tables(kind, int(z["S"]), int(z["E"]), int(z["table_seed"]))
    assert table_sha256(u, t) == str(z["sha256"])
    m = TableModel.from_log_ratios(u[:-1]) if kind == "shared" else TableModel(u, t)
    assert np.array_equal(m.U, u) and np.array_equal(m.T, t)
    return m, NEMOrderMCMC(m, z["order0"], **kw)


@pytest.mark.parametrize("kind", KINDS)
def test_generic_trajectory_equals_reference(kind):
    """20 steps of method() on a TableModel, strict=True: the reference's
    proposals, accepts, scores, best order, final weights and random state."""
    z = golden(f"generic_traj_9x300_{kind}.npz")
    state = random.getstate()
    try:
        random.seed(int(z["seed"]))
        with warnings.catch_warnings():
            warnings.simplefilter("error", ExactArithmeticWarning)
            m, smp = _run_traj(z, kind, strict=True)
        assert smp.engine is Engine.for_model(m) and smp.engine.get_option("exact_ok") == 1
        best, _ = smp.method(n_iterations=int(z["n_iter"]), gamma=float(z["gamma"]),
                             swap_prob=float(z["swap_prob"]), verbose=False)
        end = np.array(random.getstate()[1])
    finally:
        random.setstate(state)
    assert np.array_equal(np.array(smp.accepted), z["acc"])
    assert np.array_equal(np.array(smp.all_score_list), z["all_scores"])
    assert best == float(z["best_score"]) and np.array_equal(smp.best_order, z["best_order"])
    assert np.array_equal(smp.parent_weights, z["final_W"])
    assert np.array_equal(end, z["rng_state_after"])


def test_generic_chain_batch_equals_single_samplers():
    from nemo.chains import ChainBatch
    from nemo.nem_order_mcmc import NEMOrderMCMC
    u, _t = generic_tables("shared", 9, 300, 11)
    m = TableModel.from_log_ratios(u[:-1])
    order = np.arange(9)
    cb = ChainBatch(m, [order] * 2, seeds=[4, 5], on_fail="continue")
    assert cb.engine is Engine.for_model(m)
    best, _ = cb.run(6)
    for c, seed in enumerate((4, 5)):
        smp = NEMOrderMCMC(m, order, strict=True)
        smp.rng = random.Random(seed)
        b1, _ = smp.method(n_iterations=6, gamma=2.0 * 9 / 300, swap_prob=0.95, verbose=False)
        assert b1 == best[c]
        assert _bits_equal(smp.parent_weights, cb.chains[c].parent_weights)


def test_generic_replica_exchange_equals_reference():
    """The replica driver on a TableModel: the reference's
    replica_exchange_method (10 replicas, 2 rounds of 3 steps) round by round
    -- every replica's score, the exchanges, the best orders, the stream."""
    from nemo.replicas import ReplicaExchange
    z = golden("replica_generic_9x300_shared.npz")
    u, t = generic_tables("shared", 9, 300, 11)
    assert table_sha256(u, t) == str(golden("generic_step_9x300.npz")["shared_sha256"])
    m = TableModel.from_log_ratios(u[:-1])
    state = random.getstate()
    try:
        random.seed(int(z["seed"]))
        rx = ReplicaExchange(m, z["order0"])
        assert rx.engine is Engine.for_model(m) and rx.engine.get_option("exact_ok") == 1
        for k in range(int(z["n_exchange"])):
            best, best_obj, nx = rx.step(int(z["n_iter"]), k % 2 == 0)
            assert np.array_equal(rx.scores, z["round_scores"][k]), k
            assert nx == int(z["round_nex"][k]) and best == float(z["round_best"][k]), k
            assert np.array_equal(np.array([np.asarray(rx.objs[r].best_order) for r in rx.obj_at_pos]),
                                  z["round_best_orders"][k]), k
        assert np.array_equal(np.array(random.getstate()[1]), z["rng_state_after"])
    finally:
        random.setstate(state)
    win = rx.objs[best_obj]
    assert np.array_equal(win.best_order, z["best_order"]) and np.array_equal(win.best_dag, z["best_dag"])


def _wide_tables(amax, s=12, e=100):
    """A generic table past the fp64 product range (|T| <= 170): entries
    uniform in [-amax, amax], one of them amax itself."""
    rng = np.random.default_rng(int(amax))
    t = rng.uniform(-amax, amax, (s, s, e))
    t[3, 7, 11] = amax
    return rng.normal(0, 1, (s + 1, e)), t


@pytest.mark.parametrize("amax", [300.0, 701.0])
def test_wide_table_fast_scores_equal_oracle(amax):
    """|T| past 170 (staged only with the option): the fast score path --
    exact 0, or a table outside the exact bounds -- against the oracle, on
    children with up to 11 parents (four factors of e^300 overflow a product
    that is not renormalised per factor).  Tolerance from the fp64 format:
    both sides round a cell of magnitude M = max|cell| a few times (the
    renormalised exponent's k ln 2, the sums with log(prod) and U; the
    product chain's 2 ulp per factor are relative errors of prod, so absolute
    errors ~1e-15 of its log) -- 32 ulp(M) per cell and per cs; ll sums E such
    cs and rounds E times at its own magnitude."""
    s, e = 12, 100
    u, t = _wide_tables(amax)
    eng = _engine(u, t)
    from nemo import limits
    covered = amax <= limits.MAX_ABS_T_EXACT_GENERIC
    assert eng.get_option("exact_ok") == (1 if covered else 0)
    rng = np.random.default_rng(2)
    perms = [np.arange(s), np.arange(s)[::-1].copy(), rng.permutation(s)]
    pos = np.array([np.argsort(p) for p in perms], dtype=np.int32)
    w01 = expit(rng.uniform(-4, 4, (3, s, s)))
    ref = [_oracle_eval(u, t, perms[b], w01[b]) for b in range(3)]
    assert all(np.isfinite(r[2]).all() for r in ref)
    if covered:   # the exact kernels on the wide table: the oracle's bits
        r = eng.score(pos, w01, want_cs=True, want_cells=True)
        for b in range(3):
            assert r["ll"][b] == ref[b][0] and _bits_equal(r["cs"][b], ref[b][1]) and _bits_equal(r["cells"][b], ref[b][2])
        eng.set_option("exact", 0)
    r = eng.score(pos, w01, want_cs=True, want_cells=True)
    eps = np.finfo(np.float64).eps
    for b in range(3):
        ll, cs, cells, _ow = ref[b]
        big = np.abs(cells).max()
        assert big > 1000.0   # products far past e^709 were formed
        assert np.isfinite(r["cells"][b]).all()
        assert np.max(np.abs(r["cells"][b] - cells)) <= 32 * eps * big, b
        assert np.max(np.abs(r["cs"][b] - cs)) <= 32 * eps * big, b
        assert abs(r["ll"][b] - ll) <= e * 32 * eps * big + e * eps * abs(ll), b
    eng.close()


def test_wide_table_other_fast_kernels_refuse():
    """The fast kernels whose products are not renormalised per factor return
    NEMO_ERR_ARG on a wide table instead of overflowing; the exact step runs."""
    from nemo.nem_order_mcmc import SIG0, SIG1
    s = 12
    u, t = _wide_tables(300.0)
    eng = _engine(u, t)
    rng = np.random.default_rng(4)
    pos = np.argsort(rng.permutation(s)).astype(np.int32)[None]
    w = np.where(pos[0][:, None] > pos[0][None, :], rng.uniform(-3, 3, (s, s)), 0.0)[None]
    w01, anc = _host_prep(pos[0], w[0])
    got = eng.optimal_weights(pos, w01[None], anc[None], w, SIG0, SIG1, raise_on_fail=False)
    assert got[1][0] == _oracle_eval(u, t, np.argsort(pos[0]), w01)[0]   # eval #1's ll, the exact kernels
    eng.set_option("exact", 0)
    for call in (lambda: eng.optimal_weights(pos, w01[None], anc[None], w, SIG0, SIG1, raise_on_fail=False),
                 lambda: eng.gamma_sweep(pos, w01[None], raise_on_fail=False),
                 lambda: eng.inverse_sweep(pos, w, raise_on_fail=False)):
        with pytest.raises(_lib.NemoError, match="product range") as ei:
            call()
        assert ei.value.code == _lib.NEMO_ERR_ARG
    assert np.isfinite(eng.score(pos, w01[None])).all()   # the score calls still run
    eng.close()
    with pytest.raises(_lib.NemoError, match="product range"):   # without the option: refused at staging, as before
        Engine(u, t)
    with pytest.raises(_lib.NemoError, match="product range"):   # past 705 with it too
        Engine(u, _wide_tables(706.0)[1], exact_generic=True)


def _warns_uncovered(eng, u, t):
    from nemo.nem_order_mcmc import NEMOrderMCMC
    assert eng.get_option("exact_generic") == 1 and eng.get_option("exact_ok") == 0
    ok, why = eng.exact_status()
    assert not ok and why.startswith("table form")
    m = TableModel(u, t)
    with pytest.warns(ExactArithmeticWarning, match="table form"):
        NEMOrderMCMC(m, np.arange(m.num_s), engine=eng)
    with pytest.raises(RuntimeError, match="table form"):
        NEMOrderMCMC(m, np.arange(m.num_s), engine=eng, strict=True)


def test_generic_gates():
    """Outside the option's bounds exact_ok stays 0 and the sampler says so;
    the option is set before staging; a factorable table is unaffected."""
    rng = np.random.default_rng(3)
    u, t = rng.normal(0, 1, (4, 8193)), rng.normal(0, 1, (3, 3, 8193))
    eng = _engine(u, t)                     # E = 8193: a second numpy buffer
    _warns_uncovered(eng, u, t)
    eng.close()
    u, t = generic_tables("own", 4, 100, 7)
    t = t.copy()
    from nemo import limits
    tmax = limits.MAX_ABS_T_EXACT_GENERIC
    assert tmax == 670.0
    for v in (701.0, 700.0, -700.0, 671.0, np.nextafter(tmax, np.inf)):
        t[1, 2, 5] = v                      # max|T| past the bound: a flushed order weight could change c
        eng = _engine(u, t)
        _warns_uncovered(eng, u, t)
        eng.close()
    t[1, 2, 5] = -tmax
    eng = _engine(u, t)
    assert eng.get_option("exact_ok") == 1
    eng.close()
    t[1, 2, 5] = tmax                       # ... and 670 is covered
    eng = _engine(u, t)
    assert eng.get_option("exact_ok") == 1 and eng.exact_status() == (True, "")
    with pytest.raises(_lib.NemoError) as ei:   # staged: the option is fixed
        eng.set_option("exact_generic", 0)
    assert ei.value.code == _lib.NEMO_ERR_STATE
    eng.close()
    plain = Engine(u, generic_tables("own", 4, 100, 7)[1])   # without the option: today's behaviour
    assert plain.get_option("exact_generic") == 0 and plain.get_option("exact_ok") == 0
    with pytest.raises(_lib.NemoError):
        plain.set_option("exact_generic", 1)
    plain.close()


def test_factorable_table_takes_the_factored_kernels_whatever_the_option():
    from nemo import generator
    from nemo.nem_order_mcmc import SIG0, SIG1
    m = generator.synthetic_nem(9, 300, 1)
    t = m.get_score_tensor()
    a, b = Engine(m.U, t, exact_generic=True), Engine(m.U, t)
    assert a.factored and b.factored and a.get_option("exact_ok") == 1
    perms, pos, w01 = _inputs(np.random.default_rng(6), 9, 2)
    ra = a.score(pos, w01, want_cs=True, want_ow=True)
    rb = b.score(pos, w01, want_cs=True, want_ow=True)
    assert all(_bits_equal(ra[k], rb[k]) for k in ("ll", "cs", "ow"))
    w = np.random.default_rng(7).uniform(-3, 3, (2, 9, 9))
    anc = np.stack([_host_prep(pos[k], w[k])[1] for k in range(2)])
    sa = a.optimal_weights(pos, expit(w), anc, w, SIG0, SIG1, raise_on_fail=False)
    sb = b.optimal_weights(pos, expit(w), anc, w, SIG0, SIG1, raise_on_fail=False)
    assert all(_bits_equal(x, y) for x, y in zip(sa[:3], sb[:3])) and np.array_equal(sa[3], sb[3])
    a.close()
    b.close()
