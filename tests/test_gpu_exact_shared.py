"""GPU: the reference's own arithmetic on row-shared real-valued tables --
per-effect log ratios, T[i][j] = R[j] for every child (option exact_generic;
csrc/nemo_exact.hip: X kept as [S][E], per-parent recompute rows with lv - 1 a
real number per element, plans of several parts past E = 8192) -- bit for bit,
no tolerance, against the oracle (numpy / scipy) and the reference's recorded
steps and trajectory (tests/golden/make_shared_goldens.py,
make_generic_goldens.py; test_shared_cpu.py and test_generic_cpu.py pin the
oracle to the same fixtures)."""
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
from generic_tables import generic_tables, step_inputs, table_sha256  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _oracle_eval(u, t, perm, w01, cap=0):
    cells = no.cell_ratios(u, t, no.parents_of(perm, cap), w01)
    ow, ll, cs = no.calculate_ll(cells)
    return ll, cs, cells, ow


def _inputs(rng, s, b):
    perms = [rng.permutation(s) for _ in range(b)]
    pos = np.array([np.argsort(p) for p in perms], dtype=np.int32)
    return perms, pos, expit(rng.uniform(-4, 4, (b, s, s)))


def _host_prep(pos, w, cap=0):
    """W~ and ancestor_x as the sampler's host path makes them."""
    gap = pos[:, None] - pos[None, :]
    mask = (gap > 0) & ((gap <= cap) if cap else True)
    mapped = w.copy()
    mapped[mask] = expit(w[mask])
    eye = np.identity(len(pos))
    return expit(w), np.clip(inv(eye - mapped) - eye, 0, 1)


def _check_step(eng, perm, w, cap, ll1, w_new, dag_ll, ow=None):
    """One fused step from host inputs and from W, with graphs on and off, and
    queued on the library's step thread."""
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
            for from_w in (False, True):   # two calls in flight
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


# (6, 130): a lane tail and an 8-element tail; (9, 300) with the last 3
# parents; (5, 8192): the largest single plan; (3, 8193): a second part of one
# term; (4, 8200): a second part of 8; (3, 16500): three parts
@pytest.mark.parametrize("s,e,cap", [(6, 130, 0), (9, 300, 3), (5, 8192, 0), (3, 8193, 0), (4, 8200, 0),
                                     (3, 16500, 0)])
def test_shared_scores_equal_oracle(s, e, cap):
    """ll, cs, the cells and the order weights of a batch of 3."""
    u, t = generic_tables("shared", s, e, 7)
    eng = Engine(u, t, exact_generic=True)
    assert not eng.factored and eng.get_option("exact_shared") == 1
    assert eng.get_option("exact_ok") == 1 and eng.exact_status(cap) == (True, "")
    perms, pos, w01 = _inputs(np.random.default_rng(100 * s + e), s, 3)
    r = eng.score(pos, w01, cap=cap, want_cs=True, want_cells=True, want_ow=True)
    ll_only = eng.score(pos, w01, cap=cap)
    for b in range(3):
        ll, cs, cells, ow = _oracle_eval(u, t, perms[b], w01[b], cap)
        assert r["ll"][b] == ll and ll_only[b] == ll, b
        assert _bits_equal(r["cs"][b], cs) and _bits_equal(r["cells"][b], cells) and _bits_equal(r["ow"][b], ow), b
    eng.close()


@pytest.mark.parametrize("name", ["4x9000", "3x16500", "4x8200"])
def test_shared_fused_step_equals_reference(name):
    """The reference's recorded steps over two and three plan parts, and
    (4, 8200) -- a second part of 8 terms -- against the oracle; staged from R
    alone."""
    s, e = (int(v) for v in name.split("x"))
    z = golden(f"shared_step_{name}.npz") if name != "4x8200" else None
    seed = int(z["seed"]) if z is not None else 11
    u, t = generic_tables("shared", s, e, seed)
    perm, w = step_inputs(s, seed)
    ora = no.OracleSampler(u, t, perm)
    ora.w = w.copy()
    dag_ll = ora.optimal_weights()
    ll1, w_new = ora.ll1, ora.w
    if z is not None:   # the reference's own record
        assert table_sha256(u, t) == str(z["sha256"])
        assert np.array_equal(z["perm"], perm) and np.array_equal(z["W"], w)
        ll1, w_new, dag_ll = float(z["ll1"]), z["W_new"], float(z["dag_ll"])
    eng = Engine.from_log_ratios(u[:-1])
    assert eng.get_option("exact_shared") == 1 and eng.get_option("exact_ok") == 1
    assert eng.exact_status() == (True, "") and eng.get_option("exact_rc") == 1
    _check_step(eng, perm, w, 0, ll1, w_new, dag_ll, ora.ow)
    assert eng.get_option("exact_form_used") == 6   # the throughput form over the plan's parts
    if z is not None:
        pos = np.argsort(perm).astype(np.int32)
        assert _bits_equal(eng.score(pos[None], expit(w)[None], want_cs=True)["cs"][0], z["cs"])
    eng.close()


@pytest.mark.parametrize("chains", [1, 3])
@pytest.mark.parametrize("cform", [1, 0])
def test_shared_kernel_forms_give_the_same_bits(cform, chains):
    """exact_form 0 (auto), 1 (latency), 2 (throughput), 4 (cached throughput)
    and 7 (slot), the work queue and the schedule on and off, on recompute rows
    (exact_cform 1) and on stored rows (0): the step fixture's bits, and the
    form that ran."""
    from nemo.nem_order_mcmc import SIG0, SIG1
    z = golden("generic_step_9x300.npz")
    s, e = 9, 300
    u, t = generic_tables("shared", s, e, int(z["shared_seed"]))
    eng = Engine.from_log_ratios(u[:-1])
    perm, w = z["shared_perm"], z["shared_W"]
    pos = np.argsort(perm).astype(np.int32)
    w01, anc = _host_prep(pos, w)
    pn, wn, w01n, ancn = (np.repeat(x[None], chains, axis=0) for x in (pos, w, w01, anc))

    def step(tag):
        got = eng.optimal_weights(pn, w01n, ancn, wn, SIG0, SIG1)
        for c in range(chains):
            assert got[1][c] == float(z["shared_ll1"]) and got[2][c] == float(z["shared_dag_ll"]), (tag, c)
            assert _bits_equal(got[0][c], z["shared_W_new"]), (tag, c)

    try:
        assert eng.get_option("exact_form_used") == 0   # nothing launched yet
        eng.set_option("exact_cform", cform)
        assert eng.get_option("exact_rc") == cform
        for form in (0, 1, 2, 4, 7):
            for persist, sched in ((1, 1), (1, 0), (0, 0)):
                eng.set_option("exact_form", form)
                eng.set_option("exact_persist", persist)
                eng.set_option("exact_sched", sched)
                for rep in range(2):   # (the schedule reads the previous step's counts)
                    step((form, persist, sched, rep))
                # auto: the latency form at these few optima; the slot form
                # needs the recompute rows and the work queue, else it runs as
                # the throughput form
                want = {0: 1, 7: 7 if cform and persist else 2}.get(form, form)
                assert eng.get_option("exact_form_used") == want, (form, persist, sched)
                assert eng.get_option("exact_rc") == cform
        eng.set_option("exact_persist", 1)
        # the pair and dual forms have no real-valued recompute instance: both
        # run as the throughput form; on stored rows the pair form needs two
        # slots (E > 1024) and the dual form the recompute rows (then: latency)
        for form, want in ((3, 2), (5, 2 if cform else 1)):
            eng.set_option("exact_form", form)
            step((form,))
            assert eng.get_option("exact_form_used") == want, form
    finally:
        eng.close()


@pytest.mark.parametrize("s,e,dtype", [(9, 300, "f64"), (9, 300, "f32"), (6, 130, "f64")])
def test_staging_from_log_ratios_equals_staging_from_tables(s, e, dtype):
    """Engine.from_log_ratios(R) against Engine(U, T, exact_generic=True) with
    the broadcast T: the exact scores, the fast scores (option exact 0) and
    the fused step, bit for bit."""
    from nemo.nem_order_mcmc import SIG0, SIG1
    u, t = generic_tables("shared", s, e, 7)
    a, b = Engine.from_log_ratios(u[:-1], dtype=dtype), Engine(u, t, dtype=dtype, exact_generic=True)
    c = Engine.from_log_ratios(u[:-1], U=u, dtype=dtype)   # U given
    try:
        for eng in (a, b, c):
            assert eng.get_option("exact_shared") == 1 and eng.get_option("exact_ok") == 1 and not eng.factored
        _perms, pos, w01 = _inputs(np.random.default_rng(9), s, 3)
        w = np.random.default_rng(10).uniform(-3, 3, (2, s, s))
        anc = np.stack([_host_prep(pos[k], w[k])[1] for k in range(2)])
        for exact in (1, 0):
            res = []
            for eng in (a, b, c):
                eng.set_option("exact", exact)
                r = eng.score(pos, w01, want_cs=True, want_cells=True, want_ow=True)
                st = eng.optimal_weights(pos[:2], expit(w), anc, w, SIG0, SIG1, raise_on_fail=False)
                res.append((r, st))
            for r, st in res[1:]:
                assert all(_bits_equal(r[k], res[0][0][k]) for k in ("ll", "cs", "cells", "ow")), exact
                assert all(_bits_equal(x, y) for x, y in zip(st[:3], res[0][1][:3])), exact
                assert np.array_equal(st[3], res[0][1][3]), exact
    finally:
        for eng in (a, b, c):
            eng.close()


def test_two_valued_log_ratios_take_the_factored_kernels():
    from nemo import generator
    from nemo.nem_order_mcmc import SIG0, SIG1
    m = generator.synthetic_nem(9, 300, 1)
    t = m.get_score_tensor()
    r = t[1, 0][None].repeat(9, axis=0)
    for j in range(9):
        r[j] = t[(j + 1) % 9, j]   # parent j's (two-valued) off-diagonal row
    tb = np.broadcast_to(r[None], (9, 9, 300)).copy()
    a, b = Engine.from_log_ratios(r, U=m.U), Engine(m.U, tb)
    try:
        assert a.factored and b.factored and a.get_option("exact_ok") == 1 and a.get_option("exact_shared") == 0
        _perms, pos, w01 = _inputs(np.random.default_rng(6), 9, 2)
        for exact in (1, 0):
            a.set_option("exact", exact)
            b.set_option("exact", exact)
            ra = a.score(pos, w01, want_cs=True, want_ow=True)
            rb = b.score(pos, w01, want_cs=True, want_ow=True)
            assert all(_bits_equal(ra[k], rb[k]) for k in ("ll", "cs", "ow")), exact
        w = np.random.default_rng(7).uniform(-3, 3, (2, 9, 9))
        anc = np.stack([_host_prep(pos[k], w[k])[1] for k in range(2)])
        sa = a.optimal_weights(pos, expit(w), anc, w, SIG0, SIG1, raise_on_fail=False)
        sb = b.optimal_weights(pos, expit(w), anc, w, SIG0, SIG1, raise_on_fail=False)
        assert all(_bits_equal(x, y) for x, y in zip(sa[:3], sb[:3])) and np.array_equal(sa[3], sb[3])
    finally:
        a.close()
        b.close()


def test_tables_outside_the_new_bounds_stay_uncovered():
    rng = np.random.default_rng(3)
    u, t = rng.normal(0, 1, (4, 9000)), rng.normal(0, 1, (3, 3, 9000))
    eng = Engine(u, t, exact_generic=True)   # its own rows per child: one numpy buffer only
    assert eng.get_option("exact_shared") == 0 and eng.get_option("exact_ok") == 0
    ok, why = eng.exact_status()
    assert not ok and why.startswith("table form") and "8192" in why
    eng.close()
    u, t = generic_tables("shared", 4, 9000, 7)
    r = u[:-1].copy()
    r[2, 5] = 701.0
    eng = Engine.from_log_ratios(r)          # max|R| = 701
    assert eng.get_option("exact_shared") == 1 and eng.get_option("exact_ok") == 0
    ok, why = eng.exact_status()
    assert not ok and why.startswith("table form") and "700" in why and "670" in why
    eng.close()
    from nemo import limits
    for v in (700.0, 671.0):                 # past max|T| <= 670: a flushed order weight could change c
        r[2, 5] = v
        eng = Engine.from_log_ratios(r)
        assert eng.get_option("exact_shared") == 1 and eng.get_option("exact_ok") == 0
        assert not eng.exact_status()[0]
        eng.close()
    r[2, 5] = limits.MAX_ABS_T_EXACT_GENERIC  # ... and 670 is covered
    eng = Engine.from_log_ratios(r)
    assert eng.get_option("exact_ok") == 1 and eng.exact_status() == (True, "")
    eng.close()
    eng = Engine.from_log_ratios(u[:-1], exact_generic=False)   # without the option: the fast kernels, as before
    assert eng.get_option("exact_shared") == 0 and eng.get_option("exact_ok") == 0
    eng.close()


def test_shared_trajectory_equals_reference():
    """20 steps of method() on TableModel.from_log_ratios at E = 9000,
    strict=True: the reference's accepts, scores, best order, final weights
    and random state -- and the S*S*E tables are never built."""
    from nemo.nem_order_mcmc import NEMOrderMCMC
    z = golden("shared_traj_5x9000.npz")
    u, t = generic_tables("shared", int(z["S"]), int(z["E"]), int(z["table_seed"]))
    assert table_sha256(u, t) == str(z["sha256"])
    m = TableModel.from_log_ratios(u[:-1])
    state = random.getstate()
    try:
        random.seed(int(z["seed"]))
        with warnings.catch_warnings():
            warnings.simplefilter("error", ExactArithmeticWarning)
            smp = NEMOrderMCMC(m, z["order0"], strict=True)
        assert smp.engine is Engine.for_model(m) and smp.engine.get_option("exact_ok") == 1
        assert smp.engine.get_option("exact_shared") == 1
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
    assert m.tables_built is False


def test_shared_chain_batch_equals_single_samplers():
    from nemo.chains import ChainBatch
    from nemo.nem_order_mcmc import NEMOrderMCMC
    z = golden("shared_traj_5x9000.npz")
    s, e = int(z["S"]), int(z["E"])
    u, _t = generic_tables("shared", s, e, int(z["table_seed"]))
    m = TableModel.from_log_ratios(u[:-1])
    order = np.arange(s)
    cb = ChainBatch(m, [order] * 2, seeds=[4, 5], on_fail="continue")
    assert cb.engine is Engine.for_model(m) and cb.engine.get_option("exact_ok") == 1
    best, _ = cb.run(6)
    for c, seed in enumerate((4, 5)):
        smp = NEMOrderMCMC(m, order, strict=True)
        smp.rng = random.Random(seed)
        b1, _ = smp.method(n_iterations=6, gamma=2.0 * s / e, swap_prob=0.95, verbose=False)
        assert b1 == best[c]
        assert _bits_equal(smp.parent_weights, cb.chains[c].parent_weights)
    assert m.tables_built is False
