"""GPU: the exact (reference-arithmetic) kernels of csrc/nemo_exact.hip at the
edge shapes of tests/exact_edge_inputs.py, in the multi-row cells branch that
batches of 512 and more take, across the error-rate ladder and at the bound of
option exact_generic -- bit for bit, no tolerance, against the oracle (numpy /
scipy on the host).  tests/test_exact_edges_cpu.py runs the host restatement
of the same arithmetic on the same inputs.

The one documented exception (include/nemo.h, option "exact"): an order weight
whose argument cell - cs lies below the restated np.exp's fast path (-707.70)
is exactly 0.0, where numpy's rare path gives at most 4.7e-308
(exact_edge_inputs.ow_mismatch)."""
import warnings

import numpy as np
import pytest
from scipy.special import expit

import exact_edge_inputs as xe
import fixed_point_models as fpm
from nemo import _lib, limits
from nemo.engine import Engine, ExactArithmeticWarning
from nemo.nem import TableModel
from nemo.nem_order_mcmc import SIG0, SIG1, NEMOrderMCMC

pytestmark = pytest.mark.gpu

FORMS = (1, 2, 3, 4, 5, 7)


def _engine(nem):
    """A new engine staged from the model's knockdown matrix (not the cached
    one of Engine.for_nem: the test closes it)."""
    eng = Engine.from_knockdown(nem.observed_knockdown_mat, nem.A, nem.B)
    assert eng.factored and eng.get_option("exact") == 1
    return eng


def _covered(eng, nem):
    """True on a model the exact kernels cover.  E = 8191 is not: numpy's
    pairwise recursion of 8191 terms has 65 leaf blocks, one more than the wave
    plan holds (nemo.limits, 441 buffer sizes in 7689 .. 8191) -- there the
    staging must say so (exact_ok 0, exact_status names the E row, the sampler
    warns or, strict, raises) and the caller has nothing to compare."""
    want = xe.exact_covered(eng.E)
    assert eng.get_option("exact_ok") == (1 if want else 0)
    ok, why = eng.exact_status()
    assert ok == want
    if not want:
        assert why.startswith("E (effects)") and "65" in why
        with pytest.warns(ExactArithmeticWarning, match="E \\(effects\\)"):
            NEMOrderMCMC(nem, np.arange(eng.S), engine=eng)
        with pytest.raises(RuntimeError, match="E \\(effects\\)"):
            NEMOrderMCMC(nem, np.arange(eng.S), engine=eng, strict=True)
    return want


def _score_dev(eng, pos, w01, cap, want):
    """nemo_score_dev on device buffers (option exact_dev set by the caller);
    want: "ll", "cs_ow" or "cells".  -> (ll, cs, cells, ow)."""
    import torch
    b, s, e = pos.shape[0], eng.S, eng.E
    eng.reserve(b)
    dpos = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.int32)).cuda()
    dw = torch.from_numpy(np.ascontiguousarray(w01, dtype=np.float64)).cuda()
    dll = torch.zeros(b, dtype=torch.float64, device="cuda")
    dcs = torch.zeros((b, e), dtype=torch.float64, device="cuda") if want == "cs_ow" else None
    dow = torch.zeros((b, s + 1, e), dtype=torch.float64, device="cuda") if want == "cs_ow" else None
    dcells = torch.zeros((b, s + 1, e), dtype=torch.float64, device="cuda") if want == "cells" else None
    _lib.check(_lib.load().nemo_score_dev(eng._ctx, b, dpos.data_ptr(), dw.data_ptr(), int(cap), dll.data_ptr(),
                                          None if dcs is None else dcs.data_ptr(),
                                          None if dcells is None else dcells.data_ptr(),
                                          None if dow is None else dow.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return (dll.cpu().numpy(), None if dcs is None else dcs.cpu().numpy(),
            None if dcells is None else dcells.cpu().numpy(), None if dow is None else dow.cpu().numpy())


def _check_eval(tag, ref, ll=None, cs=None, cells=None, ow=None):
    rll, rcs, rcells, row = ref
    if ll is not None:
        assert ll == rll, (tag, "ll", ll, rll)
    if cs is not None:
        assert xe.bits_equal(cs, rcs), (tag, "cs")
    if cells is not None:
        assert xe.bits_equal(cells, rcells), (tag, "cells")
    if ow is not None:
        assert xe.ow_mismatch(ow, rcells, rcs, row) == "", (tag, "ow")


def test_one_s_gene_is_refused():
    """nemo_ctx_create takes num_s in [2, 256]: S = 1 is NEMO_ERR_ARG (a
    RuntimeError from the engine), so the edge shapes start at S = 2."""
    m, _u, _t = xe.model(1, 65)
    with pytest.raises(RuntimeError, match="num_s=1") as ei:
        Engine.from_knockdown(m.observed_knockdown_mat, m.A, m.B)
    assert ei.value.code == _lib.NEMO_ERR_ARG
    with pytest.raises(RuntimeError, match="num_s=1"):
        Engine(np.zeros((2, 65)), np.zeros((1, 1, 65)))


# --------------------------------------------------------------------------
# 1. scores at every edge shape
# --------------------------------------------------------------------------
@pytest.mark.parametrize("se", xe.shapes(), ids=xe.shape_id)
def test_scores_equal_oracle_at_edge_shapes(se):
    """ll, cs, the cells and the order weights of batches of 7, 5 and 1
    evaluations (every order kind against every weight kind: U(-3, 3), U(-40,
    40), expit exactly 1.0 and 0.0), through the host-pointer score and
    through nemo_score_dev with option exact_dev (ll alone; cs and order
    weights; cells), with parent caps 0, 1, 3 and S - 2 on the batch of 7."""
    s, e = se
    m, u, t = xe.model(s, e)
    perms, pos, ws, _kinds = xe.evals(s, e)
    w01 = expit(ws)
    eng = _engine(m)
    try:
        if not _covered(eng, m):    # (E = 8191: no wave plan; the engine says so)
            return
        eng.set_option("exact_dev", 1)
        batches = [list(range(0, 7)), list(range(7, 12)), [12]]
        for cap in xe.caps(s):
            for idx in (batches if cap == 0 else batches[:1]):
                ref = [xe.oracle_eval(u, t, perms[k], w01[k], cap) for k in idx]
                r = eng.score(pos[idx], w01[idx], cap=cap, want_cs=True, want_cells=True, want_ow=True)
                ll_only = eng.score(pos[idx], w01[idx], cap=cap)
                d_ll = _score_dev(eng, pos[idx], w01[idx], cap, "ll")
                d_ow = _score_dev(eng, pos[idx], w01[idx], cap, "cs_ow")
                d_cells = _score_dev(eng, pos[idx], w01[idx], cap, "cells")
                for q, k in enumerate(idx):
                    tag = (cap, len(idx), k)
                    _check_eval(tag + ("host",), ref[q], r["ll"][q], r["cs"][q], r["cells"][q], r["ow"][q])
                    _check_eval(tag + ("host ll",), ref[q], ll_only[q])
                    _check_eval(tag + ("dev ll",), ref[q], d_ll[0][q])
                    _check_eval(tag + ("dev cs ow",), ref[q], d_ow[0][q], d_ow[1][q], None, d_ow[3][q])
                    _check_eval(tag + ("dev cells",), ref[q], d_cells[0][q], None, d_cells[2][q])
        # a one-evaluation call gives the batch's bits
        ref = xe.oracle_eval(u, t, perms[3], w01[3], 0)
        r = eng.score(pos[3:4], w01[3:4], want_cs=True, want_cells=True, want_ow=True)
        _check_eval("single host", ref, r["ll"][0], r["cs"][0], r["cells"][0], r["ow"][0])
        d = _score_dev(eng, pos[3:4], w01[3:4], 0, "cs_ow")
        _check_eval("single dev", ref, d[0][0], d[1][0], None, d[3][0])
    finally:
        eng.close()


# --------------------------------------------------------------------------
# 2. batches of 512 and more: the multi-row cells branch
# --------------------------------------------------------------------------
def _big_inputs(s, e, n):
    rng = np.random.default_rng(77 * s + e)
    perms, ws = [], []
    for k in range(n):
        perms.append(xe.order(xe.ORDER_KINDS[k % 3] if k < 6 else "random", s, rng))
        ws.append(xe.raw_weights(xe.WEIGHT_KINDS[k % 4] if k % 16 < 4 else "u3", s, rng))
    return perms, np.stack([xe.pos_of(p) for p in perms]), expit(np.stack(ws))


@pytest.mark.parametrize("cap", [0, 3])
@pytest.mark.parametrize("s,e", [(3, 65), (12, 257), (64, 130), (65, 130), (100, 65), (128, 130)])
def test_batches_from_512_take_the_multi_row_branch_with_the_same_bits(s, e, cap):
    """launch_exact_eval gives exact_cells_kernel rows = min(8, 512 / S)
    children per block once batch >= 512: ragged last chunks (S = 12: 8 + 5
    rows; S = 65: rows 7, last chunk 3; S = 100: rows 5, last chunk 1), a last
    chunk that is row S alone (S = 64, 128), one block with nr = 4 < rows (S =
    3), with and without a parent cap.  Calls of 512 and of 515 evaluations
    give the ll, cs, cells and order weights of the same evaluations issued in
    calls of 64 (one child per block), bit for bit, and evaluations 0, 255,
    511 and 514 are the oracle's; the host-pointer score at batch 512 too.
    (Both entries pass the caller's whole batch to launch_exact_eval:
    nemo_score and score_dev in csrc/nemo_abi.cpp call it once with `batch`,
    after nemo_reserve(batch) -- neither splits a call.)"""
    m, u, t = xe.model(s, e)
    n = 515
    perms, pos, w01 = _big_inputs(s, e, n)
    eng = _engine(m)
    try:
        assert _covered(eng, m)
        eng.set_option("exact_dev", 1)
        small = {"ll": [], "cs": [], "cells": [], "ow": []}
        for lo in range(0, n, 64):
            hi = min(n, lo + 64)
            a = _score_dev(eng, pos[lo:hi], w01[lo:hi], cap, "cs_ow")
            c = _score_dev(eng, pos[lo:hi], w01[lo:hi], cap, "cells")
            assert xe.bits_equal(a[0], c[0])
            small["ll"].append(a[0])
            small["cs"].append(a[1])
            small["ow"].append(a[3])
            small["cells"].append(c[2])
        small = {k: np.concatenate(v) for k, v in small.items()}
        for k in (0, 255, 511, 514):
            ref = xe.oracle_eval(u, t, perms[k], w01[k], cap)
            _check_eval((k, "calls of 64"), ref, small["ll"][k], small["cs"][k], small["cells"][k], small["ow"][k])
        for b in (512, 515):
            a = _score_dev(eng, pos[:b], w01[:b], cap, "cs_ow")
            c = _score_dev(eng, pos[:b], w01[:b], cap, "cells")
            ll_only = _score_dev(eng, pos[:b], w01[:b], cap, "ll")[0]
            assert xe.bits_equal(a[0], small["ll"][:b]) and xe.bits_equal(c[0], small["ll"][:b]), b
            assert xe.bits_equal(ll_only, small["ll"][:b]), b
            assert xe.bits_equal(a[1], small["cs"][:b]), b
            assert xe.bits_equal(a[3], small["ow"][:b]), b
            assert xe.bits_equal(c[2], small["cells"][:b]), b
        r = eng.score(pos[:512], w01[:512], cap=cap, want_cs=True, want_cells=True, want_ow=True)
        assert xe.bits_equal(r["ll"], small["ll"][:512]) and xe.bits_equal(r["cs"], small["cs"][:512])
        assert xe.bits_equal(r["cells"], small["cells"][:512]) and xe.bits_equal(r["ow"], small["ow"][:512])
        assert xe.bits_equal(eng.score(pos[:512], w01[:512], cap=cap), small["ll"][:512])
    finally:
        eng.close()


# --------------------------------------------------------------------------
# 3. fused steps at edge E
# --------------------------------------------------------------------------
def _step_refs(u, t, perms, ws):
    refs = [xe.oracle_step(u, t, perms[c], ws[c]) for c in range(len(perms))]
    s = t.shape[0]
    infos = []
    for r in refs:
        nit, nfev = np.full((s, s), -1), np.full((s, s), -1)
        for i, k, _c, _anc, _x0, _x, ni, nf in r["local"]:
            nit[i, k], nfev[i, k] = ni, nf
        infos.append((nit, nfev))
    return refs, infos


def _check_step(tag, got, refs, infos, chains):
    w_new, ll1, lld, info = got
    for c in chains:
        r = refs[c]
        q = c - chains[0]
        assert ll1[q] == r["ll1"] and lld[q] == r["dag"], (tag, c)
        assert xe.bits_equal(w_new[q], r["w"]), (tag, c)
        pair = infos[c][0] >= 0
        assert np.array_equal(info[q] != -1, pair), (tag, c)
        assert np.array_equal((info[q][pair] >> 4) & 0xfff, infos[c][0][pair]), (tag, c, "nit")
        assert np.array_equal(info[q][pair] >> 16, infos[c][1][pair]), (tag, c, "nfev")
        assert np.all((info[q][pair] & 15) <= 1), (tag, c, "status")


@pytest.mark.parametrize("e", xe.E_LIST)
@pytest.mark.parametrize("s", [2, 6, 12])
def test_fused_steps_equal_oracle_at_edge_e(s, e):
    """One fused step (eval #1, every pair's local optimum, the dag score) for
    one chain and for five, in the latency, throughput, pair, cached
    throughput, dual and slot forms with c stored and recomputed: ll1, every
    new weight, the dag ll and each pair's nit / nfev against
    OracleSampler(record_local=True), and the form that ran
    (exact_form_used) is the documented fall-back: 3 -> 2 with one slot, 5 -> 1
    past two slots or on stored rows, 7 -> 2 on stored rows, 6 whenever E >
    8192.  No oracle step raises at these seeds (model seed 3; orders and W
    from default_rng(7 E + S)): no E is left out for an abnormal line search.
    At E = 8191 the staging covers no exact step at all (65 leaf blocks,
    _covered): the test asserts that the engine says so."""
    m, u, t = xe.model(s, e)
    perms, ws = xe.step_inputs(s, e, 5)
    refs, infos = _step_refs(u, t, perms, ws)
    pos = np.stack([xe.pos_of(p) for p in perms])
    prep = [xe.host_prep(pos[c], ws[c]) for c in range(5)]
    w01, anc = np.stack([p[0] for p in prep]), np.stack([p[1] for p in prep])
    eng = _engine(m)
    try:
        if not _covered(eng, m):    # (E = 8191: no wave plan; the engine says so)
            return
        for form in FORMS:
            for cform in (0, 1):
                eng.set_option("exact_form", form)
                eng.set_option("exact_cform", cform)
                for chains in ([0], [0, 1, 2, 3, 4]):
                    got = eng.optimal_weights(pos[chains], w01[chains], anc[chains], ws[chains], SIG0, SIG1,
                                              raise_on_fail=False)
                    _check_step((form, cform), got, refs, infos, chains)
                    assert eng.get_option("exact_form_used") == xe.form_expected(form, cform, e), (form, cform)
                    _check_eval((form, cform, "order weights"),
                                xe.oracle_eval(u, t, perms[chains[-1]], w01[chains[-1]]),
                                ow=eng.order_weights(len(chains) - 1))
    finally:
        eng.close()


# --------------------------------------------------------------------------
# 4. the error-rate ladder in the exact arithmetic
# --------------------------------------------------------------------------
LADDER_SHAPES = [(k, s, e) for s, e in ((16, 40), (33, 130), (64, 40)) for k in range(len(fpm.LADDER))]
LADDER_SHAPES += [(k, 128, 40) for k in (9, 11, 12)]
# the rungs whose cells reach more than 707.70 below the column maximum
TAIL_RUNGS = {(9, 128), (11, 64), (11, 128), (12, 64), (12, 128)}


@pytest.mark.parametrize("k,s,e", LADDER_SHAPES, ids=[f"nem{k:02d}-S{s}-E{e}" for k, s, e in LADDER_SHAPES])
def test_error_rate_ladder_in_the_exact_arithmetic(k, s, e):
    """Error rates from (0.47, 0.47) down to 1e-12: |A|, |B| up to 27.6 and
    cells down to 2800 below the column maximum.  ll, cs and the cells to the
    bit; the order weights to the bit where the reference's argument cell - cs
    >= -707.70, exactly 0.0 below (reference <= 4.7e-308) -- the named rungs do
    reach there.  Up to S = 64 one fused step too: every weight, ll1, the dag
    ll and every pair's nit / nfev, to the bit (a flushed order weight leaves
    every local optimum where it is: |T| <= 170)."""
    mm = fpm.get_model(f"nem{k:02d}-S{s}-E{e}")
    u, t = np.ascontiguousarray(mm.U, dtype=np.float64), np.ascontiguousarray(mm.T, dtype=np.float64)
    perms, pos, w01 = fpm.inputs(s)
    eng = _engine(mm.nem)
    try:
        assert _covered(eng, mm.nem)
        r = eng.score(pos, w01, want_cs=True, want_cells=True, want_ow=True)
        tails = 0
        with np.errstate(under="ignore"):
            for b in range(len(perms)):
                ref = xe.oracle_eval(u, t, perms[b], w01[b])
                assert np.isfinite(ref[2]).all()
                _check_eval(b, ref, r["ll"][b], r["cs"][b], r["cells"][b], r["ow"][b])
                tails += int(xe.tail_mask(ref[2], ref[1]).sum())
        if (k, s) in TAIL_RUNGS:
            assert tails > 0
        if s <= 64:
            # (seeds at which every oracle step completes: with 31 S + k the line
            # search of one nem04-S64 pair ends abnormally in scipy itself)
            rng = np.random.default_rng(97 * s + k)
            sp, sw = [rng.permutation(s)], rng.uniform(-3, 3, (1, s, s))
            with np.errstate(under="ignore"):
                refs, infos = _step_refs(u, t, sp, sw)
            p1 = xe.pos_of(sp[0])[None]
            a01, anc = xe.host_prep(p1[0], sw[0])
            got = eng.optimal_weights(p1, a01[None], anc[None], sw, SIG0, SIG1, raise_on_fail=False)
            _check_step("step", got, refs, infos, [0])
            with np.errstate(under="ignore"):
                _check_eval("step ow", xe.oracle_eval(u, t, sp[0], a01), ow=eng.order_weights(0))
    finally:
        eng.close()


# --------------------------------------------------------------------------
# the gate of option exact_generic: max|T| <= 670
# --------------------------------------------------------------------------
def _tail_parent_tables(tval):
    """S = 3, order (0, 1, 2), real-valued rows: parent row 0 lies 707 .. 740
    below the column maximum U[3] = 700 (three of its five order weights in
    the flushed tail), and child 1 reads it through T[1][0] up to `tval` with
    w01[1][0] = 1.0."""
    e = 5
    rng = np.random.default_rng(670)
    u = rng.normal(0.0, 1.0, (4, e))
    u[3] = 700.0
    u[0] = [-7.0, -7.5, -8.0, -9.0, -40.0]
    t = rng.normal(0.0, 1.0, (3, 3, e))
    t[1, 0] = np.array([1.0, 1.0, 1.0, 0.999, 0.97]) * tval
    w = rng.uniform(-3, 3, (3, 3))
    w[1, 0] = 800.0          # expit = 1.0 exactly
    return u, t, np.arange(3), w


def test_generic_gate_tail_parent_row_at_the_bound():
    """A generic table whose flushed order weights meet lv = e^T: at max|T| =
    670 (limits.MAX_ABS_T_EXACT_GENERIC) the table is covered and the fused
    step is the oracle's to the bit -- |c| <= e^(670 - 707.70) < 2^-54, so 1 +
    c ex = 1 with numpy's weight or with 0.0; at 700 the table stages with
    exact_ok 0 and the sampler warns."""
    tmax = limits.MAX_ABS_T_EXACT_GENERIC
    u, t, perm, w = _tail_parent_tables(tmax)
    eng = Engine(u, t, exact_generic=True)
    try:
        assert not eng.factored and eng.get_option("exact_ok") == 1 and eng.exact_status() == (True, "")
        pos = xe.pos_of(perm)
        w01, anc = xe.host_prep(pos, w)
        assert w01[1, 0] == 1.0
        with np.errstate(under="ignore"):
            ref = xe.oracle_eval(u, t, perm, w01)
            refs, infos = _step_refs(u, t, [perm], w[None])
        tail = xe.tail_mask(ref[2], ref[1])
        assert tail[0].sum() == 3 and (ref[3][0][tail[0]] > 0.0).all()     # numpy's tail weights are not zero
        r = eng.score(pos[None], w01[None], want_cs=True, want_cells=True, want_ow=True)
        _check_eval("score", ref, r["ll"][0], r["cs"][0], r["cells"][0], r["ow"][0])
        assert (r["ow"][0][0][tail[0]] == 0.0).all()
        got = eng.optimal_weights(pos[None], w01[None], anc[None], w[None], SIG0, SIG1, raise_on_fail=False)
        _check_step("step", got, refs, infos, [0])
    finally:
        eng.close()
    u, t, perm, w = _tail_parent_tables(700.0)
    eng = Engine(u, t, exact_generic=True)
    try:
        assert eng.get_option("exact_generic") == 1 and eng.get_option("exact_ok") == 0
        ok, why = eng.exact_status()
        assert not ok and why.startswith("table form") and "670" in why
        with pytest.warns(ExactArithmeticWarning, match="table form"):
            NEMOrderMCMC(TableModel(u, t), perm, engine=eng)
        with pytest.raises(RuntimeError, match="table form"):
            NEMOrderMCMC(TableModel(u, t), perm, engine=eng, strict=True)
    finally:
        eng.close()
    with warnings.catch_warnings():          # and inside the bound the sampler constructs silently
        warnings.simplefilter("error", ExactArithmeticWarning)
        u, t, perm, w = _tail_parent_tables(tmax)
        eng = Engine(u, t, exact_generic=True)
        NEMOrderMCMC(TableModel(u, t), perm, engine=eng, strict=True)
        eng.close()
