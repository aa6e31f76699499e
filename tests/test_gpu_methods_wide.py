"""The fixed-order optimizer kernels (nemo_methods.hip) at the shapes
test_gpu_methods.py does not reach, each against a reference of the same
operation:

  a. gamma / inverse sweeps at S = 65, 96, 160 (column_solve<2> / <4>) against
     the reference's own output (methods_wide_*.npz, test_methods_wide_cpu.py);
  b. every NPL class of both pair kernels (E = 1 .. 5120; E > 2048 runs the
     objective that re-reads its table row), and the refusal at E = 5121,
     against the oracle (nemo_oracle.opt_gamma / opt_b, pinned to the reference
     by test_methods_oracle.py);
  c. the ancestral matrix for S = 2 .. 256 against a long-double forward
     substitution;
  d. the gamma sweep with a parent cap;
  e. batched against single calls at S = 70 (two-word reachability rows);
  f. f32 engines against the oracle on the float32-rounded tables.

Tolerances: ll within 1e-6 and every permissible pair's weight within
1e-6 max(1, |w_ref|) (test_gpu_methods.py's, relative for the inverse sweep's
large x); (c) and (f) measure theirs on the CPU, see there.  Every test prints
its worst errors (MEASUREMENTS.md, "Fixed-order optimizers past S = 64").

Starts make pairs move: gamma from uniform(0, 1), the inverse sweep from
uniform(-3, 1) (S <= 16) or a sparse DAG (methods_wide_inputs.inverse_start);
from the all-equal starts of test_gpu_methods.py most pairs stop where they
began and a wrong B[a][b] changes nothing."""
import functools
import sys

import numpy as np
import pytest
from conftest import GOLDEN, golden

import methods_wide_inputs as mw
import nemo_oracle as no
from nemo import _lib, generator
from nemo.engine import Engine

sys.path.insert(0, GOLDEN)
from generic_tables import generic_tables  # noqa: E402

pytestmark = pytest.mark.gpu

CONVERGED = (_lib.LBFGSB_CONV_PGTOL, _lib.LBFGSB_CONV_REL)


@functools.lru_cache(maxsize=None)
def _model(s, e, seed):
    return generator.synthetic_nem(s, e, seed)


def _engine(s, e, seed, dtype="f64"):
    return Engine.for_nem(_model(s, e, seed), dtype=dtype)  # cached on the model


def _unpack(info):
    return info & 15, (info >> 4) & 0xfff, (info >> 16) & 0x7fff


def _oracle_sweep(kind, u, t, order, w0, cap=0):
    """(ll, w, nit, nfev) of one oracle sweep, nit / nfev dense (-1 off the pairs)."""
    spy = mw.MinimizeSpy(no.minimize)
    real = no.minimize
    no.minimize = spy
    try:
        if kind == "inverse":
            ll, w = no.opt_b(u, t, order, w0)
        elif cap == 0:
            ll, w = no.opt_gamma(u, t, order, w0)
        else:
            ll, w = _opt_gamma_capped(u, t, order, w0, cap)
    finally:
        no.minimize = real
    s = len(order)
    nit = np.full((s, s), -1, dtype=np.int64)
    nfev = np.full((s, s), -1, dtype=np.int64)
    calls = iter(zip(spy.nit, spy.nfev))
    for i, pa in enumerate(no.parents_of(order, cap)):
        for k in pa:
            nit[i][k], nfev[i][k] = next(calls)
    return ll, w, nit, nfev


def _opt_gamma_capped(u, t, order, weights, cap):
    """nemo_oracle.opt_gamma (methods.py:397-405) on the parent sets of the
    build-defined cap: the last ``cap`` predecessors (parents_of)."""
    parents = no.parents_of(order, cap)
    ow, ll, _ = no.calculate_ll(no.cell_ratios(u, t, parents, weights))
    new = np.array(weights, dtype=np.float64, copy=True)
    for i in range(t.shape[0]):
        for k in parents[i]:
            lv = np.exp(t[i][k])
            a = (lv - 1.0) * ow[k]
            c = a / (1.0 - new[i][k] * a + new[i][k] * (lv - 1.0))
            res = no.minimize(no.local_ll_sum_gamma, x0=new[i][k], bounds=[(0, 1)], args=(c,), jac=True,
                              method="L-BFGS-B", tol=0.01)
            assert res.success
            new[i][k] = res.x[0]
    return ll, new


def _check_sweep(tag, kind, order, w0, got, ref, cap=0, w_tol=1e-6, ll_tol=1e-6):
    """The assertions on one problem of a sweep: got = (w, ll, info) from the
    device, ref = (ll, w, nit, nfev) of the reference.  Returns (pairs with the
    reference's (nit, nfev), pairs) for _check_share."""
    w, ll, info = got
    ll_ref, w_ref, nit_ref, nfev_ref = ref
    order = np.asarray(order)
    s = len(order)
    mask = np.zeros((s, s), dtype=bool)
    for i, pa in enumerate(no.parents_of(order, cap)):
        mask[i, pa] = True
    ll_err = abs(ll - ll_ref)
    # outside the (capped) parent sets: the weights as given, info untouched
    assert np.array_equal(w[~mask], w0[~mask]), tag
    assert (info[~mask] == -1).all(), tag
    status, nit, nfev = _unpack(info)
    assert np.isin(status[mask], CONVERGED).all(), (tag, np.unique(status[mask]))
    scale = np.maximum(1.0, np.abs(w_ref))
    err = np.where(mask, np.abs(w - w_ref) / scale, 0.0)
    same = mask & (nit == nit_ref) & (nfev == nfev_ref)
    moved = mask & (w_ref != w0)
    share_moved = (same & moved).sum() / max(1, moved.sum())
    if kind == "inverse":
        # pairs outside the lower triangle of order_arr's arrangement (node i sits
        # at index order[i]): B[a][b] = 0 whatever x, the clipped start comes back
        skipped = mask & (order[:, None] < order[None, :])
        assert np.array_equal(w[skipped], np.clip(w0[skipped], -5000.0, 500.0)), tag
        assert (nit[skipped] == 0).all() and (nfev[skipped] == 2).all(), tag
    bad = np.argwhere(err > w_tol)
    print(f"MW {tag}: pairs {mask.sum()} moved {moved.sum()} ll_err {ll_err:.3e} w_err {err.max():.3e} "
          f"same_nit_nfev {same.sum()} share_of_moved {share_moved:.4f}")
    assert ll_err <= ll_tol, (tag, ll, ll_ref)
    assert len(bad) == 0, (tag, "pairs past the tolerance (i, k, err, nit/nfev got, ref):",
                           [(int(i), int(k), float(err[i, k]), (int(nit[i, k]), int(nfev[i, k])),
                             (int(nit_ref[i, k]), int(nfev_ref[i, k]))) for i, k in bad[:10]])
    return int(same.sum()), int(mask.sum())


def _check_share(tag, counts):
    """At least 0.9 of a call's pairs took the reference's (nit, nfev): the
    figure test_bounded_spec_matches_scipy holds the specification to."""
    same, pairs = (sum(c) for c in zip(*counts))
    print(f"MW {tag}: (nit, nfev) as the reference's for {same} of {pairs} pairs, share {same / pairs:.4f}")
    assert same >= 0.9 * pairs, (tag, same, pairs)


# ---------------------------------------------------------------------------
# a. the fixture shapes: column_solve<2> and <4>
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture(name):
    z = golden(f"methods_wide_{name}.npz")
    order = z["order"].astype(np.int64)
    ii, kk = mw.pair_list(order)
    out = {"order": order}
    for kind, w0 in zip(("gamma", "inverse"), mw.fixture_starts(name, order)):
        assert w0.sum() == float(z[f"{kind}_start_sum"])
        w1 = w0.copy()
        w1[ii, kk] = z[f"{kind}_w"]
        s = len(order)
        nit = np.full((s, s), -1, dtype=np.int64)
        nfev = np.full((s, s), -1, dtype=np.int64)
        nit[ii, kk] = z[f"{kind}_nit"]
        nfev[ii, kk] = z[f"{kind}_nfev"]
        out[kind] = (w0, (float(z[f"{kind}_ll"]), w1, nit, nfev))
    return out


@pytest.mark.parametrize("kind", ["gamma", "inverse"])
@pytest.mark.parametrize("name", sorted(mw.FIXTURES))
def test_sweep_matches_reference_wide(name, kind):
    f = mw.FIXTURES[name]
    fx = _fixture(name)
    eng = _engine(f["S"], f["E"], f["model_seed"])
    w0, ref = fx[kind]
    pos = mw.positions(fx["order"])
    w, ll, info = (eng.gamma_sweep if kind == "gamma" else eng.inverse_sweep)(pos[None], w0)
    tag = f"a {name} {kind}"
    _check_share(tag, [_check_sweep(tag, kind, fx["order"], w0, (w[0], ll[0], info[0]), ref)])


# ---------------------------------------------------------------------------
# b. the NPL classes of both pair kernels
# ---------------------------------------------------------------------------
E_CLASSES = [1, 63, 64, 65, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097, 5119, 5120]


def _small_starts(kind, s, n, seed):
    """n orders of s nodes with a start on their permissible pairs: gamma
    uniform(0, 1), inverse uniform(-3, 1) over -5000."""
    rng = np.random.default_rng(seed)
    orders, ws = [], []
    for _ in range(n):
        order = rng.permutation(s)
        w = np.zeros((s, s)) if kind == "gamma" else np.full((s, s), -5000.0)
        for i, pa in enumerate(no.parents_of(order)):
            w[i, pa] = rng.uniform(0.0, 1.0, len(pa)) if kind == "gamma" else rng.uniform(-3.0, 1.0, len(pa))
        orders.append(order)
        ws.append(w)
    return orders, np.array(ws)


@pytest.mark.parametrize("kind", ["gamma", "inverse"])
@pytest.mark.parametrize("e", E_CLASSES)
def test_sweep_matches_oracle_every_npl(e, kind):
    """S = 6, three orders in one call.  npl_m picks NPL = 4, 8, 16, 32, 48,
    64, 80 at E <= 256, 512, 1024, 2048, 3072, 4096, 5120; each class is run
    at its upper edge and one past the edge below it."""
    s = 6
    m = _model(s, e, 100 + e)
    eng = _engine(s, e, 100 + e)
    t = m.get_score_tensor()
    orders, ws = _small_starts(kind, s, 3, 7000 + e)
    pos = np.array([mw.positions(o) for o in orders])
    w, ll, info = (eng.gamma_sweep if kind == "gamma" else eng.inverse_sweep)(pos, ws)
    counts = []
    for p, order in enumerate(orders):
        ref = _oracle_sweep(kind, m.U, t, order, ws[p])
        counts.append(_check_sweep(f"b E={e} {kind} #{p}", kind, order, ws[p], (w[p], ll[p], info[p]), ref))
    _check_share(f"b E={e} {kind}", counts)


def test_e_past_5120_is_refused():
    """80 elements per lane is the largest instantiation: E = 5121 fails in the
    argument checks of all three calls, before anything is copied or launched."""
    s, e = 6, 5121
    eng = _engine(s, e, 100 + e)
    orders, ws = _small_starts("gamma", s, 1, 1)
    pos = mw.positions(orders[0])[None]
    for call in (lambda: eng.gamma_sweep(pos, ws), lambda: eng.inverse_sweep(pos, ws),
                 lambda: eng.inverse_ancestral(pos, ws)):
        with pytest.raises(_lib.NemoError) as ei:
            call()
        assert ei.value.code == _lib.NEMO_ERR_ARG and "5120" in str(ei.value), str(ei.value)


# ---------------------------------------------------------------------------
# c. the ancestral matrix for every NS
# ---------------------------------------------------------------------------
def _ancestral_longdouble(order, w):
    """unorder_arr(B / (1 + B)), B = (I - order_arr(exp(W)))^-1 by forward
    substitution on the lower triangle, in np.longdouble."""
    s = len(order)
    m = no.order_arr(order, np.exp(w.astype(np.longdouble)))
    b = np.zeros((s, s), dtype=np.longdouble)
    one = np.longdouble(1.0)
    for c in range(s):
        row = m[c, :c] @ b[:c, :] if c else np.zeros(s, dtype=np.longdouble)
        row[c] += one
        b[c] = row / (one - m[c, c])
    return no.unorder_arr(order, b / (one + b))


def _ancestral_cases(s, seed):
    """Five (order, W): three with uniform(-3, 1) on the permissible pairs, one
    sparse DAG (density 0.1), one sparse DAG with entries at the bounds: a few
    pairs written as -5000 explicitly, and three parents of the node at the
    last index of order_arr's arrangement at 500 (no path holds two of them,
    so exp(500) stays inside fp64)."""
    rng = np.random.default_rng(seed)
    cases = []
    for kind in ("dense", "dense", "dense", "sparse", "bounds"):
        order = rng.permutation(s)
        w = np.full((s, s), -5000.0)
        for i, pa in enumerate(no.parents_of(order)):
            v = rng.uniform(-3.0, 1.0, len(pa))
            if kind != "dense":
                v = np.where(rng.random(len(pa)) < 0.1, v, -5000.0)
            w[i, pa] = v
        if kind == "bounds":
            last = int(np.where(order == s - 1)[0][0])  # node i with order[i] = s - 1
            pa = no.parents_of(order)[last]
            w[last, pa[:3]] = 500.0
            w[last, pa[3:6]] = -5000.0
        cases.append((kind, order, w))
    return cases


@pytest.mark.parametrize("s", [2, 63, 64, 65, 127, 128, 129, 255, 256])
def test_ancestral_matches_longdouble(s):
    """ancestral_kernel<1> (S <= 64), <2> (<= 128), <4> (<= 256) at both edges
    of each.  Per case the deviation of scipy's fp64 solve_triangular
    (nemo_oracle._b_inv) from the long-double reference is measured here; the
    kernel is allowed four times that, and no less than 1e-12 relative (its exp
    and its summation order differ from scipy's by a few ulp per term).
    Entries above the column (outside the lower triangle) are exactly 0."""
    eng = _engine(s, 8, 200 + s)
    cases = _ancestral_cases(s, 300 + s)
    pos = np.array([mw.positions(o) for _, o, _ in cases])
    got = eng.inverse_ancestral(pos, np.array([w for _, _, w in cases]))
    for p, (kind, order, w) in enumerate(cases):
        ref = _ancestral_longdouble(order, w)
        assert np.isfinite(ref.astype(np.float64)).all()
        ref64 = ref.astype(np.float64)
        nz = ref64 != 0.0
        dev_scipy = float(np.max(np.abs((no._b_inv(order, w, np.eye(s)) - ref)[nz] / ref[nz])))
        dev_kernel = float(np.max(np.abs((got[p] - ref)[nz] / ref[nz])))
        tol = max(4.0 * dev_scipy, 1e-12)
        print(f"MW c S={s} {kind} #{p}: scipy_dev {dev_scipy:.3e} kernel_dev {dev_kernel:.3e} tol {tol:.3e}")
        assert dev_kernel <= tol, (s, kind, dev_kernel, tol)
        # index space: node i sits at index order[i]; above the diagonal is 0,
        # and so is every entry the reference has at 0 (no path)
        upper = order[:, None] < order[None, :]
        assert (got[p][upper] == 0.0).all()
        assert (got[p][~nz] == 0.0).all()
        assert (np.diag(got[p]) == 0.5).all()  # B[c][c] = 1 / (1 - exp(-5000)) = 1


# ---------------------------------------------------------------------------
# d. the gamma sweep with a parent cap
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 5, 32])
def test_gamma_sweep_with_cap(cap):
    """pairs_per_chain(S, cap) pairs per problem, read from pairs[b S S + n]:
    three orders in one call, so problems 1 and 2 read past problem 0's list."""
    s, e = 33, 184
    m = _model(s, e, 8)
    eng = _engine(s, e, 8)
    t = m.get_score_tensor()
    rng = np.random.default_rng(80 + cap)
    orders = [rng.permutation(s) for _ in range(3)]
    ws = np.array([np.where(generator.permissible_mask(mw.positions(o)), rng.uniform(0.0, 1.0, (s, s)), 0.0)
                   for o in orders])
    pos = np.array([mw.positions(o) for o in orders])
    w, ll, info = eng.gamma_sweep(pos, ws, cap=cap)
    counts = []
    for p, order in enumerate(orders):
        ref = _oracle_sweep("gamma", m.U, t, order, ws[p], cap=cap)
        assert (ref[2] >= 0).sum() == sum(min(q, cap) for q in range(s))
        counts.append(_check_sweep(f"d cap={cap} #{p}", "gamma", order, ws[p], (w[p], ll[p], info[p]), ref, cap=cap))
    _check_share(f"d cap={cap}", counts)


# ---------------------------------------------------------------------------
# e. batched against single calls past S = 64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gamma", "inverse"])
def test_batched_problems_equal_single_wide(kind):
    """test_batched_problems_equal_single at S = 70: the merged inverse
    schedule with two-word reachability rows, column_solve<2>."""
    s, e = 70, 100
    eng = _engine(s, e, 6)
    eng.reserve(3, 3)
    rng = np.random.default_rng(9)
    orders = [rng.permutation(s) for _ in range(3)]
    pos = np.array([mw.positions(o) for o in orders])
    if kind == "gamma":
        ws = np.array([mw.gamma_start(o, 90 + p) for p, o in enumerate(orders)])
    else:
        ws = np.array([mw.inverse_start(o, 90 + p, 0.1) for p, o in enumerate(orders)])
    f = eng.gamma_sweep if kind == "gamma" else eng.inverse_sweep
    wb, llb, infob = f(pos, ws)
    moved = 0
    for p in range(3):
        w1, ll1, info1 = f(pos[p:p + 1], ws[p:p + 1])
        assert np.array_equal(w1[0], wb[p]) and ll1[0] == llb[p] and np.array_equal(info1[0], infob[p])
        moved += int((w1[0] != ws[p]).sum())
    print(f"MW e {kind}: moved {moved}")
    assert moved >= 30


# ---------------------------------------------------------------------------
# f. f32 engines
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gamma", "inverse"])
@pytest.mark.parametrize("tables", ["nem", "own"])
def test_f32_engine_matches_oracle_on_rounded_tables(tables, kind):
    """The float instantiations of both pair kernels (S = 16, E = 500).  An
    f32 engine stores float32(U) and float32(exp(T)); the reference is the
    oracle on exactly those values.  What remains is the f32 arithmetic of the
    score kernel in the order weights.  Its allowance is measured here: the
    distance the oracle's outputs move between the fp64 and the rounded
    inputs, times four.

    ``nem``: the tables of synthetic_nem(16, 500, 0).  They are factorable, so
    the evaluation runs the factored score kernels, which keep U in fp64: the
    device lands on the fp64 oracle (ll to 1e-12, x* to 1e-8) and uses none of
    the allowance beyond the inputs' own distance.  ``own``: real-valued
    tables with a row of their own per (child, parent) (generic_tables), which
    the generic f32 score kernel evaluates: each cell is a product of up to
    S - 1 fp32 factors, every factor and every product rounded once (unit
    roundoff u = 2^-24), so a cell's log is off by at most 2 S u and the sum
    of the E column log-sum-exps by at most 2 S E u = 9.5e-4; the ll is allowed
    that on top (measured: 6.7e-6 and 4.6e-6, against input distances of
    2.3e-7 and 3.3e-7).  The weights keep four times the input distance."""
    s, e = 16, 500
    if tables == "nem":
        m = _model(s, e, 0)
        u, t = m.U, m.get_score_tensor()
    else:
        u, t = generic_tables("own", s, e, 21)
    eng = Engine(u, t, dtype="f32")
    u32 = u.astype(np.float32).astype(np.float64)
    t32 = np.log(np.exp(t).astype(np.float32).astype(np.float64))
    orders, ws = _small_starts(kind, s, 1, 16)
    order, w0 = orders[0], ws[0]
    ref64 = _oracle_sweep(kind, u, t, order, w0)
    ref32 = _oracle_sweep(kind, u32, t32, order, w0)
    mask = generator.permissible_mask(mw.positions(order))
    scale = np.maximum(1.0, np.abs(ref32[1]))
    d_ll = abs(ref64[0] - ref32[0])
    d_w = float(np.max(np.abs(ref64[1] - ref32[1])[mask] / scale[mask]))
    w, ll, info = (eng.gamma_sweep if kind == "gamma" else eng.inverse_sweep)(mw.positions(order)[None], w0)
    status, nit, nfev = _unpack(info[0])
    e_ll = abs(ll[0] - ref32[0])
    e_w = float(np.max(np.abs(w[0] - ref32[1])[mask] / scale[mask]))
    share = ((nit == ref32[2]) & (nfev == ref32[3]))[mask].mean()
    print(f"MW f {tables} {kind}: oracle fp64->rounded d_ll {d_ll:.3e} d_w {d_w:.3e}; "
          f"device e_ll {e_ll:.3e} e_w {e_w:.3e} share {share:.4f}; "
          f"device to the fp64 oracle: ll {abs(ll[0] - ref64[0]):.3e} "
          f"w {float(np.max(np.abs(w[0] - ref64[1])[mask] / scale[mask])):.3e}")
    assert d_ll > 0.0 and d_w > 0.0
    assert np.isin(status[mask], CONVERGED).all()
    assert np.array_equal(w[0][~mask], w0[~mask]) and (info[0][~mask] == -1).all()
    ll_allow = 4.0 * d_ll + (2.0 * s * e * 2.0 ** -24 if tables == "own" else 0.0)
    assert e_ll <= ll_allow, (e_ll, d_ll, ll_allow)
    assert e_w <= 4.0 * d_w, (e_w, d_w)
