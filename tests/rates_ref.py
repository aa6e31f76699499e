"""Long-double reference, tolerances, inputs and a plain fp64 restatement for
the order score at per-gene error rates (nemo_score_rates, csrc/nemo_grad.hip).

With D (S, E) the knockdown matrix and per-gene A_k = log(alpha_k / (1 -
beta_k)), B_k = log(beta_k / (1 - alpha_k)), the tables of nem.py:25-64 become

    T[i][j][e] = D[j][e] ? -A_j : B_j                       (j != i)
    U[i][e]    = (D[i][e] ? 0 : B_i) + sum_{k != i} D[k][e] A_k
    U[S][e]    = sum_k D[k][e] A_k.

``tables`` builds them in np.longdouble; ll, d ll / d w and their tolerances
then come from fixed_point_models.reference(full=True) and
score_grad_ref.grad_reference as they stand.  The derivatives in the rates
are the direct per-effect sums over the order weights ow = exp(cell - cs),

    dA_k = sum_e D[k][e] (1 - ow[k][e] - sum_i h_ik ow[i][e])
    dB_k = sum_e (1 - D[k][e]) (ow[k][e] + sum_i k_ik ow[i][e]),

i over the children that have k as a permissible parent, h_ik = w e^{-A_k} /
(1 - w + w e^{-A_k}), k_ik = w e^{B_k} / (1 - w + w e^{B_k}), w = w01[i][k].

Tolerances, derived as score_grad_ref derives its own.  An error d of a cell
or of cs is a relative error d of an order weight: 2 tol_cell(n, big), n the
most parents of any child and big the evaluation's largest finite |cell|; the
sums over E, the part and wave sums and the sum over up to S children add (E +
64 + S) 2^-52.  Each derivative is a sum of terms of one sign per group, so
with rel = 2 tol_cell + (E + 64 + S) 2^-52

    tol_A[k] = 4 rel (n_k + M_kk + sum_i h_ik M_ik)
    tol_B[k] = 4 rel (R_k + sum_i k_ik R_i)

(M_ik = sum_e ow[i][e] D[k][e], R_i = sum_e ow[i][e]: R - M is formed by
subtraction, so its error is relative to R), the factor 4 as in
score_grad_ref.  The kernel adds sum_k A_k n_k to the offset form's sum in S
further additions: tol_ll += (S + 4) 2^-53 sum_k |A_k| n_k.

``rates_numpy`` is a plain fp64 restatement of the kernel's assembly (the
offset form, M, R, the diagonal, R - M); tests/test_rates_cpu.py holds it to a
quarter of every tolerance.  No GPU and no library here.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import fixed_point_models as fm
import score_grad_ref as gr
import stream_models as sm

LD = np.longdouble
EPS52 = 2.0 ** -52
EPS53 = 2.0 ** -53

LADDER_RUNGS = gr.LADDER_RUNGS
FUSED_S = gr.FUSED_S
SMALL_S = gr.SMALL_S
SMALL_E = gr.SMALL_E
SETTINGS = ("scalar", "per-gene", "per-eval")
DIAG_S = (16, 33, 64)
FIT_ERRORS = (0.05, 0.10)
FIT_START = (0.2, 0.2)
REL_DIFF = 1e-8


def log_ratios(alpha, beta):
    alpha, beta = np.asarray(alpha, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    return np.log(alpha / (1.0 - beta)), np.log(beta / (1.0 - alpha))


# ---- inputs ------------------------------------------------------------------
def ladder_ids():
    return [f"{r}-S{s}-E{e}" for r in LADDER_RUNGS for s in FUSED_S for e in fm.EFFECTS]


def small_ids():
    return [f"small-S{s}-E{e}" for s in SMALL_S for e in SMALL_E] + ["small-S17-E1040"]


def small_d(s, e):
    """A seeded D of density 0.4 with rows that start with 1 and with 0, one
    all-ones row and (S > 2) one all-zeros row."""
    rng = np.random.default_rng(7000 + 100 * s + e)
    d = (rng.random((s, e)) < 0.4).astype(np.uint8)
    d[::2, 0] = 1
    d[1::2, 0] = 0
    d[s - 1] = 1
    if s > 2:
        d[s // 2] = 0
    return d


def per_gene_rates(s, seed):
    """alpha, beta log-uniform in [1e-9, 0.45], all 2 S of them distinct -> (A, B) (S,)."""
    rng = np.random.default_rng(seed)
    r = np.exp(rng.uniform(np.log(1e-9), np.log(0.45), 2 * s))
    assert np.unique(r).size == 2 * s
    return log_ratios(r[:s], r[s:])


@functools.lru_cache(maxsize=4)
def model_d(name):
    """(D uint8 (S, E), the model's own scalar (A, B))."""
    kind, s, e = name.split("-")
    s, e = int(s[1:]), int(e[1:])
    if kind == "small":
        return small_d(s, e), log_ratios(0.07, 0.12)
    m = fm.get_model(name)
    return np.ascontiguousarray(m.nem.observed_knockdown_mat, dtype=np.uint8), (float(m.nem.A), float(m.nem.B))


def case_inputs(name, setting):
    """(D, perms, pos, w01, A (n, S), B (n, S)) of a model under one of SETTINGS."""
    d, (a0, b0) = model_d(name)
    s = d.shape[0]
    perms, pos, w01 = fm.inputs(s)
    n = len(perms)
    if setting == "scalar":
        a, b = np.full((n, s), a0), np.full((n, s), b0)
    elif setting == "per-gene":
        ag, bg = per_gene_rates(s, 900 + s)
        a, b = np.tile(ag, (n, 1)), np.tile(bg, (n, 1))
    else:
        ab = [per_gene_rates(s, 1300 + 17 * k + s) for k in range(n)]
        a, b = np.stack([x[0] for x in ab]), np.stack([x[1] for x in ab])
    return d, perms, np.ascontiguousarray(pos), np.ascontiguousarray(w01), np.ascontiguousarray(a), np.ascontiguousarray(b)


# ---- the long-double reference -------------------------------------------------
def tables(d, a, b):
    """(U (S + 1, E), T (S, S, E), exp(T)) in long double; T and exp(T) are
    read-only broadcasts of their (S, E) rows (the diagonal is never read)."""
    d = np.asarray(d).astype(bool)
    s, e = d.shape
    a, b = np.broadcast_to(np.asarray(a, dtype=LD), (s,)), np.broadcast_to(np.asarray(b, dtype=LD), (s,))
    rows = np.where(d, -a[:, None], b[:, None])
    null = (d * a[:, None]).sum(axis=0)
    u = np.empty((s + 1, e), dtype=LD)
    u[:s] = np.where(d, LD(0), b[:, None]) + (null[None] - d * a[:, None])
    u[s] = null
    return u, np.broadcast_to(rows[None], (s, s, e)), np.broadcast_to(np.exp(rows)[None], (s, s, e))


@dataclass
class RatesRef:
    ll: float
    cs: np.ndarray       # (E,) long double
    g: np.ndarray        # (S, S) long double
    tol: np.ndarray      # (S, S)
    tol_ll: float
    da: np.ndarray       # (S,) long double
    db: np.ndarray
    tol_a: np.ndarray    # (S,) float64
    tol_b: np.ndarray


def rates_reference(d, a, b, perm, w01, cap=0) -> RatesRef:
    d = np.asarray(d).astype(bool)
    s, e = d.shape
    perm = np.asarray(perm)
    a, b = np.broadcast_to(np.asarray(a, dtype=LD), (s,)), np.broadcast_to(np.asarray(b, dtype=LD), (s,))
    u, t, et = tables(d, a, b)
    full = fm.reference(u, t, perm, w01, cap, full=True, et=et)
    ref = gr.grad_reference(u, t, perm, w01, cap, et=et, full=full)
    _, cs, cells, ow = full
    big = float(np.abs(cells[np.isfinite(cells)]).max())
    nk = d.sum(axis=1).astype(LD)
    one = LD(1)
    dl = d.astype(LD)
    ena, eb = np.exp(-a), np.exp(b)
    suma = np.zeros((s, e), dtype=LD)     # sum_i h_ik ow[i][e]
    sumb = np.zeros((s, e), dtype=LD)
    ta = np.zeros(s, dtype=LD)            # sum_i h_ik M_ik
    tb = np.zeros(s, dtype=LD)            # sum_i k_ik R_i
    for p in range(s):
        i = perm[p]
        pa = gr._parents(perm, p, cap)
        if not pa.size:
            continue
        w = w01[i, pa].astype(LD)
        h = w * ena[pa] / (one - w + w * ena[pa])
        k = w * eb[pa] / (one - w + w * eb[pa])
        suma[pa] += h[:, None] * ow[i][None]
        sumb[pa] += k[:, None] * ow[i][None]
        ta[pa] += h * (dl[pa] * ow[i][None]).sum(axis=1)
        tb[pa] += k * ow[i].sum()
    da = (dl * (one - ow[:s] - suma)).sum(axis=1)
    db = ((one - dl) * (ow[:s] + sumb)).sum(axis=1)
    mkk = (dl * ow[:s]).sum(axis=1)
    rk = ow[:s].sum(axis=1)
    rel = 2.0 * sm.tol_cell(int(ref.n.max()), big) + (e + 64 + s) * EPS52
    tol_a = (4.0 * rel * (nk + mkk + ta)).astype(np.float64)
    tol_b = (4.0 * rel * (rk + tb)).astype(np.float64)
    tol_ll = ref.tol_ll + (s + 4) * EPS53 * float((np.abs(a) * nk).sum())
    return RatesRef(ref.ll, cs, ref.g, ref.tol, tol_ll, da, db, tol_a, tol_b)


@functools.lru_cache(maxsize=None)
def case_refs(name, setting, cap):
    """RatesRef of every evaluation of a model under a setting and a cap, computed once."""
    d, perms, _, w01, a, b = case_inputs(name, setting)
    return [rates_reference(d, a[k], b[k], perms[k], w01[k], cap) for k in range(len(perms))]


def ll_longdouble(d, a, b, perm, w01, cap=0):
    """ll alone, in long double (for differences)."""
    u, t, et = tables(d, a, b)
    return fm.reference(u, t, perm, w01, cap, full=True, et=et)[1].sum()


# ---- a plain fp64 restatement of the kernel's assembly ---------------------------
def rates_numpy(d, a, b, perm, w01, cap=0):
    """-> (ll, grad (S, S), dA (S,), dB (S,)) in numpy fp64: the offset form x =
    cell - U[S], M = ow D^T, R, the diagonal M_kk, and f'_lo (R - M) + f'_hi M."""
    d = np.asarray(d).astype(bool)
    s, e = d.shape
    df = d.astype(np.float64)
    perm = np.asarray(perm)
    a, b = np.broadcast_to(np.asarray(a, dtype=np.float64), (s,)), np.broadcast_to(np.asarray(b, dtype=np.float64), (s,))
    ena, eb = np.exp(-a), np.exp(b)
    nk = df.sum(axis=1)
    x = np.where(d, -a[:, None], b[:, None])
    fac = {}
    for p in range(s):
        i = perm[p]
        pa = gr._parents(perm, p, cap)
        if pa.size:
            w = w01[i, pa]
            dlo, dhi = w * eb[pa] + (1.0 - w), w * ena[pa] + (1.0 - w)
            lo, hi = np.log(dlo), np.log(dhi)
            x[i] = x[i] + (lo.sum() + (hi - lo) @ df[pa])
            fac[i] = (pa, w, dlo, dhi)
    m = np.maximum(x.max(axis=0), 0.0)
    cs = m + np.log(np.exp(x - m).sum(axis=0) + np.exp(-m))
    ow = np.exp(x - cs)
    ll = float((a * nk).sum() + cs.sum())
    # M[i][k] and R[i] as sums of the same kind over e, as in the kernel, where both leave one
    # MFMA chain: for an all-ones row D[k] the addends ow D = ow and the order are R's own, so
    # M = R bit for bit and R - M is exactly 0, whatever f'_lo of the absent value 0 is
    mm = (ow[:, None, :] * df[None]).sum(axis=2)
    r = ow.sum(axis=1)
    diag = (ow * df).sum(axis=1)
    g = np.zeros((s, s))
    suma, sumb = np.zeros(s), np.zeros(s)
    for i, (pa, w, dlo, dhi) in fac.items():
        g[i, pa] = (eb[pa] - 1.0) / dlo * (r[i] - mm[i, pa]) + (ena[pa] - 1.0) / dhi * mm[i, pa]
        suma[pa] += w * ena[pa] / dhi * mm[i, pa]
        sumb[pa] += w * eb[pa] / dlo * (r[i] - mm[i, pa])
    return ll, g, nk - diag - suma, (r - diag) + sumb


# ---- the absolute likelihood and the fit case ------------------------------------
def baseline(d, alpha, beta):
    """sum_k [ n_k log(1 - beta_k) + (E - n_k) log(1 - alpha_k) ] in fp64."""
    d = np.asarray(d)
    n = d.sum(axis=1).astype(np.float64)
    al, be = np.broadcast_to(alpha, n.shape), np.broadcast_to(beta, n.shape)
    return float((n * np.log1p(-be) + (d.shape[1] - n) * np.log1p(-al)).sum())


def mixture_ll(d, alpha, beta, perm, w01):
    """log prod_e (1 / (S + 1)) sum_{i or null} P(D[:, e] | effect e attached to i) for 0/1
    weights, computed directly in long double: the effect responds to the knockdown of gene k
    iff k is i or one of i's parents with weight 1 (w01[i][k] = 1, k before i)."""
    d = np.asarray(d).astype(bool)
    s, e = d.shape
    al, be = np.broadcast_to(np.asarray(alpha, dtype=LD), (s,)), np.broadcast_to(np.asarray(beta, dtype=LD), (s,))
    ok = gr.permissible(perm)
    p1 = np.where(d, (1 - be)[:, None], be[:, None])     # P(D[k][e] | responds)
    p0 = np.where(d, al[:, None], (1 - al)[:, None])     # P(D[k][e] | does not)
    tot = np.prod(p0, axis=0)                            # the null attachment
    for i in range(s):
        resp = (ok[i] & (w01[i] == 1.0))
        resp[i] = True
        tot = tot + np.prod(np.where(resp[:, None], p1, p0), axis=0)
    return float(np.log(tot / LD(s + 1)).sum())


@functools.lru_cache(maxsize=1)
def fit_case():
    """(D, order, W): synthetic_nem(16, 130, 5, errors = FIT_ERRORS), the genes sorted stably by
    their number of ancestors in the graph's closure C (C[i][j] = 1: i is a parent of j), and the
    fixed weights W[j][i] = C[i][j]."""
    from nemo import generator
    m = generator.synthetic_nem(16, 130, 5, errors=FIT_ERRORS)
    c = generator.transitive_closure(np.asarray(m.adj_matrix))
    order = np.argsort(c.sum(axis=0), kind="stable")
    return np.ascontiguousarray(m.observed_knockdown_mat, dtype=np.uint8), order, c.T.astype(np.float64)


def big_l_numpy(d, order, w, alpha, beta):
    """(L, dL/dalpha, dL/dbeta) at scalar rates, from rates_numpy and the chain rule."""
    a, b = log_ratios(alpha, beta)
    ll, _, da, db = rates_numpy(d, a, b, order, w)
    n = np.asarray(d).sum(axis=1).astype(np.float64)
    e = d.shape[1]
    sa, sb = da.sum(), db.sum()
    # A = log alpha - log(1 - beta), B = log beta - log(1 - alpha)
    dl_al = sa / alpha + sb / (1.0 - alpha) - (e - n).sum() / (1.0 - alpha)
    dl_be = sa / (1.0 - beta) + sb / beta - n.sum() / (1.0 - beta)
    return ll + baseline(d, alpha, beta), float(dl_al), float(dl_be)


@functools.lru_cache(maxsize=1)
def cpu_fit(bounds=(1e-12, 0.5)):
    """scipy's L-BFGS-B on -L of the restatement over the sigmoid parameters, from FIT_START:
    -> (L_fit, alpha, beta, iterations, L_start, L at the generating rates)."""
    from scipy.optimize import minimize
    from scipy.special import expit
    d, order, w = fit_case()
    lo, hi = bounds

    def rate(u):
        return lo + (hi - lo) * expit(u)

    def fun(u):
        al, be = rate(u[0]), rate(u[1])
        big_l, gal, gbe = big_l_numpy(d, order, w, al, be)
        sig = expit(u)
        return -big_l, -np.array([gal, gbe]) * (hi - lo) * sig * (1.0 - sig)

    t0 = (np.array(FIT_START) - lo) / (hi - lo)
    u0 = np.log(t0 / (1.0 - t0))
    res = minimize(fun, u0, jac=True, method="L-BFGS-B", options={"ftol": REL_DIFF, "gtol": 1e-10, "maxiter": 200})
    l_start = big_l_numpy(d, order, w, *FIT_START)[0]
    l_truth = big_l_numpy(d, order, w, *FIT_ERRORS)[0]
    return float(-res.fun), float(rate(res.x[0])), float(rate(res.x[1])), int(res.nit), l_start, l_truth
