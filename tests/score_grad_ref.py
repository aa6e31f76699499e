"""Long-double reference, tolerance and inputs for the order-score gradient
(nemo_score_grad, csrc/nemo_grad.hip).

With cell[i][e] = U[i][e] + sum_{j in pa(i)} log(1 - w_ij + w_ij v), v =
exp(T[i][j][e]), and ll = sum_e logsumexp_i cell[i][e] (null row included),

    d ll / d w_ij = sum_e ow[i][e] f'_ij(e),   f' = (v - 1) / (1 - w + w v),

at the permissible pairs and 0 elsewhere.  The reference starts from
``fixed_point_models.reference(..., full=True)`` (cs, cells and order weights
in np.longdouble) and forms the sums in long double.

Tolerance, from the project's own cell tolerance (stream_models.tol_cell):

    tol_ij = 4 [ (2 tol_cell(n_i, big) + (E + 64) 2^-52) scale_ij
                 + 2^-52 sum_e ow[i][e] max(v, 1) / den_ij(e) ]
    scale_ij = (sum_e ow[i][e]) max_e |f'_ij(e)|

n_i = parents of i under the cap, big = the evaluation's largest finite
|cell|.  An error d of a cell or of cs is a relative error d of ow = exp(cell -
cs): 2 tol_cell.  (E + 64) 2^-52 covers the sum over E and the quotient; the
last term is the rounding of the staged exp(T) (a relative error 2^-53 of v
moves f' by at most 2^-53 max(v, 1) / den).  The factor 4 covers the kernels'
table exponential and the MFMA's summation order, which numpy does not share.
tests/test_score_grad_cpu.py holds a plain numpy fp64 restatement (and, for
factored models, the kernels' assembly f'_lo (R - M) + f'_hi M) to a quarter
of it on every input below.

No GPU and no library here.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import fixed_point_models as fm
import stream_models as sm

LD = np.longdouble
EPS52 = 2.0 ** -52

# ---- inputs ----------------------------------------------------------------
LADDER_RUNGS = ("nem00", "nem04", "nem08", "nem12")
FUSED_S = (16, 33, 60, 64)
TABLE_MODELS = ("table-mixed-S16-E40", "table-deep-S8-E40", "table-edge-S8-E40")
SMALL_S = (2, 15, 17)
SMALL_E = (1, 15, 16, 17, 63, 64, 65)
PART_MODEL = "small-S17-E1040"     # past the fused kernel's E cut (1024 effects per block): two parts
WIDE_MODEL = "nem04-S128-E40"      # 64 < S: the two-pass path on auto
GENERIC = ("f64-shared-S2-E63-a3", "f64-own-S9-E64-a70", "f64-shared-S9-E65-a70", "f64-own-S18-E130-a3",
           "f64-own-S65-E65-a3", "f64-shared-S5-E4100-a3", "f64-own-S9-E63-a171-generic")


def factored_ids():
    """The factored models with S <= 64 (the fused path; the two-pass path under grad_path 1)."""
    ids = [f"{r}-S{s}-E{e}" for r in LADDER_RUNGS for s in FUSED_S for e in fm.EFFECTS]
    return ids + list(TABLE_MODELS) + [f"small-S{s}-E{e}" for s in SMALL_S for e in SMALL_E] + [PART_MODEL]


def factored_caps(s):
    return tuple(dict.fromkeys(c for c in (0, 1, 3, s - 2, s + 5) if c >= 0))


def generic_caps(s):
    return tuple(dict.fromkeys((0, 1, 3, s - 1)))


def _small_model(s, e):
    """A seeded two-valued table T[i][j] = R[j] at the smallest shapes where a
    row block, a 16-effect tile or a 64-bit word ends."""
    rng = np.random.default_rng(4000 + 100 * s + e)
    lo = rng.uniform(-3.0, 1.0, s)
    hi = lo + rng.choice([-1.0, 1.0], s) * rng.uniform(0.5, 4.0, s)
    bits = rng.random((s, e)) < 0.4
    bits[:, 0] = False
    r = np.where(bits, hi[:, None], lo[:, None])
    t = np.empty((s, s, e))
    t[:] = r[None]
    return fm.Model(f"small-S{s}-E{e}", rng.normal(-2.0, 2.0, (s + 1, e)), t)


@functools.lru_cache(maxsize=4)
def get_model(name) -> fm.Model:
    if name.startswith("small-"):
        _, s, e = name.split("-")
        return _small_model(int(s[1:]), int(e[1:]))
    return fm.get_model(name)


def factored_inputs(name):
    """(model, perms, pos, w01): fixed_point_models.inputs' evaluations of a factored model."""
    m = get_model(name)
    perms, pos, w01 = fm.inputs(m.S)
    return m, perms, np.ascontiguousarray(pos), np.ascontiguousarray(w01)


def generic_inputs(name):
    """(case, U, T, perms, pos, w01) of one of stream_models' cases."""
    c = sm.BY_NAME[name]
    u, t = sm.tables(name)
    perms, pos, w01 = sm.evals(c.s, c.nevals)
    return c, u, t, perms, pos, w01


# ---- the reference -----------------------------------------------------------
def permissible(perm, cap=0):
    """(S, S) bool by node: j is a permissible parent of i."""
    s = len(perm)
    pos = np.empty(s, dtype=np.int64)
    pos[np.asarray(perm)] = np.arange(s)
    d = pos[:, None] - pos[None, :]
    ok = d > 0
    if 0 < cap < s - 1:
        ok &= d <= cap
    return ok


@dataclass
class GradRef:
    ll: float
    cs: np.ndarray       # (E,) long double
    g: np.ndarray        # (S, S) long double, 0 off the permissible set
    tol: np.ndarray      # (S, S) float64 (0 off the permissible set)
    tol_ll: float
    n: np.ndarray        # (S,) parents per child


def _parents(perm, p, cap):
    return perm[max(0, p - cap) if cap else 0:p]


def grad_reference(u, t, perm, w01, cap=0, et=None, full=None) -> GradRef:
    """The long-double gradient of one evaluation and its tolerance.  ``et``:
    exp(T) in long double; ``full``: fm.reference(..., full=True) of the same
    evaluation, when the caller already holds it."""
    s, e = t.shape[0], t.shape[2]
    perm = np.asarray(perm)
    ll, cs, cells, ow = full if full is not None else fm.reference(u, t, perm, w01, cap, full=True, et=et)
    big = float(np.abs(cells[np.isfinite(cells)]).max())
    g = np.zeros((s, s), dtype=LD)
    tol = np.zeros((s, s))
    n = np.zeros(s, dtype=np.int64)
    one = LD(1)
    for p in range(s):
        i = perm[p]
        pa = _parents(perm, p, cap)
        n[i] = pa.size
        if not pa.size:
            continue
        w = w01[i, pa].astype(LD)[:, None]
        v = np.exp(t[i, pa].astype(LD)) if et is None else et[i, pa]
        den = one - w + w * v
        fp = (v - one) / den
        g[i, pa] = (ow[i][None] * fp).sum(axis=1)
        scale = ow[i].sum() * np.abs(fp).max(axis=1)
        stage = (ow[i][None] * np.maximum(v, one) / den).sum(axis=1)
        tol[i, pa] = 4.0 * ((2.0 * sm.tol_cell(int(pa.size), big) + (e + 64) * EPS52) * scale
                            + EPS52 * stage).astype(np.float64)
    tll = sm.tol_ll(cs, sm.tol_cell(int(n.max()), big))
    return GradRef(float(ll), cs, g, tol, tll, n)


@functools.lru_cache(maxsize=None)
def factored_refs(name, cap):
    """GradRef of every evaluation of a factored model under ``cap``, computed once."""
    m, perms, _, w01 = factored_inputs(name)
    et = np.exp(m.T.astype(LD))
    return [grad_reference(m.U, m.T, p, w, cap, et=et) for p, w in zip(perms, w01)]


@functools.lru_cache(maxsize=None)
def generic_refs(name, cap):
    """The same for one of stream_models' cases (its cached reference extended)."""
    c, u, t, perms, _, w01 = generic_inputs(name)
    r = sm.refs(name, cap)
    et = sm._exp_table(name)
    return [grad_reference(u, t, perms[k], w01[k], cap, et=et,
                           full=(float(r.ll[k]), r.cs[k], r.cells[k], r.ow[k])) for k in range(len(perms))]


# ---- a plain fp64 restatement (what the tolerance is checked against on the CPU) ----
def grad_numpy(u, t, perm, w01, cap=0, assembly="direct"):
    """The gradient in numpy fp64.  ``assembly``: "direct" sums ow f' over E;
    "factored" (two-valued rows only) forms f'_lo (R - M) + f'_hi M with M =
    sum_e ow D1 and R = sum_e ow, as the fused kernel does."""
    s = t.shape[0]
    perm = np.asarray(perm)
    cell = np.array(u, dtype=np.float64)
    fac = {}
    for p in range(s):
        i = perm[p]
        pa = _parents(perm, p, cap)
        if pa.size:
            w = w01[i, pa][:, None]
            v = np.exp(t[i, pa])
            den = (1.0 - w) + w * v
            fac[i] = (pa, w, v, den)
            cell[i] += np.log(den).sum(axis=0)
    mx = cell.max(axis=0)
    cs = mx + np.log(np.exp(cell - mx).sum(axis=0))
    ow = np.exp(cell - cs)
    g = np.zeros((s, s))
    for i, (pa, w, v, den) in fac.items():
        if assembly == "direct":
            g[i, pa] = (ow[i][None] * ((v - 1.0) / den)).sum(axis=1)
            continue
        lo = t[i, pa][:, :1]
        bits = t[i, pa] != lo
        vlo = np.exp(lo)
        vhi = np.exp(np.where(bits.any(axis=1, keepdims=True), np.max(np.where(bits, t[i, pa], -np.inf), axis=1,
                                                                      keepdims=True), lo))
        flo = (vlo - 1.0) / ((1.0 - w) + w * vlo)
        fhi = (vhi - 1.0) / ((1.0 - w) + w * vhi)
        r = ow[i].sum()
        mm = (ow[i][None] * bits).sum(axis=1, keepdims=True)
        g[i, pa] = (flo * (r - mm) + fhi * mm)[:, 0]
    return float(cs.sum()), g
