"""Long-double reference, tolerance and inputs for one sequential sweep over
the single-weight moves of an order (nemo_edge_sweep, csrc/nemo_sweep.hip).

The call visits the permissible pairs in order -- children by order position q
= 1 .. S - 1, within a child its parents by order position -- scores the move
w_ij -> w'_ij at the CURRENT state as moves_ref does,

    gain = sum_e t_e,   t_e = log1p(x_e),   x_e = ow[i][e] kappa_ij(e),

and takes it iff gain > thr[i][j].  Taking it moves the state exactly:

    cs[e] += t_e,   ow[i][e] *= (1 + kappa_ij(e)) / (1 + x_e),   ow[k][e] /= 1 + x_e  (k != i),

with 1 + kappa = f_ij(w') / f_ij(w).  ``sweep_reference`` keeps, in long double,
the rows ow0[k] times their own moves' ratios and one c[e] = the change of
cs[e] so far; the current row of child i is rows[i] exp(-c).  1 + x is formed
without the cancellation of 1 - ow[i], as in moves_ref: the other rows' order
weights plus ow[i] f(w') / f(w).  tests/test_sweep_cpu.py checks gains and the
final score against brute-force rescoring of the swept weights.

Tolerance of a visit's gain, derived as moves_ref derives tol_ij.  The visit's
x_e carries the relative error of its order weight and of kappa,

    relx_e = 8 2^-52 + ec_e + er_e.

8 2^-52 is kappa and the product (moves_ref).  ec_e bounds the absolute error
dc of c[e], which is a relative error -dc of every current row.  er_e bounds the
relative error dr the child's row carries beside that: it starts, when the
child's turn comes, at moves_ref's cell / cs term 2 tol_cell(n_i, big) + 8
2^-52 (ow0 itself, exp(-c) and their product).  A taken move carries both on, to
first order and with signs: t_e moves by (dr - dc) x / (1 + x) + fresh, so

    dc' = dc + dt = dc / (1 + x) + dr x / (1 + x) + fresh,
    row' = row (1 + kappa) / (1 + x):  dr' - dc' = (dr - dc) / (1 + x) + ...,  so  dr' = dr + fresh,

    ec' = ec / (1 + x) + er |x| / (1 + x) + fresh,     er' = er + fresh + 12 2^-52,
    fresh = 8 2^-52 (|x| / (1 + x) + max(|t|, 0.5 [|x| >= 2^-8])) + 2 2^-52 |t|

(kappa's error through t, the log1p routine's own error, the additions; 12
2^-52 for the quotient, the products and the clamp).  A move that lowers the
child's cell (x < 0) amplifies the error of c by 1 / (1 + x), one that raises it
damps it: that is the conditioning of holding ow rather than 1 - ow.  Then

    tol = 4 [ sum_e relx_e |x_e| / (1 + x_e) + (E + 64) 2^-52 sum_e |t_e|
              + 8 2^-52 sum_e max(|t_e|, 0.5 if |x_e| >= 2^-8 else 0) ]

-- moves_ref's tol_ij at the visit's state with its first term widened per
effect; the factor 4 covers the kernels' table exponential and summation
order.  Where ow[i][e] rounds to 1 and v is below the rounding of 1 the first
term is astronomically wide (moves_ref), and after such a move is taken every
later visit's is: such models belong to the forced-decision tests only.

ll0: stream_models.tol_ll at w01.  ll: stream_models.tol_ll of the swept
weights plus the sum of the taken visits' tolerances (ll = ll0 + sum_e c[e],
and c is the sum of the taken t).  A plain numpy fp64 restatement
(``sweep_numpy``, the kernel's own bookkeeping) stays within a half of both on
every input below (tests/test_sweep_cpu.py).

No GPU and no library here.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import fixed_point_models as fm
import moves_ref as mr
import stream_models as sm
from score_grad_ref import (SMALL_E, SMALL_S, _parents, factored_caps, generic_caps, get_model,  # noqa: F401
                            permissible)

LD = np.longdouble
EPS52 = 2.0 ** -52
SMALL = 2.0 ** -8
FLOOR = 2.0 ** -54

# ---- the cases ---------------------------------------------------------------
# the smallest shapes at which the kernel can go wrong: a single pair; fewer
# effects than threads, the wave and word edges, one wave at 1 and 2 effects
# per thread (E <= 64, 65); 4 per thread (129); every block-size switch (257:
# 128 threads, 513: 256, 1025 and 1040: 512, 2049: 1024) and the instances
# that keep no t_e (4097: 8, 8193: 16 effects per thread); the ladder; past S = 64
SMALL_MODELS = tuple(f"small-S{s}-E{e}" for s in SMALL_S for e in SMALL_E)
SWITCH_MODELS = ("small-S17-E1040", "small-S5-E129", "small-S5-E257", "small-S5-E513", "small-S5-E1025",
                 "small-S3-E2049", "small-S3-E4097", "small-S2-E8193")
LADDER_MODELS = ("nem04-S16-E40", "nem08-S16-E40", "nem04-S33-E40", "nem00-S60-E130", "nem04-S64-E130")
TABLE_MODELS = ("table-mixed-S16-E40", "table-edge-S8-E40")
WIDE_MODEL = mr.WIDE_MODEL
DECISION_FACTORED = SMALL_MODELS + SWITCH_MODELS + LADDER_MODELS + TABLE_MODELS + (WIDE_MODEL,)
GENERIC = tuple(n for n in mr.GENERIC if n.endswith("-a3"))
# No decision margin: a saturated child (ow = 1 in fp64) against e^T below the
# rounding of 1 -- the tolerance of such a visit is astronomically wide, and a
# run of taken moves that lower a nearly saturated child's cell multiplies the
# error of c by 1 / (1 + x) each (measured here: nem08-S60-E130 and nem12-S60-E40
# reach tolerances of 1e5 and 1e22 at a few visits, the tables of amplitude 70
# and 171 reach 1e60).  These run in the forced-decision and same-bits tests.
FORCED_FACTORED = ("table-deep-S8-E40", "nem08-S60-E130")
FORCED_GENERIC = tuple(n for n in mr.GENERIC if not n.endswith("-a3"))


def eval_subset(s, n):
    """The evaluations of a case's list the sweep tests take: all of them up to S
    = 17; from there on a soft and a saturated random order and a random DAG
    (the reference walks S (S - 1) / 2 visits per evaluation and cap)."""
    if s <= 17:
        return tuple(range(n))
    return (0, 5) if s > 64 else (0, 1, 5)


def thresholds(tag, n, s):
    """thr (n, S, S): logit(u), u ~ U(0, 1) from a generator seeded per evaluation by the case's name."""
    base = sum(ord(ch) * (k + 1) for k, ch in enumerate(tag)) % 100003
    out = np.empty((n, s, s))
    for k in range(n):
        u = np.random.default_rng(9000 + 137 * base + k).random((s, s))
        out[k] = np.log(u) - np.log1p(-u)
    return out


@functools.lru_cache(maxsize=None)
def factored_case(name):
    """(model, perms, pos, w01, w_alt, thr) of a factored model's sweep tests."""
    m, perms, pos, w01 = mr.factored_inputs(name)
    wa = mr.factored_alt(name)
    keep = list(eval_subset(m.S, len(perms)))
    thr = thresholds(name, len(perms), m.S)
    c = np.ascontiguousarray
    return m, [perms[k] for k in keep], c(pos[keep]), c(w01[keep]), c(wa[keep]), c(thr[keep])


@functools.lru_cache(maxsize=None)
def generic_case(name):
    """(case, U, T, perms, pos, w01, w_alt, thr) of one of stream_models' cases."""
    cs, u, t, perms, pos, w01 = mr.generic_inputs(name)
    wa = mr.generic_alt(name)
    keep = list(eval_subset(cs.s, len(perms)))
    thr = thresholds(name, len(perms), cs.s)
    c = np.ascontiguousarray
    return cs, u, t, [perms[k] for k in keep], c(pos[keep]), c(w01[keep]), c(wa[keep]), c(thr[keep])


# ---- the reference -------------------------------------------------------------
@dataclass
class SweepRef:
    w_out: np.ndarray     # (S, S) float64
    alt_out: np.ndarray
    cs0: np.ndarray       # (E,) long double, at w01
    cs: np.ndarray        # (E,) long double, at w_out (cs0 + c)
    gain: np.ndarray      # (S, S) long double, 0 off the permissible set
    tol: np.ndarray       # (S, S) float64 (0 off the permissible set and where w_alt == w01)
    acc: np.ndarray       # (S, S) bool
    margin: np.ndarray    # (S, S) |gain - thr| (inf off the permissible set)
    visits: list          # (i, j) in visit order
    nacc: int
    tol_ll0: float
    tol_ll: float


def sweep_reference(u, t, perm, w01, w_alt, thr, cap=0, et=None) -> SweepRef:
    """The long-double sweep of one evaluation and its tolerances."""
    s, e = t.shape[0], t.shape[2]
    perm = np.asarray(perm)
    _, cs0, cells, ow = fm.reference(u, t, perm, w01, cap, full=True, et=et)
    cells = np.array(cells, dtype=LD)
    big = float(np.abs(cells[np.isfinite(cells)]).max())
    rows = np.array(ow, dtype=LD)
    one = LD(1)
    c = np.zeros(e, dtype=LD)
    ec = np.zeros(e, dtype=LD)
    w_out, alt_out = np.array(w01, dtype=np.float64), np.array(w_alt, dtype=np.float64)
    gain = np.zeros((s, s), dtype=LD)
    tol = np.zeros((s, s))
    acc = np.zeros((s, s), dtype=bool)
    margin = np.full((s, s), np.inf)
    visits, nmax, tol_taken = [], 0, 0.0
    for q in range(1, s):
        i = perm[q]
        pa = _parents(perm, q, cap)
        nmax = max(nmax, int(pa.size))
        rest0 = np.delete(rows, i, axis=0).sum(axis=0)
        er = np.full(e, 2.0 * sm.tol_cell(int(pa.size), big) + 8.0 * EPS52, dtype=LD)
        for j in pa:
            visits.append((int(i), int(j)))
            w, wa = LD(w01[i, j]), LD(w_alt[i, j])
            d = wa - w
            th = thr[i, j]
            if d == 0:
                g, tl, take = LD(0), 0.0, 0.0 > th
            else:
                v = np.exp(t[i, j].astype(LD)) if et is None else et[i, j]
                den = one - w + w * v
                ratio = (one - wa + wa * v) / den
                scale = np.exp(-c)
                owi = rows[i] * scale
                x = owi * (d * (v - one) / den)
                onepx = rest0 * scale + owi * ratio
                small = np.abs(x) < SMALL
                tt = np.where(small, np.log1p(np.where(small, x, 0)), np.log(onepx))
                g = tt.sum()
                at = np.abs(tt)
                rout = np.maximum(at, np.where(small, LD(0), LD(0.5)))
                relx = 8.0 * EPS52 + ec + er
                sens = np.abs(x) / onepx
                tl = float(4.0 * ((relx * sens).sum() + (e + 64) * EPS52 * at.sum() + 8.0 * EPS52 * rout.sum()))
                take = bool(g > th)
                if take:
                    fresh = 8.0 * EPS52 * (sens + rout) + 2.0 * EPS52 * at
                    ec = ec / onepx + er * sens + fresh
                    er = er + fresh + 12.0 * EPS52
                    c = c + tt
                    rows[i] = rows[i] * ratio
                    cells[i] = cells[i] + np.log(ratio)
            gain[i, j], tol[i, j] = g, tl
            margin[i, j] = abs(float(g) - th)
            if take:
                acc[i, j] = True
                tol_taken += tl
                w_out[i, j], alt_out[i, j] = w_alt[i, j], w01[i, j]
    cs = cs0 + c
    big1 = max(big, float(np.abs(cells[np.isfinite(cells)]).max()))
    return SweepRef(w_out, alt_out, cs0, cs, gain, tol, acc, margin, visits, int(acc.sum()),
                    sm.tol_ll(cs0, sm.tol_cell(nmax, big)), sm.tol_ll(cs, sm.tol_cell(nmax, big1)) + tol_taken)


@functools.lru_cache(maxsize=None)
def factored_refs(name, cap):
    """SweepRef of every evaluation of factored_case(name) under ``cap``, computed once."""
    m, perms, _, w01, wa, thr = factored_case(name)
    et = np.exp(m.T.astype(LD))
    return [sweep_reference(m.U, m.T, p, w, a, th, cap, et=et) for p, w, a, th in zip(perms, w01, wa, thr)]


@functools.lru_cache(maxsize=None)
def generic_refs(name, cap):
    _, u, t, perms, _, w01, wa, thr = generic_case(name)
    et = sm._exp_table(name)
    return [sweep_reference(u, t, p, w, a, th, cap, et=et) for p, w, a, th in zip(perms, w01, wa, thr)]


# ---- a plain fp64 restatement: the kernel's own bookkeeping -----------------------
def sweep_numpy(u, t, perm, w01, w_alt, thr, cap=0):
    """(w_out, alt_out, ll0, ll, gain (S, S), nacc) in numpy fp64: the forward of
    moves_ref.moves_numpy, then c[e] and the current child's row as the kernel keeps them."""
    s, e = t.shape[0], t.shape[2]
    perm = np.asarray(perm)
    cell = np.array(u, dtype=np.float64)
    for p in range(s):
        i = perm[p]
        pa = _parents(perm, p, cap)
        if pa.size:
            w = w01[i, pa][:, None]
            cell[i] += np.log((1.0 - w) + w * np.exp(t[i, pa])).sum(axis=0)
    mx = cell.max(axis=0)
    cs = mx + np.log(np.exp(cell - mx).sum(axis=0))
    ow = np.exp(cell - cs)
    c = np.zeros(e)
    w_out, alt_out = np.array(w01, dtype=np.float64), np.array(w_alt, dtype=np.float64)
    gain = np.zeros((s, s))
    nacc = 0
    for q in range(1, s):
        i = perm[q]
        owc = ow[i] * np.exp(-c)
        for j in _parents(perm, q, cap):
            w, wa = w01[i, j], w_alt[i, j]
            d = wa - w
            g = 0.0
            if d != 0.0:
                v = np.exp(t[i, j])
                f = (1.0 - w) + w * v
                x = owc * (d * ((v - 1.0) / f))
                small = np.abs(x) < SMALL
                tt = np.where(small, np.log1p(np.where(small, x, 0.0)), np.log(np.maximum(1.0 + x, FLOOR)))
                g = float(tt.sum())
            gain[i, j] = g
            if g > thr[i, j]:
                nacc += 1
                w_out[i, j], alt_out[i, j] = wa, w
                if d != 0.0:
                    c += tt
                    owc = np.minimum(owc * (((1.0 - wa) + wa * v) / f) / np.maximum(1.0 + x, FLOOR), 1.0)
    ll0 = float(cs.sum())
    return w_out, alt_out, ll0, ll0 + float(c.sum()), gain, nacc


class NumpySweepEngine(mr.NumpyEngine):
    """``Engine.edge_sweep`` (and ``score_moves``) on the CPU through sweep_numpy:
    what sweep_flips and gibbs_edges are driven by without a device."""

    def edge_sweep(self, pos, w01, w_alt, thr, cap=0):
        pos = np.atleast_2d(pos)
        b = len(pos)
        w_out, alt_out = np.empty((b, self.S, self.S)), np.empty((b, self.S, self.S))
        ll0, ll = np.empty(b), np.empty(b)
        gain = np.empty((b, self.S, self.S))
        nacc = np.empty(b, dtype=np.int32)
        for k, pk in enumerate(pos):
            w_out[k], alt_out[k], ll0[k], ll[k], gain[k], nacc[k] = sweep_numpy(
                self.U, self.T, np.argsort(pk), np.asarray(w01)[k], np.asarray(w_alt)[k], np.asarray(thr)[k], cap)
        return w_out, alt_out, ll0, ll, gain, nacc


class Recording:
    """An engine's edge_sweep with the arguments of every call kept."""

    def __init__(self, eng):
        self.eng, self.calls = eng, []

    def edge_sweep(self, pos, w01, w_alt, thr, cap=0):
        self.calls.append((np.array(pos), np.array(w01), np.array(w_alt), np.array(thr), cap))
        return self.eng.edge_sweep(pos, w01, w_alt, thr, cap=cap)


def call_refs(m, calls):
    """SweepRef of every problem of every recorded call: [call][problem]."""
    et = np.exp(m.T.astype(LD))
    return [[sweep_reference(m.U, m.T, np.argsort(pos[k]), w01[k], wa[k], thr[k], cap, et=et) for k in range(len(pos))]
            for pos, w01, wa, thr, cap in calls]


def least_clearance(refs, calls):
    """min over every visit of every recorded call of |gain - thr| - 2 tol (must be positive)."""
    least = np.inf
    for row, (pos, _, _, _, cap) in zip(refs, calls):
        for k, ref in enumerate(row):
            ok = permissible(np.argsort(pos[k]), cap)
            least = min(least, float((ref.margin[ok] - 2.0 * ref.tol[ok]).min()))
    return least


# ---- the Gibbs tests' model, chains and seed ---------------------------------------
# tests/test_sweep_cpu.py enumerates the 8 DAGs of the order's 3 pairs and asserts, on
# the CPU, that edge_prob lies within 5 standard errors of the exact marginals with room
GIBBS_MODEL = "small-S3-E17"
GIBBS_B = 48
GIBBS_SWEEPS = 60
GIBBS_BURN = 10
GIBBS_BETA = 0.7
GIBBS_RHO = -0.4
GIBBS_SEED = 11


def gibbs_inputs():
    """(model, pos (B, 3), weights (B, 3, 3)): B chains on one seeded order, random 0/1 starts."""
    m = get_model(GIBBS_MODEL)
    rng = np.random.default_rng(GIBBS_SEED)
    perm = rng.permutation(m.S)
    pos = np.empty((GIBBS_B, m.S), dtype=np.int32)
    pos[:, perm] = np.arange(m.S)
    w = (rng.random((GIBBS_B, m.S, m.S)) < 0.5) * permissible(perm)[None]
    return m, pos, w.astype(np.float64)
