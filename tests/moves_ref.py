"""Long-double reference, tolerance and inputs for the exact score change of
every single-weight move (nemo_score_moves, csrc/nemo_moves.hip).

With cell[i][e] = U[i][e] + sum_{j in pa(i)} log f_ij(e), f = 1 - w + w v, v =
exp(T[i][j][e]), ow = exp(cell - cs) and ll = sum_e cs[e], replacing ONE
weight w_ij by w'_ij moves only row i of the cells, so

    ll(w with w_ij := w'_ij) - ll(w) = sum_e log1p(ow[i][e] kappa_ij(e)),
    kappa_ij(e) = (w'_ij - w_ij) (v - 1) / f_ij(e)

at the permissible pairs and 0 elsewhere.  The reference starts from
``fixed_point_models.reference(..., full=True)`` and forms the sums in long
double; tests/test_moves_cpu.py checks the closed form against brute-force
rescoring.

Tolerance per pair, derived as score_grad_ref derives its own.  With x_e =
ow[i][e] kappa_ij(e) and t_e = log1p(x_e):

    tol_ij = 4 [ (2 tol_cell(n_i, big) + 8 2^-52) sum_e |x_e| / (1 + x_e)
                 + (E + 64) 2^-52 sum_e |t_e|
                 + 8 2^-52 sum_e max(|t_e|, 0.5 if |x_e| >= 2^-8 else 0) ]

An error d of a cell or of cs is a relative error d of ow (2 tol_cell), and
kappa -- a difference, a quotient, a product and the staged exp(T) -- carries
a few ulp more (8 2^-52); a relative error of x moves log1p(x) by |x| / (1 +
x) times it.  (E + 64) 2^-52 covers the sum over E.  The last term is the
device's log1p routine: relative below 2^-8 (the series), log_fast's absolute
ulp of max(|t|, 0.5) from there on.  The factor 4 covers the kernels' table
exponential and summation order, as in score_grad_ref.  Where ow[i][e] rounds
to 1 and v is below the rounding of 1 (a saturated child against a table entry
past -37), 1 + x has no correct digit in fp64 -- the true value needs 1 - ow --
and the first term says so: it grows like 1 / (1 + x), so such a pair's
tolerance is astronomically wide and only a finite value is asked there.  (The
reference forms 1 + x for these terms without the cancellation, see below.)  A plain numpy fp64
restatement stays within a half of it on every input below
(tests/test_moves_cpu.py).

No GPU and no library here.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import fixed_point_models as fm
import stream_models as sm
from score_grad_ref import (GENERIC, PART_MODEL, WIDE_MODEL, _parents, factored_caps, factored_ids,  # noqa: F401
                            factored_inputs, generic_caps, generic_inputs, get_model, permissible)

LD = np.longdouble
EPS52 = 2.0 ** -52
SMALL = 2.0 ** -8


# ---- inputs ------------------------------------------------------------------
def alt_weights(w01, seed):
    """w_alt of one evaluation: uniform in [0, 1]; a quarter of the entries 0, a
    quarter 1, a fifth the flip of the rounded w01, a twentieth w01 itself
    (those moves must score exactly 0)."""
    rng = np.random.default_rng(seed)
    out = rng.random(w01.shape)
    r = rng.random(w01.shape)
    out[r < 0.25] = 0.0
    out[(r >= 0.25) & (r < 0.5)] = 1.0
    flip = (r >= 0.5) & (r < 0.7)
    out[flip] = 1.0 - np.round(w01[flip])
    same = (r >= 0.7) & (r < 0.75)
    out[same] = w01[same]
    return out


def alt_batch(w01, tag):
    """w_alt (n, S, S) of a batch of evaluations, seeded by the case's name."""
    base = sum(ord(ch) * (k + 1) for k, ch in enumerate(tag)) % 100003
    return np.ascontiguousarray(np.stack([alt_weights(w, 7000 + 131 * base + k) for k, w in enumerate(w01)]))


@functools.lru_cache(maxsize=None)
def factored_alt(name):
    return alt_batch(factored_inputs(name)[3], name)


@functools.lru_cache(maxsize=None)
def generic_alt(name):
    return alt_batch(generic_inputs(name)[5], name)


# ---- the reference -------------------------------------------------------------
@dataclass
class MovesRef:
    ll: float
    cs: np.ndarray       # (E,) long double
    dll: np.ndarray      # (S, S) long double, 0 off the permissible set
    tol: np.ndarray      # (S, S) float64 (0 off the permissible set)
    tol_ll: float


def moves_reference(u, t, perm, w01, w_alt, cap=0, et=None, full=None) -> MovesRef:
    """The long-double move scores of one evaluation and their tolerance.
    ``et``: exp(T) in long double; ``full``: fm.reference(..., full=True)."""
    s, e = t.shape[0], t.shape[2]
    perm = np.asarray(perm)
    ll, cs, cells, ow = full if full is not None else fm.reference(u, t, perm, w01, cap, full=True, et=et)
    big = float(np.abs(cells[np.isfinite(cells)]).max())
    dll = np.zeros((s, s), dtype=LD)
    tol = np.zeros((s, s))
    nmax = 0
    one = LD(1)
    for p in range(s):
        i = perm[p]
        pa = _parents(perm, p, cap)
        nmax = max(nmax, int(pa.size))
        if not pa.size:
            continue
        w = w01[i, pa].astype(LD)[:, None]
        d = w_alt[i, pa].astype(LD)[:, None] - w
        v = np.exp(t[i, pa].astype(LD)) if et is None else et[i, pa]
        den = one - w + w * v
        x = ow[i][None] * (d * (v - one) / den)
        # 1 + x without the cancellation of 1 - ow[i] and of v - 1, which long
        # double loses where ow[i] = 1 and v < 2^-64 to its rounding (tables past
        # |T| = 44): the other rows' order weights plus ow[i] f(w') / f(w)
        wa = w_alt[i, pa].astype(LD)[:, None]
        onepx = np.delete(ow, i, axis=0).sum(axis=0)[None] + ow[i][None] * ((one - wa + wa * v) / den)
        tt = np.where(np.abs(x) < SMALL, np.log1p(np.where(np.abs(x) < SMALL, x, 0)), np.log(onepx))
        dll[i, pa] = tt.sum(axis=1)
        at = np.abs(tt)
        tc = 2.0 * sm.tol_cell(int(pa.size), big) + 8.0 * EPS52
        rout = np.maximum(at, np.where(np.abs(x) >= SMALL, LD(0.5), LD(0)))
        tol[i, pa] = 4.0 * (tc * (np.abs(x) / onepx).sum(axis=1) + (e + 64) * EPS52 * at.sum(axis=1)
                            + 8.0 * EPS52 * rout.sum(axis=1)).astype(np.float64)
    tll = sm.tol_ll(cs, sm.tol_cell(nmax, big))
    return MovesRef(float(ll), cs, dll, tol, tll)


@functools.lru_cache(maxsize=None)
def factored_refs(name, cap):
    """MovesRef of every evaluation of a factored model under ``cap``, computed once."""
    m, perms, _, w01 = factored_inputs(name)
    wa = factored_alt(name)
    et = np.exp(m.T.astype(LD))
    return [moves_reference(m.U, m.T, p, w, a, cap, et=et) for p, w, a in zip(perms, w01, wa)]


@functools.lru_cache(maxsize=None)
def generic_refs(name, cap):
    """The same for one of stream_models' cases (its cached reference extended)."""
    c, u, t, perms, _, w01 = generic_inputs(name)
    wa = generic_alt(name)
    r = sm.refs(name, cap)
    et = sm._exp_table(name)
    return [moves_reference(u, t, perms[k], w01[k], wa[k], cap, et=et,
                            full=(float(r.ll[k]), r.cs[k], r.cells[k], r.ow[k])) for k in range(len(perms))]


# ---- a plain fp64 restatement (what the tolerance is checked against on the CPU) ----
def moves_numpy(u, t, perm, w01, w_alt, cap=0):
    """(ll, dll (S, S)) in numpy fp64: the forward of score_grad_ref.grad_numpy,
    then sum_e log1p(ow kappa)."""
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
    dll = np.zeros((s, s))
    for i, (pa, w, v, den) in fac.items():
        d = w_alt[i, pa][:, None] - w
        x = ow[i][None] * (d * ((v - 1.0) / den))
        small = np.abs(x) < SMALL
        # (1 + x rounds to 0 where ow = 1 and v < 2^-53; it then stands for a value
        # in (0, 2^-54], and the device's routine takes 2^-54)
        dll[i, pa] = np.where(small, np.log1p(np.where(small, x, 0.0)),
                              np.log(np.maximum(1.0 + x, 2.0 ** -54))).sum(axis=1)
    return float(cs.sum()), dll


class NumpyEngine:
    """``Engine.score_moves`` on the CPU through moves_numpy: what a pure-numpy
    greedy search is driven by (no device, no library)."""

    def __init__(self, u, t):
        self.U, self.T = np.asarray(u, dtype=np.float64), np.asarray(t, dtype=np.float64)
        self.S, self.E = self.T.shape[0], self.T.shape[2]
        self.calls = []      # the w01 of every call

    def score_moves(self, pos, w01, w_alt, cap=0):
        pos = np.atleast_2d(pos)
        self.calls.append(np.array(w01))
        ll = np.empty(len(pos))
        dll = np.empty((len(pos), self.S, self.S))
        for k, pk in enumerate(pos):
            ll[k], dll[k] = moves_numpy(self.U, self.T, np.argsort(pk), w01[k], w_alt[k], cap)
        return ll, dll


def numpy_greedy(eng, pos, weights, cap=0, max_iter=None, min_gain=1e-9):
    """The greedy search written out problem by problem: -> (weights, flips,
    margins); flips[k] the (i, j) sequence of problem k, margins[k] each step's
    best gain minus the second best (and, at the last call, min_gain minus the
    best: how clearly the search stopped)."""
    pos = np.atleast_2d(pos)
    b, s = pos.shape
    out = np.array(weights, dtype=np.float64)
    flips, margins = [], []
    for k in range(b):
        w = out[k]
        ok = permissible(np.argsort(pos[k]), cap)
        fl, mg = [], []
        for _ in range(s * s if max_iter is None else max_iter):
            _, dll = eng.score_moves(pos[k:k + 1], w[None], 1.0 - w[None], cap=cap)
            gain = np.where(ok, dll[0], -np.inf).ravel()
            order = np.argsort(-gain, kind="stable")
            if not gain[order[0]] > min_gain:
                mg.append(min_gain - gain[order[0]])
                break
            mg.append(gain[order[0]] - max(gain[order[1]], min_gain) if ok.sum() > 1 else np.inf)
            i, j = divmod(int(order[0]), s)
            w[i, j] = 1.0 - w[i, j]
            fl.append((i, j))
        flips.append(fl)
        margins.append(mg)
    return out, flips, margins


def flips_of(calls):
    """The (i, j) sequence of every problem from the w01 of successive score_moves calls."""
    b = calls[0].shape[0]
    seq = [[] for _ in range(b)]
    for prev, cur in zip(calls, calls[1:]):
        for k in range(b):
            for i, j in zip(*np.nonzero(prev[k] != cur[k])):
                seq[k].append((int(i), int(j)))
    return seq


# the greedy tests' model, batch and seed: tests/test_moves_cpu.py asserts that on
# the CPU every step's best gain clears the second best (and the stop clears
# min_gain) by more than GREEDY_MARGIN, so a device within tolerance takes the same steps
GREEDY_MODEL = "nem04-S16-E40"
GREEDY_B = 9
GREEDY_SEED = 2
GREEDY_MARGIN = 1e-9


def greedy_inputs(start):
    """(model, pos (B, S), weights (B, S, S)) of the greedy tests: B seeded
    orders; ``start`` "zero" or "rounded": fm.inputs' soft, saturated and
    coin-flip weights rounded at 0.5, cycled, on each order's permissible pairs
    (its all-0 evaluation is the zero start; from all ones the search walks
    through runs of near-ties below 1e-10, whatever the seed)."""
    m = fm.get_model(GREEDY_MODEL)
    rng = np.random.default_rng(GREEDY_SEED)
    perms = [rng.permutation(m.S) for _ in range(GREEDY_B)]
    pos = np.empty((GREEDY_B, m.S), dtype=np.int32)
    for k, p in enumerate(perms):
        pos[k, p] = np.arange(m.S)
    w = np.zeros((GREEDY_B, m.S, m.S))
    if start == "rounded":
        w01 = fm.inputs(m.S)[2][[0, 1, 5, 6, 7, 8]]
        for k, p in enumerate(perms):
            w[k] = np.round(w01[k % len(w01)]) * permissible(p)
    return m, pos, w
