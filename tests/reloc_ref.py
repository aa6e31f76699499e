"""Long-double reference, tolerance and inputs for the exact score change of
every single-node relocation of an order (nemo_score_relocations,
csrc/nemo_reloc.hip).

The state is (order, W) with a FULL weight matrix: W[i][j] is the weight pair
(i, j) carries whenever j precedes i.  With cell[i][e] = U[i][e] + sum_{j before
i} log f_ij(e), f_ij = 1 - w_ij + w_ij v_ij, v = exp(T[i][j][e]), z = cell - cs,
ow = exp(z) and ll = sum_e cs[e], moving node a from position p to position q
changes only these rows of the cells: for q > p the nodes m at positions p+1 ..
q lose parent a and a gains them all; for q < p the nodes m at q .. p-1 gain
parent a and a loses them all.  So

    ll(a moved to q) - ll = sum_e log(1 + X_aq(e)),
    q > p:  X = -ow[a] + sum_m ow[m] (1 / f_ma - 1) + exp(y),  y = z_a + sum_m log f_am
    q < p:  X = -ow[a] + sum_m ow[m] (f_ma - 1)     + exp(y),  y = z_a - sum_m log f_am

and dll[a][q] holds it by NODE a and target POSITION q, 0 at q = pos[a].  The
reference starts from ``fixed_point_models.reference(..., full=True)`` and forms
1 + X in long double from positive terms only (the other rows' order weights,
ow[m] / f_ma or ow[m] f_ma, and exp(y)), so nothing cancels;
tests/test_reloc_cpu.py checks the closed form against brute-force rescoring of
every relocated order.

Tolerance per entry, derived as moves_ref derives tol_ij.  Per effect, with c_m =
1 / f_ma - 1 or f_ma - 1, P = ow[a] + sum_m ow[m] |c_m| (the sum's terms), Y =
exp(y) and t = log(1 + X):

    tol_aq = 4 [ sum_e ( (tc P + (tc + ty) Y) / (1 + X) )
                 + (E + 64) 2^-52 sum_e |t_e|
                 + 8 2^-52 sum_e max(|t_e|, 0.5 if |X_e| >= 2^-8 else 0)
                 + sum_e FLUSH (1 + sum_m |c_m|) / (1 + X) ]
    tc = 2 tol_cell(S - 1, big) + 8 2^-52
    ty = 2^-52 ( 8 + sum_m (8 + 4 |log f_am|) + k max(|z_a|, max_j |y_j|) )

An error d of a cell or of cs is a relative error d of ow and of exp(y) (2
tol_cell); a factor c_m -- a product, a difference and a quotient of the staged
exp(T) -- carries a few ulp more (8 2^-52).  The exponent y is a SUM OF LOGS: each
log f_am comes from the device's log routine with an absolute error of an ulp of
max(|log f|, 0.5), and each of the k additions rounds at the running sum's
magnitude, which is ty, a relative error of exp(y); the 8 in front is the table
exponential.  A relative error of a term moves log(1 + X) by |term| / (1 + X)
times it.  (E + 64) 2^-52 covers the sum over E and the third term the device's
log1p routine (relative below 2^-8, log_fast's absolute ulp of max(|t|, 0.5)
from there on).  FLUSH = 2^-1022: an order weight or exp(-|y|) below the
smallest normal may flush to 0, which loses at most that much of a term of the
sum (times |c_m|) or of 1 + X's rest.  The factor 4 covers the kernels' table
exponential and summation order, as in score_grad_ref.

Where 1 + X has no correct digit in fp64 the tolerance is astronomically wide and
only a finite value is asked: a saturated node (ow[a] rounds to 1, so 1 - ow[a]
rounds to 0) that gains parents against a table past -37 per factor has 1 + X =
(rest) + exp(y) with both below the rounding of ow[a]; the first term, P / (1 +
X), says so, and such an entry's tolerance is clipped at 1e300 to stay a finite
fp64 number.  A plain numpy fp64 restatement in the device's log form stays
within a half of the tolerance on every input below (tests/test_reloc_cpu.py).

No GPU and no library here.
"""
from __future__ import annotations

import functools
import itertools
from dataclasses import dataclass

import numpy as np

import fixed_point_models as fm
import stream_models as sm
from score_grad_ref import (GENERIC, PART_MODEL, WIDE_MODEL, factored_inputs, generic_inputs,  # noqa: F401
                            get_model as _grad_model)

LD = np.longdouble
EPS52 = 2.0 ** -52
SMALL = 2.0 ** -8
FLUSH = 2.0 ** -1022
TOL_CLIP = 1e300
EXP_MAX = 709.0          # log of the largest fp64: past it exp(y) leaves fp64

# ---- the cases -----------------------------------------------------------------
SPAD_EDGES = ("nem04-S16-E40", "small-S15-E16", "small-S17-E16", "nem04-S33-E40", "nem04-S60-E40", "nem04-S64-E40")
TILE_EDGES = tuple(f"small-S17-E{e}" for e in (1, 15, 16, 17, 63, 64, 65))
LADDER_S64 = tuple(f"nem{k:02d}-S64-E40" for k in (0, 4, 8, 12))
TABLES = ("table-mixed-S16-E40", "table-deep-S8-E40", "table-edge-S8-E40")
OVERFLOW_MODEL = "up-S8-E40"     # table-deep's mirror: six parents at +120, so y passes +709 (see _up_model)
BRUTE = ("small-S2-E17", "small-S15-E16", "nem08-S16-E40", "table-deep-S8-E40", "f64-own-S9-E64-a70")
RESCORE = ("nem08-S16-E40", "small-S17-E65")


def factored_ids():
    """The factored models with S <= 64 (each run on auto and under reloc_path 1)."""
    ids = ("small-S2-E17",) + SPAD_EDGES + TILE_EDGES + (PART_MODEL,) + LADDER_S64 + TABLES + (OVERFLOW_MODEL,)
    return list(dict.fromkeys(ids + RESCORE))


def _up_model(s=8, e=40):
    """table-deep mirrored: six parents whose table sits at +120 (+120.5 where the
    bit is set).  A node that gains them at weight 1 has y = z_a + sum log f near
    +720, past the largest fp64 exponent: exp(y) would overflow, the log form must not."""
    rng = np.random.default_rng(1000 + s)
    a, b = rng.uniform(-0.2, 0.2, s), rng.uniform(-0.2, 0.2, s)
    lo = rng.uniform(-1, 1, s)
    lo[:6] = 120.0
    m = fm._table_model(OVERFLOW_MODEL, s, e, lo, lo + 0.5, a, b, s)
    return m


@functools.lru_cache(maxsize=4)
def get_model(name) -> fm.Model:
    if name == OVERFLOW_MODEL:
        return _up_model()
    return _grad_model(name)


def full_weights(w01, perms, tag):
    """Full weight matrices (n, S, S) from the generators' soft, saturated, all-0,
    all-1 and coin-flip ones: every third evaluation keeps the generator's own
    matrix at every entry (all ones stays all ones: the widest log range), the
    others have their non-permissible entries filled from a seed: uniform, a
    quarter 0, a quarter 1.  The diagonal is never read; it is left as it is."""
    base = sum(ord(ch) * (k + 1) for k, ch in enumerate(tag)) % 100003
    out = np.array(w01, dtype=np.float64)
    for k, perm in enumerate(perms):
        if k % 3 == 2:
            continue
        rng = np.random.default_rng(9000 + 131 * base + k)
        s = len(perm)
        pos = np.empty(s, dtype=np.int64)
        pos[np.asarray(perm)] = np.arange(s)
        fill = rng.random((s, s))
        r = rng.random((s, s))
        fill[r < 0.25] = 0.0
        fill[(r >= 0.25) & (r < 0.5)] = 1.0
        off = pos[:, None] < pos[None, :]        # j after i: not permissible now
        out[k][off] = fill[off]
    return np.ascontiguousarray(out)


@functools.lru_cache(maxsize=None)
def factored_case(name):
    """(model, perms, pos, w (n, S, S) full) of a factored model."""
    m = get_model(name)
    perms, pos, w01 = fm.inputs(m.S)
    w = full_weights(w01, perms, name)
    if name == OVERFLOW_MODEL:
        # one more evaluation: the reverse order with weight 0 on every permissible pair
        # (every cell is its U, cs is of order 1) and weight 1 on every other pair, so the
        # first node, moved to the end, gains the six parents at +120: y = z_a + 720
        rev = np.arange(m.S)[::-1].copy()
        perms = list(perms) + [rev]
        pos = np.vstack([pos, np.argsort(rev).astype(np.int32)[None]])
        extra = (np.argsort(rev)[:, None] < np.argsort(rev)[None, :]).astype(np.float64)
        w = np.concatenate([w, extra[None]])
    return m, perms, np.ascontiguousarray(pos), np.ascontiguousarray(w)


@functools.lru_cache(maxsize=None)
def generic_case(name):
    """(case, U, T, perms, pos, w full) of one of stream_models' cases."""
    c, u, t, perms, pos, w01 = generic_inputs(name)
    return c, u, t, perms, pos, full_weights(w01, perms, name)


def apply_relocation(perm, a, q):
    """The order (node by position) after node a moves to position q."""
    rest = [int(x) for x in perm if x != a]
    rest.insert(int(q), int(a))
    return np.asarray(rest)


# ---- the reference -------------------------------------------------------------
@dataclass
class RelocRef:
    ll: float
    cs: np.ndarray       # (E,) long double
    dll: np.ndarray      # (S, S) long double by [node a][target position q], 0 at q = pos[a]
    tol: np.ndarray      # (S, S) float64 (0 at q = pos[a])
    tol_ll: float
    ymax: float          # the largest and
    ymin: float          # the smallest y = z_a +- sum log f over (a, q, e)


def reloc_reference(u, t, perm, w, et=None, full=None) -> RelocRef:
    """The long-double relocation scores of one evaluation and their tolerance.
    ``et``: exp(T) in long double; ``full``: fm.reference(..., full=True) at cap 0."""
    s, e = t.shape[0], t.shape[2]
    perm = np.asarray(perm)
    ll, cs, cells, ow = full if full is not None else fm.reference(u, t, perm, w, 0, full=True, et=et)
    if et is None:
        et = np.exp(t.astype(LD))
    big = float(np.abs(cells[np.isfinite(cells)]).max())
    one = LD(1)
    wl = np.asarray(w, dtype=LD)
    dll = np.zeros((s, s), dtype=LD)
    tol = np.zeros((s, s))
    tc = LD(2.0 * sm.tol_cell(s - 1, big) + 8.0 * EPS52)
    ymax, ymin = -np.inf, np.inf
    for p in range(s):
        a = perm[p]
        za = cells[a] - cs
        for up in (True, False):
            ms = perm[p + 1:] if up else perm[:p][::-1]
            if not ms.size:
                continue
            wma = wl[ms, a][:, None]
            wam = wl[a, ms][:, None]
            fma = one - wma + wma * et[ms, a]           # (k, E)
            fam = one - wam + wam * et[a, ms]
            lf = np.log(fam)
            dma = wma * (et[ms, a] - one)               # f_ma - 1
            c = -dma / fma if up else dma               # 1 / f_ma - 1 or f_ma - 1
            newm = ow[ms] / fma if up else ow[ms] * fma  # the rows of the m after the move, over exp(cs)
            y = za[None] + np.cumsum(lf if up else -lf, axis=0)
            # the untouched rows (the null row and the other side of p, then the m not yet
            # reached) plus the moved rows: positive terms only
            other = np.setdiff1d(np.arange(s + 1), np.append(ms, a))
            back = np.cumsum(ow[ms][::-1], axis=0)[::-1]
            tail = np.concatenate([back[1:], np.zeros((1, e), dtype=LD)])
            rest = ow[other].sum(axis=0)[None] + tail + np.cumsum(newm, axis=0)
            # log(rest + exp(y)) without an overflow of exp, and X for the small branch
            ypos = y > 0
            ey = np.exp(-np.abs(y))
            logt = np.where(ypos, y + np.log1p(np.where(ypos, rest * ey, 0)),
                            np.log(np.where(ypos, one, rest + ey)))
            x = np.cumsum(ow[ms] * c, axis=0) + ow[a][None] * np.expm1(y - za[None])
            small = np.abs(x) < SMALL
            tt = np.where(small, np.log1p(np.where(small, x, 0)), logt)
            qs = p + 1 + np.arange(ms.size) if up else p - 1 - np.arange(ms.size)
            dll[a, qs] = tt.sum(axis=1)
            # ---- the tolerance
            at = np.abs(tt)
            psum = ow[a][None] + np.cumsum(ow[ms] * np.abs(c), axis=0)
            steps = (1 + np.arange(ms.size))[:, None]
            ybig = np.maximum(np.abs(za)[None], np.maximum.accumulate(np.abs(y), axis=0))
            ty = EPS52 * (8.0 + np.cumsum(8.0 + 4.0 * np.abs(lf), axis=0) + steps * ybig)
            yrel = np.exp(y - logt)                      # exp(y) / (1 + X) <= 1
            inv = np.exp(-logt)                          # 1 / (1 + X)
            first = tc * psum * inv + (tc + ty) * yrel
            rout = np.maximum(at, np.where(small, LD(0), LD(0.5)))
            flush = FLUSH * (one + np.cumsum(np.abs(c), axis=0)) * inv
            tq = 4.0 * (first.sum(axis=1) + (e + 64) * EPS52 * at.sum(axis=1) + 8.0 * EPS52 * rout.sum(axis=1)
                        + flush.sum(axis=1))
            tol[a, qs] = np.minimum(tq, LD(TOL_CLIP)).astype(np.float64)
            ymax, ymin = max(ymax, float(y.max())), min(ymin, float(y.min()))
    tll = sm.tol_ll(cs, sm.tol_cell(s - 1, big))
    return RelocRef(float(ll), cs, dll, tol, tll, ymax, ymin)


@functools.lru_cache(maxsize=None)
def factored_refs(name):
    """RelocRef of every evaluation of a factored model, computed once."""
    m, perms, _, w = factored_case(name)
    et = np.exp(m.T.astype(LD))
    return [reloc_reference(m.U, m.T, p, wk, et=et) for p, wk in zip(perms, w)]


@functools.lru_cache(maxsize=None)
def generic_refs(name):
    """The same for one of stream_models' cases."""
    c, u, t, perms, _, w = generic_case(name)
    et = sm._exp_table(name)
    return [reloc_reference(u, t, perms[k], w[k], et=et) for k in range(len(perms))]


# ---- a plain fp64 restatement in the device's log form ------------------------------
def reloc_numpy(u, t, perm, w):
    """(ll, dll (S, S) by [node][target position]) in numpy fp64: the forward of
    score_grad_ref.grad_numpy, then per node the two walks -- the running sum
    -ow[a] + sum ow[m] c_m, the running exponent y = z_a +- sum log f_am, and
    log(1 + X) as log1p(sum + e^y) for y <= 0, y + log1p((1 + sum) e^-y) past it."""
    s = t.shape[0]
    perm = np.asarray(perm)
    w = np.asarray(w, dtype=np.float64)
    v = np.exp(t)
    cell = np.array(u, dtype=np.float64)
    for p in range(1, s):
        i, pa = perm[p], perm[:p]
        wi = w[i, pa][:, None]
        cell[i] += np.log((1.0 - wi) + wi * v[i, pa]).sum(axis=0)
    mx = cell.max(axis=0)
    cs = mx + np.log(np.exp(cell - mx).sum(axis=0))
    z = cell - cs
    ow = np.exp(z)
    dll = np.zeros((s, s))
    for p in range(s):
        a = perm[p]
        for up in (True, False):
            ms = perm[p + 1:] if up else perm[:p][::-1]
            if not ms.size:
                continue
            wma, wam = w[ms, a][:, None], w[a, ms][:, None]
            d = wma * (v[ms, a] - 1.0)
            c = -d / ((1.0 - wma) + wma * v[ms, a]) if up else d
            lf = np.log((1.0 - wam) + wam * v[a, ms])
            sumv = -ow[a][None] + np.cumsum(ow[ms] * c, axis=0)
            y = z[a][None] + np.cumsum(lf if up else -lf, axis=0)
            ey = np.exp(-np.abs(y))
            x = np.where(y > 0.0, (1.0 + sumv) * ey, sumv + ey)
            small = np.abs(x) < SMALL
            r = np.where(small, np.log1p(np.where(small, x, 0.0)), np.log(np.maximum(1.0 + x, 2.0 ** -54)))
            tt = np.where(y > 0.0, y + r, r)
            qs = p + 1 + np.arange(ms.size) if up else p - 1 - np.arange(ms.size)
            dll[a, qs] = tt.sum(axis=1)
    return float(cs.sum()), dll


class NumpyEngine:
    """``Engine.score_relocations`` on the CPU through reloc_numpy: what a
    pure-numpy greedy search or Gibbs sampler over orders is driven by."""

    def __init__(self, u, t):
        self.U, self.T = np.asarray(u, dtype=np.float64), np.asarray(t, dtype=np.float64)
        self.S, self.E = self.T.shape[0], self.T.shape[2]
        self.calls = []      # the pos of every call

    def score_relocations(self, pos, w01, cap=0):
        pos = np.atleast_2d(pos)
        assert cap == 0 or cap >= self.S - 1
        self.calls.append(np.array(pos))
        ll = np.empty(len(pos))
        dll = np.empty((len(pos), self.S, self.S))
        for k, pk in enumerate(pos):
            ll[k], dll[k] = reloc_numpy(self.U, self.T, np.argsort(pk), w01[k])
        return ll, dll


def numpy_greedy(eng, pos, weights, max_iter=None, min_gain=1e-9):
    """The hill-climb written out problem by problem: -> (pos, moves, margins);
    moves[k] the (a, q) sequence of problem k, margins[k] each step's best gain
    minus the second best (and, at the last call, min_gain minus the best: how
    clearly the search stopped)."""
    pos = np.array(np.atleast_2d(pos), dtype=np.int32)
    b, s = pos.shape
    moves, margins = [], []
    for k in range(b):
        mv, mg = [], []
        for _ in range(s * s if max_iter is None else max_iter):
            _, dll = eng.score_relocations(pos[k:k + 1], weights[k:k + 1])
            gain = dll[0].ravel()
            order = np.argsort(-gain, kind="stable")
            if not gain[order[0]] > min_gain:
                # (the entries q = pos[a] are exactly 0 on every engine: the best REAL relocation counts)
                real = np.delete(dll[0], np.arange(s) * s + pos[k])
                mg.append(min_gain - real.max())
                break
            a, q = divmod(int(order[0]), s)
            # an adjacent transposition is one neighbour reached by two (a, q): the runner-up is the next OTHER order
            perm = np.argsort(pos[k])
            twin = (int(perm[q]), int(pos[k, a])) if abs(q - int(pos[k, a])) == 1 else None
            second = next(g for i, g in ((int(i), gain[i]) for i in order[1:]) if divmod(i, s) != twin)
            mg.append(gain[order[0]] - max(second, min_gain))
            perm = apply_relocation(perm, a, q)
            pos[k, perm] = np.arange(s)
            mv.append((a, q))
        moves.append(mv)
        margins.append(mg)
    return pos, moves, margins


def moves_of(calls):
    """The sequence of orders (pos tuples) every problem stepped through, from the
    pos of successive calls.  Orders, not (a, q): an adjacent transposition is ONE
    neighbour reached by two (a, q) whose gains agree only to rounding."""
    b = calls[0].shape[0]
    seq = [[] for _ in range(b)]
    for prev, cur in zip(calls, calls[1:]):
        for k in range(b):
            if not np.array_equal(prev[k], cur[k]):
                seq[k].append(tuple(int(x) for x in cur[k]))
    return seq


# the greedy tests' model, batch and seed: tests/test_reloc_cpu.py asserts that on
# the CPU every step's best gain clears the best gain of any OTHER order (and the
# stop clears min_gain) by more than GREEDY_MARGIN, so a device within tolerance
# reaches the same orders step by step
GREEDY_MODEL = "nem04-S16-E40"
GREEDY_B = 7
GREEDY_SEED = 3
GREEDY_MARGIN = 1e-9


def greedy_inputs():
    """(model, pos (B, S), weights (B, S, S) full): B seeded orders, each with a
    seeded soft full weight matrix in (0.02, 0.98).  (Weights of exactly 0 or 1
    make different orders score exactly alike -- a node moved past a neighbour it
    shares no weight with -- and a tie's winner is decided by rounding.)"""
    m = fm.get_model(GREEDY_MODEL)
    rng = np.random.default_rng(GREEDY_SEED)
    perms = [rng.permutation(m.S) for _ in range(GREEDY_B)]
    pos = np.empty((GREEDY_B, m.S), dtype=np.int32)
    for k, p in enumerate(perms):
        pos[k, p] = np.arange(m.S)
    w = rng.uniform(0.02, 0.98, (GREEDY_B, m.S, m.S))
    return m, pos, np.ascontiguousarray(w)


# ---- the Gibbs tests' model: S = 4, E = 12, its 24 orders enumerated ----------------
GIBBS_SEED = 11
GIBBS_CHAINS = 48
GIBBS_SWEEPS = 40
GIBBS_BURN = 8


@functools.lru_cache(maxsize=None)
def gibbs_model():
    """(U (5, 12), T (4, 4, 12) two-valued rows, W (4, 4) full) of the Gibbs tests."""
    rng = np.random.default_rng(77)
    s, e = 4, 12
    lo = rng.uniform(-1.5, 0.5, s)
    hi = lo + rng.choice([-1.0, 1.0], s) * rng.uniform(0.3, 0.8, s)
    bits = rng.random((s, e)) < 0.45
    bits[:, 0] = False
    t = np.empty((s, s, e))
    t[:] = np.where(bits, hi[:, None], lo[:, None])[None]
    u = rng.normal(-1.0, 0.4, (s + 1, e))
    w = rng.uniform(0.1, 0.9, (s, s))
    return u, t, w


@functools.lru_cache(maxsize=None)
def gibbs_enumeration(beta=1.0):
    """P(j precedes i) (4, 4) under the posterior proportional to exp(beta ll(order))
    over the 24 orders, in long double."""
    u, t, w = gibbs_model()
    perms = [np.asarray(p) for p in itertools.permutations(range(4))]
    lls = np.array([LD(fm.reference(u, t, p, w, 0, full=True)[1].sum()) for p in perms], dtype=LD)
    pr = np.exp(LD(beta) * (lls - lls.max()))
    pr /= pr.sum()
    before = np.zeros((4, 4), dtype=LD)
    for p, x in zip(perms, pr):
        pos = np.argsort(p)
        before += x * (pos[None, :] < pos[:, None])
    return before.astype(np.float64)


def gibbs_z(before, exact):
    """The worst z-score of the chains' mean marginals against the enumeration:
    |mean over chains - exact| / (std over chains / sqrt(B)), off the diagonal."""
    b = before.shape[0]
    mean = before.mean(axis=0)
    se = before.std(axis=0, ddof=1) / np.sqrt(b)
    off = ~np.eye(before.shape[1], dtype=bool)
    return float((np.abs(mean - exact)[off] / se[off]).max())
