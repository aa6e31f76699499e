"""Long-double reference, tolerance, decision margins and a numpy fp64 restatement
for relocations walked in sequence (nemo_order_sweep, csrc/nemo_order_sweep.hip).

A sweep is a list of visits.  Visit k takes node a = visit[k] at its position p in
the order HELD, scores its S positions (reloc_ref's closed form, here for the one
visited node: ``row_reference``), chooses q* (a Gibbs draw from the uniform u[k] by
inverse CDF over exp(beta row), positions ascending; or, beta = inf, the largest
gain above min_gain, ties to the lowest position) and moves a there.  The reference
holds no drifting state: after a move it scores the new order from scratch in long
double (fixed_point_models.reference), so its row at every visit is the exact row
of the order held and its ll the exact score.

Tolerance of a visit's row.  The device carries the cells across the moves: a move
adds -+log f_ma to each passed node's row of cells and +-log f_am, step by step, to
a's row, and forms cs afresh from the updated column.  Each such add rounds at the
running cell's magnitude (2^-53 |cell|) and its addend comes from the device's log
routine with an absolute error of an ulp of max(|log f|, 0.5), so an add applied to
a row contributes at most

    2^-52 (running |cell| + max(|log f|, 0.5))

to that row's error, and these add up over the adds applied to the row so far:
``drift[i]``, kept per row of cells (the null row never moves: 0).  A fresh cs is a
log-sum-exp of the drifted column, a convex combination in the cells, so it moves
by at most the largest drift of the column's rows on top of its own rounding (which
tol_cell covers).  reloc_ref's tolerance takes an error d of a cell or of cs as a
relative error d of an order weight and of exp(y): its cell term tc = 2 tol_cell + 8
2^-52 becomes

    tc = 2 (tol_cell(S - 1, big) + max_i drift[i]) + 8 2^-52

and everything else in tol_aq stands as derived there.  ll after a visit: tol_ll of
the held order with the same widened cell tolerance.

Decision margins.  Gibbs: the draw lands on q* = #{q : cdf[q] < u total}; a device
row within tol of the reference's moves pq[q] = exp(beta r[q] - max) by a relative
beta tol[q] (twice: the maximum moves too) plus the exp and the sum's roundings (16
2^-52), so the comparison at q is safe when

    |cdf[q] - u total| > 2 (sum_{q' <= q} pq (beta tol + 16 2^-52) + u (the same sum over all q'))

and the visit's margin is the least slack over q < S - 1.  Greedy: the best gain
minus the second best, and the best against min_gain, each minus twice the
tolerances involved.

No GPU and no library here.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import fixed_point_models as fm
import reloc_ref as rr
import stream_models as sm

LD = np.longdouble
EPS52 = rr.EPS52
SMALL = rr.SMALL
FLUSH = rr.FLUSH


def row_reference(full, et, perm, wl, a, tc):
    """reloc_ref.reloc_reference's row of node ``a`` alone at the order ``perm``:
    -> (row (S,) long double by target position, tol (S,) float64), 0 at a's own
    position.  ``full``: fm.reference(..., full=True) of the order; ``tc``: the cell
    term of the tolerance."""
    _, cs, cells, ow = full
    perm = np.asarray(perm)
    s, e = len(perm), cs.shape[0]
    p = int(np.nonzero(perm == a)[0][0])
    one = LD(1)
    tc = LD(tc)
    row = np.zeros(s, dtype=LD)
    tol = np.zeros(s)
    za = cells[a] - cs
    for up in (True, False):
        ms = perm[p + 1:] if up else perm[:p][::-1]
        if not ms.size:
            continue
        wma = wl[ms, a][:, None]
        wam = wl[a, ms][:, None]
        fma = one - wma + wma * et[ms, a]
        fam = one - wam + wam * et[a, ms]
        lf = np.log(fam)
        dma = wma * (et[ms, a] - one)
        c = -dma / fma if up else dma
        newm = ow[ms] / fma if up else ow[ms] * fma
        y = za[None] + np.cumsum(lf if up else -lf, axis=0)
        other = np.setdiff1d(np.arange(s + 1), np.append(ms, a))
        back = np.cumsum(ow[ms][::-1], axis=0)[::-1]
        tail = np.concatenate([back[1:], np.zeros((1, e), dtype=LD)])
        rest = ow[other].sum(axis=0)[None] + tail + np.cumsum(newm, axis=0)
        ypos = y > 0
        ey = np.exp(-np.abs(y))
        logt = np.where(ypos, y + np.log1p(np.where(ypos, rest * ey, 0)), np.log(np.where(ypos, one, rest + ey)))
        x = np.cumsum(ow[ms] * c, axis=0) + ow[a][None] * np.expm1(y - za[None])
        small = np.abs(x) < SMALL
        tt = np.where(small, np.log1p(np.where(small, x, 0)), logt)
        qs = p + 1 + np.arange(ms.size) if up else p - 1 - np.arange(ms.size)
        row[qs] = tt.sum(axis=1)
        at = np.abs(tt)
        psum = ow[a][None] + np.cumsum(ow[ms] * np.abs(c), axis=0)
        steps = (1 + np.arange(ms.size))[:, None]
        ybig = np.maximum(np.abs(za)[None], np.maximum.accumulate(np.abs(y), axis=0))
        ty = EPS52 * (8.0 + np.cumsum(8.0 + 4.0 * np.abs(lf), axis=0) + steps * ybig)
        yrel = np.exp(y - logt)
        inv = np.exp(-logt)
        first = tc * psum * inv + (tc + ty) * yrel
        rout = np.maximum(at, np.where(small, LD(0), LD(0.5)))
        flush = FLUSH * (one + np.cumsum(np.abs(c), axis=0)) * inv
        tq = 4.0 * (first.sum(axis=1) + (e + 64) * EPS52 * at.sum(axis=1) + 8.0 * EPS52 * rout.sum(axis=1)
                    + flush.sum(axis=1))
        tol[qs] = np.minimum(tq, LD(rr.TOL_CLIP)).astype(np.float64)
    return row, tol


def gibbs_draw(row, u, beta, xp=np.float64):
    """(q*, pq, cdf): gibbs_orders' rule on one row."""
    g = xp(beta) * np.asarray(row, dtype=xp)
    pq = np.exp(g - g.max())
    cdf = np.cumsum(pq)
    q = min(int((cdf < xp(u) * cdf[-1]).sum()), len(pq) - 1)
    return q, pq, cdf


def gibbs_margin(row, tol, u, beta):
    """The least slack of the draw's comparisons (module docstring), as a fraction
    of the CDF total; the long-double row decides."""
    _, pq, cdf = gibbs_draw(row, u, beta, LD)
    err = np.cumsum(pq * (LD(beta) * np.asarray(tol, dtype=LD) + 16.0 * EPS52))
    slack = np.abs(cdf - LD(u) * cdf[-1]) - 2.0 * (err + LD(u) * err[-1])
    return float((slack[:-1] / cdf[-1]).min()) if len(pq) > 1 else np.inf


def greedy_pick(row, p, min_gain):
    """(q*, best): the largest entry, ties to the lowest position, taken only above min_gain."""
    row = np.asarray(row)
    best = int(np.argmax(row))
    return (best if row[best] > min_gain else p), best


def decide(row, p, u, beta, min_gain):
    """The device's decision on one fp64 row: a row that holds a NaN, or whose CDF total is not a
    number (an infinite entry: inf - inf), leaves the node at p; else the greedy pick (beta = inf) or
    the Gibbs draw.  Always within [0, S - 1]."""
    row = np.asarray(row, dtype=np.float64)
    if np.isnan(row).any():
        return int(p)
    if np.isinf(beta):
        return int(greedy_pick(row, p, min_gain)[0])
    with np.errstate(invalid="ignore"):
        q, _, cdf = gibbs_draw(row, u, beta)
    return int(p) if np.isnan(cdf[-1]) else int(q)


def greedy_margin(row, tol, p, min_gain):
    """A move taken: the best gain minus the second best and minus min_gain; nothing
    taken: min_gain minus every real relocation's gain; each minus twice the
    tolerances involved."""
    row = np.asarray(row, dtype=LD)
    tol = np.asarray(tol, dtype=np.float64)
    real = np.delete(np.arange(len(row)), p)
    if not real.size:
        return np.inf
    br = int(real[np.argmax(row[real])])
    if not row[br] > min_gain:
        return float((min_gain - row[real] - 2.0 * tol[real]).min())
    rest = real[real != br]
    m = float(row[br]) - min_gain - 2.0 * tol[br]
    if rest.size:
        m = min(m, float((row[br] - row[rest] - 2.0 * (tol[br] + tol[rest])).min()))
    return m


@dataclass
class SweepRef:
    rows: np.ndarray      # (nvisit, S) long double
    tols: np.ndarray      # (nvisit, S) float64, 0 at the visited node's position
    p: np.ndarray         # (nvisit,) the visited node's position before the visit
    q: np.ndarray         # (nvisit,) the position taken
    perms: list           # nvisit + 1 orders (node by position)
    ll: np.ndarray        # (nvisit + 1,) long double: the initial score, then after every visit
    tol_ll: np.ndarray    # (nvisit + 1,)
    drift: np.ndarray     # (nvisit + 1,) the largest drift of a row of cells
    margin: np.ndarray    # (nvisit,)
    nmoved: int


def sweep_reference(u, t, perm, w, visit, us=None, beta=1.0, min_gain=0.0, et=None) -> SweepRef:
    """The long-double sweep of one evaluation (module docstring)."""
    s = t.shape[0]
    if et is None:
        et = np.exp(t.astype(LD))
    wl = np.asarray(w, dtype=LD)
    one = LD(1)
    perm = np.asarray(perm).copy()
    full = fm.reference(u, t, perm, w, 0, full=True, et=et)
    drift = np.zeros(s + 1)
    greedy = np.isinf(beta)

    def cell_tol():
        big = float(np.abs(full[2][np.isfinite(full[2])]).max())
        return sm.tol_cell(s - 1, big) + float(drift.max())

    nv = len(visit)
    out = SweepRef(np.zeros((nv, s), dtype=LD), np.zeros((nv, s)), np.zeros(nv, dtype=np.int64),
                   np.zeros(nv, dtype=np.int64), [perm.copy()], np.zeros(nv + 1, dtype=LD), np.zeros(nv + 1),
                   np.zeros(nv + 1), np.zeros(nv), 0)
    out.ll[0], out.tol_ll[0] = full[1].sum(), sm.tol_ll(full[1], cell_tol())
    for k, a in enumerate(int(x) for x in visit):
        p = int(np.nonzero(perm == a)[0][0])
        row, tol = row_reference(full, et, perm, wl, a, 2.0 * cell_tol() + 8.0 * EPS52)
        if greedy:
            q, _ = greedy_pick(row, p, min_gain)
            out.margin[k] = greedy_margin(row, tol, p, min_gain)
        else:
            q, _, _ = gibbs_draw(row, us[k], beta, LD)
            out.margin[k] = gibbs_margin(row, tol, us[k], beta)
        out.rows[k], out.tols[k], out.p[k], out.q[k] = row, tol, p, q
        if q != p:
            up = q > p
            ms = perm[p + 1:q + 1] if up else perm[q:p][::-1]
            old = full[2]
            perm = rr.apply_relocation(perm, a, q)
            full = fm.reference(u, t, perm, w, 0, full=True, et=et)
            new = full[2]
            run = old[a].copy()
            for m in ms:
                lm = np.log(one - wl[m, a] + wl[m, a] * et[m, a])
                lf = np.log(one - wl[a, m] + wl[a, m] * et[a, m])
                drift[m] += EPS52 * (max(float(np.abs(old[m]).max()), float(np.abs(new[m]).max()))
                                     + max(float(np.abs(lm).max()), 0.5))
                nxt = run + (lf if up else -lf)
                drift[a] += EPS52 * (max(float(np.abs(run).max()), float(np.abs(nxt).max()))
                                     + max(float(np.abs(lf).max()), 0.5))
                run = nxt
            out.nmoved += 1
        out.perms.append(perm.copy())
        out.ll[k + 1], out.tol_ll[k + 1], out.drift[k + 1] = full[1].sum(), sm.tol_ll(full[1], cell_tol()), drift.max()
    return out


# ---- a plain fp64 restatement in the device's form -----------------------------------
def _lse(cell):
    mx = cell.max(axis=0)
    return mx + np.log(np.exp(cell - mx).sum(axis=0))


def sweep_numpy(u, t, perm, w, visit, us=None, beta=1.0, min_gain=0.0):
    """-> (pos_out (S,), ll0, ll, q (nv,), dll (nv, S), ll_vis (nv,), nmoved) in numpy
    fp64 with the device's state: the forward's cells and cs, per visit the two walks
    of reloc_ref.reloc_numpy for the visited node at the CURRENT cells, the decision,
    and on a move the cells updated add by add and cs formed afresh."""
    s = t.shape[0]
    perm = np.asarray(perm).copy()
    w = np.asarray(w, dtype=np.float64)
    v = np.exp(np.asarray(t, dtype=np.float64))
    cell = np.array(u, dtype=np.float64)
    for p in range(1, s):
        i, pa = perm[p], perm[:p]
        wi = w[i, pa][:, None]
        cell[i] += np.log((1.0 - wi) + wi * v[i, pa]).sum(axis=0)
    cs = _lse(cell)
    ll0 = ll = float(cs.sum())
    nv = len(visit)
    qo, dll, vis = np.zeros(nv, dtype=np.int32), np.zeros((nv, s)), np.zeros(nv)
    nmoved = 0
    greedy = np.isinf(beta)
    for k, a in enumerate(int(x) for x in visit):
        p = int(np.nonzero(perm == a)[0][0])
        z = cell - cs
        ow = np.exp(z)
        row = np.zeros(s)
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
            row[qs] = tt.sum(axis=1)
        dll[k] = row
        q = decide(row, p, None if greedy else us[k], beta, min_gain)
        if q != p:
            up = q > p
            for m in (perm[p + 1:q + 1] if up else perm[q:p][::-1]):
                lm = np.log((1.0 - w[m, a]) + w[m, a] * v[m, a])
                lf = np.log((1.0 - w[a, m]) + w[a, m] * v[a, m])
                cell[m] += -lm if up else lm
                cell[a] += lf if up else -lf
            cs = _lse(cell)
            ll = float(cs.sum())
            perm = rr.apply_relocation(perm, a, q)
            nmoved += 1
        qo[k], vis[k] = q, ll
    return np.argsort(perm).astype(np.int32), ll0, ll, qo, dll, vis, nmoved


class NumpyEngine(rr.NumpyEngine):
    """``Engine.order_sweep`` (and ``score_relocations``) on the CPU."""

    def order_sweep(self, pos, w01, visit, u=None, beta=1.0, min_gain=0.0, cap=0):
        pos = np.atleast_2d(pos)
        assert cap == 0 or cap >= self.S - 1
        b = len(pos)
        visit = np.asarray(visit).reshape(b, -1) if np.asarray(visit).size else np.zeros((b, 0), dtype=np.int32)
        self.sweeps = getattr(self, "sweeps", 0) + 1
        outs = [sweep_numpy(self.U, self.T, np.argsort(pos[k]), w01[k], visit[k], None if u is None else u[k], beta,
                            min_gain) for k in range(b)]
        return (np.stack([o[0] for o in outs]), np.array([o[1] for o in outs]), np.array([o[2] for o in outs]),
                np.stack([o[3] for o in outs]), np.stack([o[4] for o in outs]), np.stack([o[5] for o in outs]),
                np.array([o[6] for o in outs], dtype=np.int32))


# ---- the inputs ------------------------------------------------------------------------
U_SEED = 5
MARGINED = ("small-S2-E17", "nem04-S16-E40", "small-S17-E65", "nem04-S33-E40", "table-mixed-S16-E40",
            "table-deep-S8-E40", "nem08-S64-E40")
MARGINED_EVALS = (0, 1, 5)            # of fm.inputs (S = 64: evaluation 0 alone)
FORCED = ("nem12-S64-E40", "up-S8-E40")
FORCED_GENERIC = ("f64-own-S9-E64-a70", "f64-own-S9-E63-a171-generic")     # the amplitude-70 and -171 tables
GENERIC_MARGINED = tuple(n for n in rr.GENERIC if n not in FORCED_GENERIC)    # (evaluation 0)


# further shapes, each run with seeded uniforms (margins asserted like MARGINED's) and forced ones: S = 3, the
# S edges of a position loop, E at the wave and word edges, E on each side of every switch of the block size
# (64 | 128 | 256 | 512 | 1024 threads: E = 64 | 65, 128 | 129, 256 | 257, 512 | 513) and of the effects per thread
# (1024 | 1025), and past 1024 effects
SHAPES = (("small-S3-E17", "small-S15-E16", "nem04-S60-E40", "nem04-S64-E40")
          + tuple(f"small-S17-E{e}" for e in (1, 15, 16, 17, 63, 64, 128, 129, 256, 257, 512, 513, 1024, 1025))
          + (rr.PART_MODEL,))
WIDE_VISITS = 16                      # of rr.WIDE_MODEL (S = 128): nodes 0, 8, 16, ...


def evals_of(name, forced=False):
    """The evaluations of fm.inputs a model runs on: 0, 1 and 5 (soft, saturated and coin-flip weights on
    random orders); evaluation 0 alone at S = 64.  At S = 60 the saturated evaluation has a visit whose
    tolerance (5e-3) is wider than a CDF step, so like nem12 it cannot be margined: it runs forced alone."""
    if "-S64-" in name:
        return (0,)
    if "-S60-" in name and not forced:
        return (0, 5)
    return MARGINED_EVALS


def visits_of(name, s):
    if name == rr.WIDE_MODEL:
        return np.arange(0, s, s // WIDE_VISITS, dtype=np.int32)
    return label_sweeps(s, N_SWEEPS)


def label_sweeps(s, n=1):
    return np.tile(np.arange(s, dtype=np.int32), n)


def seeded_u(nv, k):
    """The uniforms of evaluation k: seed 5, one stream per evaluation."""
    return np.random.default_rng([U_SEED, k]).random(nv)


def forced_u(nv):
    """u alternating 0 and 2.0: the visited node goes to position 0, then to S - 1."""
    return np.where(np.arange(nv) % 2 == 0, 0.0, 2.0)


def forced_q(nv, s):
    return np.where(np.arange(nv) % 2 == 0, 0, s - 1)


import functools  # noqa: E402

N_SWEEPS = 2       # visits run on an updated state with drift


@functools.lru_cache(maxsize=None)
def _et(name):
    return np.exp(rr.get_model(name).T.astype(LD))


def factored_sweep_case(name, k, forced=False):
    """(model, perm, pos (S,), w (S, S), visit, u) of evaluation k of a factored model: N_SWEEPS
    sweeps in label order, seeded or forced uniforms."""
    m, perms, pos, w = rr.factored_case(name)
    visit = visits_of(name, m.S)
    us = forced_u(len(visit)) if forced else seeded_u(len(visit), k)
    return m, perms[k], pos[k], w[k], visit, us


@functools.lru_cache(maxsize=None)
def factored_sweep_ref(name, k, forced=False) -> SweepRef:
    m, perm, _, w, visit, us = factored_sweep_case(name, k, forced)
    return sweep_reference(m.U, m.T, perm, w, visit, us, et=_et(name))


def generic_sweep_case(name, k, forced=True):
    c, u, t, perms, pos, w = rr.generic_case(name)
    visit = label_sweeps(t.shape[0], N_SWEEPS)
    us = forced_u(len(visit)) if forced else seeded_u(len(visit), k)
    return c, u, t, perms[k], pos[k], w[k], visit, us


@functools.lru_cache(maxsize=None)
def generic_sweep_ref(name, k, forced=True) -> SweepRef:
    _, u, t, perm, _, w, visit, us = generic_sweep_case(name, k, forced)
    return sweep_reference(u, t, perm, w, visit, us, et=sm._exp_table(name))


@functools.lru_cache(maxsize=None)
def greedy_sweep_refs(min_gain=1e-9):
    """One greedy sweep in label order of every problem of reloc_ref.greedy_inputs()."""
    m, pos, w = rr.greedy_inputs()
    et = np.exp(m.T.astype(LD))
    visit = label_sweeps(m.S)
    return [sweep_reference(m.U, m.T, np.argsort(pos[k]), w[k], visit, None, beta=np.inf, min_gain=min_gain, et=et)
            for k in range(len(pos))]


def gibbs_start():
    b = rr.GIBBS_CHAINS
    rng = np.random.default_rng(rr.GIBBS_SEED)
    return np.stack([np.argsort(rng.permutation(4)) for _ in range(b)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def gibbs_margins():
    """The margin of every draw of the fused run on reloc_ref.gibbs_model() (48 chains, 40 sweeps, seed 11):
    -> (least margin, final pos)."""
    u, t, w = rr.gibbs_model()
    et = np.exp(t.astype(LD))
    pos = gibbs_start()
    rng = np.random.default_rng(rr.GIBBS_SEED)
    visit = label_sweeps(4)
    least = np.inf
    for _ in range(rr.GIBBS_SWEEPS):
        us = rng.random((4, len(pos)))
        for c in range(len(pos)):
            ref = sweep_reference(u, t, np.argsort(pos[c]), w, visit, us[:, c], et=et)
            least = min(least, float(ref.margin.min()))
            pos[c] = np.argsort(ref.perms[-1])
    return least, pos
