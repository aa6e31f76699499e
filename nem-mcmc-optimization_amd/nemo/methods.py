"""The fixed-order weight optimizers of the reference's methods.py on the GPU.

Mirrors ``InverseMethod`` (methods.py:21-172, the optimizer ``main()`` runs,
main.py:115-116) and ``Method`` (methods.py:342-436) with the reference's
constructor, attributes and ``optimize`` loop; the weight sweep of each
(``opt_b`` / ``opt_γ``) is one C-ABI call that evaluates the order score and
runs every pair's bounded L-BFGS-B on the device (``nemo_inverse_sweep`` /
``nemo_gamma_sweep``).  The host keeps only the loop
of ``optimize``: the ll bookkeeping, the best sweep and the final rounding.

``ExpitMethod`` / ``ExpMethod`` are not mirrored: the first has no
``optimize``; the second feeds exp(6.0) = 403 as a weight into
log(1 - w + w e^T), which is NaN for every table nem.py builds (e^B < 1),
so it has no meaningful output to match.
"""
from __future__ import annotations

import numpy as np

from .engine import Engine

INVERSE_BOUNDS = [(-5000, 500)]   # methods.py:132
GAMMA_BOUNDS = [(0, 1)]           # methods.py:408


def _positions(order):
    order = np.asarray(order)
    pos = np.empty(len(order), dtype=np.int32)
    pos[order] = np.arange(len(order))
    return pos


class _Base:
    def __init__(self, order, num_s, num_e, U, score_tables, engine: Engine | None = None,
                 device: int = 0, dtype: str = "f64"):
        self.order = order
        self.num_s = num_s
        self.num_e = num_e
        self.U = U
        self.score_tables = score_tables
        self.eye = np.eye(self.num_s)
        self.mask = np.zeros((self.num_s, self.num_s))
        self.get_permissible_parents(order, self.mask, init_val=1.0)
        self.engine = engine if engine is not None else Engine.for_tables(U, score_tables, device, dtype)
        self.engine.reserve(1, 1)
        self._pos = _positions(order)

    def get_permissible_parents(self, perm_order, weights, init_val=0.5, i1=None, i2=None):
        """methods.py:34-42: parents_list[i] = the order prefix before i; sets
        weights[i][j] = init_val on it (in place) and returns weights."""
        perm_order = np.asarray(perm_order)
        parents_list = np.empty(self.num_s, dtype=object)
        for i in range(self.num_s):
            index = int(np.where(perm_order == i)[0][0])
            parents_list[i] = perm_order[:index]
            for j in parents_list[i]:
                weights[i][j] = init_val
        self.parents_list = parents_list
        return weights

    def create_dag(self, weights):
        """methods.py:44-47."""
        return 1 * (weights > 0.5)

    def compute_cell_ratios(self, weights, score_tables):
        """methods.py:49-58 (raw weights, no expit) on the GPU."""
        eng = self.engine if score_tables is self.score_tables else Engine.for_tables(self.U, score_tables)
        out = eng.score(self._pos[None, :], np.asarray(weights, dtype=np.float64)[None], want_cells=True)
        return out["cells"][0]

    def calculate_ll(self, cell_ratios):
        """methods.py:60-64 -> (order_weights, ll)."""
        ll, _cs, ow = self.engine.lse(cell_ratios, want_ow=True)
        return ow, ll

    def _ll_of(self, weights):
        return float(self.engine.score(self._pos[None, :], np.asarray(weights, dtype=np.float64)[None])[0])

    @staticmethod
    def _loop(sweep, weights, max_iter, rel_diff):
        """The common loop of optimize (methods.py:150-164 / :418-429): stop
        when |ll - ll_old| <= rel_diff; best = the sweep whose evaluated ll
        is highest, its returned weights are kept."""
        ll_diff = float("inf")
        ll_old = -float("inf")
        ll_list, weight_list = [], []
        best_ll = -float("inf")
        best_index = 0
        iter_count = 0
        while iter_count < max_iter and ll_diff > rel_diff:
            ll, weights = sweep(weights)
            ll_list.append(ll)
            if ll > best_ll:
                best_ll = ll
                best_index = iter_count
            weight_list.append(weights)
            ll_diff = np.abs(ll - ll_old)
            ll_old = ll
            iter_count += 1
        return ll_list, weight_list, best_ll, best_index


class InverseMethod(_Base):
    """Reference: methods.py:21-172."""

    def exp_parent_weights(self, weights):
        """methods.py:66-71."""
        new_weights = np.array(weights, dtype=np.float64, copy=True)
        for i in range(self.num_s):
            for j in self.parents_list[i]:
                new_weights[i][j] = np.exp(new_weights[i][j])
        return new_weights

    def opt_b(self, weights, bounds):
        """methods.py:117-129: the evaluation on B/(1+B) and every pair's
        local optimum in the reference's loop order, in one device call."""
        if [tuple(b) for b in bounds] != [tuple(b) for b in INVERSE_BOUNDS]:
            raise NotImplementedError(f"opt_b runs with the reference's bounds {INVERSE_BOUNDS}")
        w_out, ll, _info = self.engine.inverse_sweep(self._pos[None, :], weights)
        return float(ll[0]), w_out[0]

    def ancestral(self, weights):
        """unorder_arr(order, B/(1+B)) of methods.py:118-121 / 160-163."""
        return self.engine.inverse_ancestral(self._pos[None, :], weights)[0]

    def optimize(self, max_iter=1000, rel_diff=1e-8, weights=None, init_weight=-5000.0, init_val=0.0,
                 use_wandb=False):
        """methods.py:131-172 -> (B_tilde.T, rounded ll).  ``use_wandb`` is
        accepted and ignored (no wandb here)."""
        bounds = INVERSE_BOUNDS
        if weights is None:
            weights = np.full((self.num_s, self.num_s), init_weight, dtype=np.float64)
            weights = self.get_permissible_parents(perm_order=self.order, weights=weights, init_val=init_val)
        else:
            weights = np.where(np.asarray(weights) == 0.0, init_weight, init_val).astype(np.float64)
        ll_list, weight_list, best_ll, best_index = self._loop(
            lambda w: self.opt_b(w, bounds), weights, max_iter, rel_diff)
        self.ll_list = ll_list
        weights = weight_list[best_index]
        print(f"Best ll: {best_ll}")
        b_tilde = 1 * (self.ancestral(weights) > 0.5)
        real_ll = self._ll_of(b_tilde)
        print(f"Rounded LL: {real_ll}")
        return b_tilde.T, real_ll


class Method(_Base):
    """Reference: methods.py:342-436 (the weights are probabilities in [0, 1])."""

    def opt_γ(self, weights, bounds):
        """methods.py:397-405."""
        if [tuple(b) for b in bounds] != [tuple(b) for b in GAMMA_BOUNDS]:
            raise NotImplementedError(f"opt_γ runs with the reference's bounds {GAMMA_BOUNDS}")
        w_out, ll, _info = self.engine.gamma_sweep(self._pos[None, :], weights)
        return float(ll[0]), w_out[0]

    def optimize(self, max_iter=1000, rel_diff=1e-8, use_wandb=False):
        """methods.py:407-436 -> (rounded weights.T, rounded ll)."""
        bounds = GAMMA_BOUNDS
        weights = np.zeros((self.num_s, self.num_s))
        weights = self.get_permissible_parents(perm_order=self.order, weights=weights, init_val=0.5)
        ll_list, weight_list, best_ll, best_index = self._loop(
            lambda w: self.opt_γ(w, bounds), weights, max_iter, rel_diff)
        self.ll_list = ll_list
        weights = 1 * (weight_list[best_index] > 0.5)
        print(f"Best ll: {best_ll}")
        real_ll = self._ll_of(weights)
        print(f"Rounded LL: {real_ll}")
        return weights.T, real_ll


class JointMethod(_Base):
    """All weights of a fixed order at once: logits X on the permissible
    pairs, w = expit(X), L-BFGS with a strong-Wolfe line search on -ll through
    ``nemo.autograd.order_score`` (the engine's gradient kernels).

    This is the working form of what the reference's
    ``NEMOrderMCMC.opt_weights`` / ``global_opt_fun`` (nem_order_mcmc.py:
    105-150) meant and crashes on; there is no reference output to match, so
    no parity is claimed.  The constructor, ``ll_list`` / ``best_ll`` and
    ``optimize``'s return follow ``Method``."""

    def optimize(self, max_iter=50, rel_diff=1e-8, use_wandb=False):
        """-> (rounded weights.T, rounded ll).  One entry of ``ll_list`` per
        evaluation of the closure (the first: every weight 0.5, ``Method``'s
        start); the weights of the best one are kept (``best_weights``,
        ``best_ll``), like the reference's ``best_index`` bookkeeping."""
        import torch

        from .autograd import order_score
        eng = self.engine
        dev = torch.device("cuda", eng.device)
        pos = torch.from_numpy(self._pos[None, :].copy()).to(dev)
        mask = torch.from_numpy(self.mask[None] > 0).to(dev)
        x = torch.zeros((1, self.num_s, self.num_s), dtype=torch.float64, device=dev, requires_grad=True)
        opt = torch.optim.LBFGS([x], max_iter=int(max_iter), tolerance_change=float(rel_diff),
                                line_search_fn="strong_wolfe")
        ll_list, best = [], {"ll": -float("inf"), "w": None}

        def closure():
            opt.zero_grad()
            w = torch.where(mask, torch.sigmoid(x), torch.zeros_like(x))
            ll = order_score(eng, pos, w)[0]
            (-ll).backward()
            v = float(ll.detach())
            ll_list.append(v)
            if v > best["ll"]:
                best["ll"], best["w"] = v, w.detach()[0].cpu().numpy()
            return -ll

        opt.step(closure)
        self.ll_list = ll_list
        self.best_ll = best["ll"]
        self.best_weights = best["w"]
        print(f"Best ll: {self.best_ll}")
        weights = 1 * (self.best_weights > 0.5)
        real_ll = self._ll_of(weights)
        print(f"Rounded LL: {real_ll}")
        return weights.T, real_ll


def greedy_flips(engine, pos, weights, cap=0, max_iter=None, min_gain=1e-9, ll_trace=None):
    """Greedy search over the DAGs of fixed orders by single-edge flips (the
    nem R package's ``nem.greedy`` within an order), B problems at once.

    ``pos`` (B, S) order positions, ``weights`` (B, S, S) with entries in {0, 1}.
    Every iteration is ONE ``engine.score_moves`` call over all B problems with
    ``w_alt = 1 - w``: the exact score change of every single flip.  Each problem
    applies its best flip if that gains more than ``min_gain`` (ties: the lowest
    (i, j)), else it is finished; the loop ends when every problem is finished or
    after ``max_iter`` iterations (default S * S).  -> (weights (B, S, S), ll
    (B,), n_flips (B,)); ll is that of a final ``score_moves`` call on the
    returned weights, not a running sum.  ``ll_trace``: a list that receives the
    (B,) ll of every call, the final one included."""
    pos = np.ascontiguousarray(np.atleast_2d(pos), dtype=np.int32)
    b, s = pos.shape
    w = np.array(weights, dtype=np.float64).reshape(b, s, s)
    if not np.isin(w, (0.0, 1.0)).all():
        raise ValueError("greedy_flips: weights must be 0 or 1")
    ok = pos[:, :, None] > pos[:, None, :]
    if 0 < cap < s - 1:
        ok &= pos[:, :, None] - pos[:, None, :] <= cap
    ok = ok.reshape(b, s * s)
    max_iter = s * s if max_iter is None else int(max_iter)
    n_flips = np.zeros(b, dtype=np.int64)
    active = np.ones(b, dtype=bool)
    rows = np.arange(b)
    it = 0
    while True:
        ll, dll = engine.score_moves(pos, w, 1.0 - w, cap=cap)
        if ll_trace is not None:
            ll_trace.append(np.array(ll))
        if it >= max_iter:
            return w, np.array(ll), n_flips
        gain = np.where(ok, np.asarray(dll).reshape(b, s * s), -np.inf)
        best = gain.argmax(axis=1)          # the first maximum: the lowest (i, j)
        active &= gain[rows, best] > min_gain
        if not active.any():                # nothing flips: this call's ll is the final one
            return w, np.array(ll), n_flips
        flat = w.reshape(b, s * s)
        flat[rows[active], best[active]] = 1.0 - flat[rows[active], best[active]]
        n_flips += active
        it += 1


class GreedyMethod(_Base):
    """Greedy single-edge search over the DAGs of one fixed order, every
    iteration one ``nemo_score_moves`` call (``greedy_flips``).  There is no
    reference counterpart in methods.py; the constructor, ``ll_list`` and
    ``optimize``'s return follow ``Method``."""

    def optimize(self, start=None, max_iter=None):
        """-> (weights.T, ll).  ``start``: a 0/1 weight matrix (default all
        zeros; entries off the permissible pairs are dropped).  ``ll_list``
        holds the ll at the start of each iteration, then the final one."""
        w = np.zeros((self.num_s, self.num_s)) if start is None else np.asarray(start, dtype=np.float64) * self.mask
        trace = []
        weights, ll, n = greedy_flips(self.engine, self._pos[None, :], w[None], max_iter=max_iter, ll_trace=trace)
        self.ll_list = [float(v[0]) for v in trace]
        self.n_flips = int(n[0])
        print(f"Greedy LL: {float(ll[0])} after {self.n_flips} flips")
        return (1 * (weights[0] > 0.5)).T, float(ll[0])


def _permissible(pos, cap):
    ok = pos[:, :, None] > pos[:, None, :]
    if 0 < cap < pos.shape[1] - 1:
        ok &= pos[:, :, None] - pos[:, None, :] <= cap
    return ok


def sweep_flips(engine, pos, weights, cap=0, max_sweeps=None, min_gain=1e-9, ll_trace=None):
    """Coordinate ascent over the DAGs of fixed orders by single-edge flips, B
    problems at once: every iteration is ONE ``engine.edge_sweep`` call with
    ``w_alt = 1 - w`` and ``thr = min_gain``, which visits every permissible
    pair in turn and takes each flip that gains more than ``min_gain`` at the
    state the earlier flips of the same sweep left.  The loop ends when a sweep
    takes nothing in every problem -- then no single flip gains more than
    ``min_gain``, ``greedy_flips``' own stop rule -- or after ``max_sweeps``
    sweeps (default S * S).  -> (weights (B, S, S), ll (B,), n_flips (B,),
    n_sweeps); ll is the last sweep's score of the returned weights.
    ``ll_trace``: a list that receives the (B,) ll before the first sweep and
    after every sweep."""
    pos = np.ascontiguousarray(np.atleast_2d(pos), dtype=np.int32)
    b, s = pos.shape
    w = np.array(weights, dtype=np.float64).reshape(b, s, s)
    if not np.isin(w, (0.0, 1.0)).all():
        raise ValueError("sweep_flips: weights must be 0 or 1")
    max_sweeps = s * s if max_sweeps is None else int(max_sweeps)
    thr = np.full((b, s, s), float(min_gain))
    n_flips = np.zeros(b, dtype=np.int64)
    n_sweeps = 0
    ll = None
    while n_sweeps < max_sweeps:
        w, _, ll0, ll, _, nacc = engine.edge_sweep(pos, w, 1.0 - w, thr, cap=cap)
        if ll_trace is not None:
            if n_sweeps == 0:
                ll_trace.append(np.array(ll0))
            ll_trace.append(np.array(ll))
        n_sweeps += 1
        n_flips += nacc
        if not np.any(nacc):
            break
    if ll is None:      # max_sweeps = 0: the score of the start (a sweep that takes nothing)
        _, _, ll, _, _, _ = engine.edge_sweep(pos, w, 1.0 - w, np.full((b, s, s), np.inf), cap=cap)
    return w, np.array(ll), n_flips, n_sweeps


def gibbs_edges(engine, pos, weights, n_sweeps, beta=1.0, log_prior_odds=0.0, burn_in=0, rng=None, cap=0):
    """Systematic-scan Gibbs sampler over the 0/1 DAGs of fixed orders, B chains
    at once, target proportional to exp(beta ll + log_prior_odds * edges).

    Every sweep is ONE ``engine.edge_sweep`` call with ``w_alt = 1 - w``: the
    host draws u ~ U(0, 1) per pair and sets thr = (logit(u) - s rho) / beta, s
    = +1 where the move switches the edge on and -1 where it switches it off --
    u < sigmoid(beta gain + s rho), the edge's full conditional, solved for the
    gain.  -> (weights (B, S, S), ll (n_sweeps, B), edge_prob (B, S, S));
    edge_prob is the Rao-Blackwellised marginal: the mean over the sweeps from
    ``burn_in`` on of sigmoid(beta (ll(edge on) - ll(edge off)) + rho), each
    edge's conditional at its visit, and 0 off the permissible pairs.  beta ->
    inf gives thr = 0, ``sweep_flips``' decision: annealing is a loop over this
    call.  ``rng``: a seed or a numpy Generator."""
    pos = np.ascontiguousarray(np.atleast_2d(pos), dtype=np.int32)
    b, s = pos.shape
    w = np.array(weights, dtype=np.float64).reshape(b, s, s)
    if not np.isin(w, (0.0, 1.0)).all():
        raise ValueError("gibbs_edges: weights must be 0 or 1")
    if not beta > 0.0:
        raise ValueError("gibbs_edges: beta must be positive")
    rng = np.random.default_rng(rng)
    ok = _permissible(pos, cap)
    rho, beta = float(log_prior_odds), float(beta)
    lls = np.empty((int(n_sweeps), b))
    prob = np.zeros((b, s, s))
    kept = 0
    for k in range(int(n_sweeps)):
        u = rng.random((b, s, s))
        sign = np.where(w < 0.5, 1.0, -1.0)
        with np.errstate(divide="ignore"):
            thr = ((np.log(u) - np.log1p(-u)) - sign * rho) / beta
        thr[~ok] = 0.0
        w, _, _, lls[k], gain, _ = engine.edge_sweep(pos, w, 1.0 - w, thr, cap=cap)
        if k >= burn_in:
            z = beta * sign * gain + rho
            prob += np.where(ok, 0.5 * (1.0 + np.tanh(0.5 * z)), 0.0)
            kept += 1
    return w, lls, prob / max(kept, 1)


class SweepMethod(_Base):
    """Coordinate ascent over the DAGs of one fixed order, every iteration one
    ``nemo_edge_sweep`` call (``sweep_flips``).  There is no reference
    counterpart in methods.py; the constructor, ``ll_list`` and ``optimize``'s
    return follow ``GreedyMethod``."""

    def optimize(self, start=None, max_sweeps=None):
        """-> (weights.T, ll).  ``start``: a 0/1 weight matrix (default all
        zeros; entries off the permissible pairs are dropped).  ``ll_list``
        holds the ll at the start and after every sweep."""
        w = np.zeros((self.num_s, self.num_s)) if start is None else np.asarray(start, dtype=np.float64) * self.mask
        trace = []
        weights, ll, n, sweeps = sweep_flips(self.engine, self._pos[None, :], w[None], max_sweeps=max_sweeps,
                                             ll_trace=trace)
        self.ll_list = [float(v[0]) for v in trace]
        self.n_flips = int(n[0])
        self.n_sweeps = int(sweeps)
        print(f"Sweep LL: {float(ll[0])} after {self.n_flips} flips in {self.n_sweeps} sweeps")
        return (1 * (weights[0] > 0.5)).T, float(ll[0])


def apply_relocation(pos, a, q):
    """The order positions after node ``a`` moves to position ``q`` and every
    other node keeps its relative order (pure numpy).  ``pos`` (S,) with scalar
    ``a``, ``q``, or (B, S) with (B,) arrays: one relocation per row.  The nodes
    between the old and the new position shift by one towards the old one."""
    pos = np.asarray(pos)
    out = np.array(np.atleast_2d(pos), dtype=pos.dtype)
    a = np.atleast_1d(np.asarray(a, dtype=np.int64))
    q = np.atleast_1d(np.asarray(q, dtype=np.int64))
    rows = np.arange(out.shape[0])
    p = out[rows, a].astype(np.int64)[:, None]
    qq = q[:, None]
    down = (out > p) & (out <= qq)       # q > p: positions p+1 .. q move down by one
    up = (out >= qq) & (out < p)         # q < p: positions q .. p-1 move up by one
    out = out - down.astype(out.dtype) + up.astype(out.dtype)
    out[rows, a] = q
    return out[0] if pos.ndim == 1 else out


def greedy_relocations(engine, pos, weights, max_iter=None, min_gain=1e-9, ll_trace=None):
    """Hill-climb over ORDERS at a fixed full weight matrix by single-node
    relocations, B problems at once.

    ``pos`` (B, S) order positions, ``weights`` (B, S, S) full weight matrices
    (weights[b, i, j]: the weight of pair (i, j) whenever j precedes i).  Every
    iteration is ONE ``engine.score_relocations`` call over all B problems.  Each
    problem applies its best (node a, position q) if that gains more than
    ``min_gain`` (ties: the lowest (a, q)), else it is finished; the loop ends
    when every problem is finished or after ``max_iter`` iterations (default S *
    S).  -> (pos (B, S), ll (B,), n_moves (B,)); ll is that of a final
    ``score_relocations`` call on the returned orders, not a running sum.
    ``ll_trace``: a list that receives the (B,) ll of every call."""
    pos = np.array(np.atleast_2d(pos), dtype=np.int32)
    b, s = pos.shape
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(b, s, s))
    max_iter = s * s if max_iter is None else int(max_iter)
    n_moves = np.zeros(b, dtype=np.int64)
    active = np.ones(b, dtype=bool)
    rows = np.arange(b)
    it = 0
    while True:
        ll, dll = engine.score_relocations(pos, w)
        if ll_trace is not None:
            ll_trace.append(np.array(ll))
        if it >= max_iter:
            return pos, np.array(ll), n_moves
        gain = np.asarray(dll).reshape(b, s * s)
        best = gain.argmax(axis=1)          # the first maximum: the lowest (a, q)
        active &= gain[rows, best] > min_gain
        if not active.any():                # nothing moves: this call's ll is the final one
            return pos, np.array(ll), n_moves
        a, q = np.divmod(best, s)
        pos[active] = apply_relocation(pos[active], a[active], q[active])
        n_moves += active
        it += 1


def gibbs_orders(engine, pos, weights, n_sweeps, beta=1.0, burn_in=0, rng=None, fused=False):
    """Systematic-scan Gibbs sampler over ORDERS at a fixed full weight matrix
    by node relocation (Kuipers & Moffa), B chains at once, target proportional
    to exp(beta ll(order)).

    For each node a in label order, ONE ``engine.score_relocations`` call over
    all B chains gives the score of every position of a; the host draws a's new
    position from its full conditional p(q) proportional to exp(beta dll[a, q])
    by inverse CDF from one uniform per chain and applies it.  -> (pos (B, S),
    ll (n_sweeps * S, B), before (B, S, S)): ll[k * S + a] is the score of the
    order each chain holds after sweep k's draw of node a (the call's ll plus
    the drawn entry of dll); before[b, i, j] is the Rao-Blackwellised marginal
    P(j precedes i): the mean, over the sweeps from ``burn_in`` on and over the
    visits of i and of j, of the visited node's conditional probability of
    landing on the matching side of the other (0 on the diagonal).  ``rng``: a
    seed or a numpy Generator.

    ``fused=True``: every sweep is ONE ``engine.order_sweep`` call that visits
    the nodes in label order on the device, with the sweep's uniforms drawn as
    ``rng.random((S, B))`` -- the stream S successive ``rng.random(B)`` consume --
    so the chains are the unfused ones wherever no uniform falls within rounding
    of a CDF step; ll comes from the call's per-visit scores and ``before`` from
    its rows and the orders replayed from the positions taken."""
    pos = np.array(np.atleast_2d(pos), dtype=np.int32)
    b, s = pos.shape
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(b, s, s))
    if not beta > 0.0:
        raise ValueError("gibbs_orders: beta must be positive")
    rng = np.random.default_rng(rng)
    beta = float(beta)
    rows = np.arange(b)
    lls = np.empty((int(n_sweeps) * s, b))
    before = np.zeros((b, s, s))
    kept = 0
    if fused:
        if not np.isfinite(beta):
            raise ValueError("gibbs_orders: beta must be finite")
        visit = np.ascontiguousarray(np.broadcast_to(np.arange(s, dtype=np.int32), (b, s)))
        for k in range(int(n_sweeps)):
            u = np.ascontiguousarray(rng.random((s, b)).T)
            pos_out, _, _, q, dll, ll_vis, _ = engine.order_sweep(pos, w, visit, u=u, beta=beta)
            lls[k * s:(k + 1) * s] = np.asarray(ll_vis).T
            for a in range(s):
                if k >= burn_in:
                    g = beta * np.asarray(dll)[:, a, :]
                    pq = np.exp(g - g.max(axis=1, keepdims=True))
                    cdf = np.cumsum(pq, axis=1)
                    rank = pos - (pos > pos[:, a][:, None])
                    above = 1.0 - cdf[rows[:, None], rank] / cdf[:, -1][:, None]
                    above[:, a] = 0.0
                    before[:, a, :] += above
                    below = 1.0 - above
                    below[:, a] = 0.0
                    before[:, :, a] += below
                pos = apply_relocation(pos, np.full(b, a), np.asarray(q)[:, a])
            pos = np.array(pos_out, dtype=np.int32)
            kept += k >= burn_in
        return pos, lls, before / max(2 * kept, 1)
    for k in range(int(n_sweeps)):
        for a in range(s):
            ll, dll = engine.score_relocations(pos, w)
            g = beta * np.asarray(dll)[:, a, :]
            pq = np.exp(g - g.max(axis=1, keepdims=True))
            cdf = np.cumsum(pq, axis=1)
            u = rng.random(b)
            q = np.minimum((cdf < (u * cdf[:, -1])[:, None]).sum(axis=1), s - 1)
            if k >= burn_in:
                # rank of every other node with a taken out; j precedes a iff a lands past it
                rank = pos - (pos > pos[:, a][:, None])
                above = 1.0 - cdf[rows[:, None], rank] / cdf[:, -1][:, None]   # P(q > rank_j)
                above[:, a] = 0.0
                before[:, a, :] += above
                below = 1.0 - above
                below[:, a] = 0.0
                before[:, :, a] += below
            lls[k * s + a] = np.asarray(ll) + np.asarray(dll)[rows, a, q]
            pos = apply_relocation(pos, np.full(b, a), q)
        kept += k >= burn_in
    return pos, lls, before / max(2 * kept, 1)


def sweep_relocations(engine, pos, weights, max_sweeps=None, min_gain=1e-9, ll_trace=None):
    """Coordinate ascent over ORDERS at a fixed full weight matrix, B problems at
    once: every iteration is ONE greedy ``engine.order_sweep`` call (``beta =
    inf``) that visits the nodes in label order and moves each to its best
    position if that gains more than ``min_gain`` at the order the earlier moves
    of the same sweep left.  The loop ends when a sweep moves nothing in every
    problem -- then no single relocation gains more than ``min_gain``,
    ``greedy_relocations``' own stop rule -- or after ``max_sweeps`` sweeps
    (default S * S).  -> (pos (B, S), ll (B,), n_moves (B,), n_sweeps); ll is
    the last sweep's score of the returned orders.  ``ll_trace``: a list that
    receives the (B,) ll before the first sweep and after every sweep."""
    pos = np.array(np.atleast_2d(pos), dtype=np.int32)
    b, s = pos.shape
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(b, s, s))
    max_sweeps = s * s if max_sweeps is None else int(max_sweeps)
    visit = np.ascontiguousarray(np.broadcast_to(np.arange(s, dtype=np.int32), (b, s)))
    n_moves = np.zeros(b, dtype=np.int64)
    n_sweeps = 0
    ll = None
    while n_sweeps < max_sweeps:
        pos, ll0, ll, _, _, _, nmoved = engine.order_sweep(pos, w, visit, beta=np.inf, min_gain=min_gain)
        if ll_trace is not None:
            if n_sweeps == 0:
                ll_trace.append(np.array(ll0))
            ll_trace.append(np.array(ll))
        n_sweeps += 1
        n_moves += nmoved
        if not np.any(nmoved):
            break
    if ll is None:      # max_sweeps = 0: the score of the start (no visits)
        _, _, ll, _, _, _, _ = engine.order_sweep(pos, w, visit[:, :0], beta=np.inf, min_gain=min_gain)
    return np.array(pos, dtype=np.int32), np.array(ll), n_moves, n_sweeps


__all__ = ["InverseMethod", "Method", "JointMethod", "GreedyMethod", "greedy_flips", "SweepMethod", "sweep_flips",
           "gibbs_edges", "apply_relocation", "greedy_relocations", "gibbs_orders", "sweep_relocations",
           "INVERSE_BOUNDS", "GAMMA_BOUNDS"]
