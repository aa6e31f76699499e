"""Nested Effects Model: observed knockdown data and the effect score tables.

Mirrors the reference ``nem.NEM`` (nem.py:8-144).  The class builds, on the
host and once per model, the two inputs of the hot path:

* the score tables ``T`` (nem.py:25-54): for child S-gene ``i`` and candidate
  parent ``j``, ``T[i][j][e]`` is the log-likelihood increment of effect ``e``;
* the node LR table ``U`` (nem.py:56-64), shape (S+1, E); row ``S`` is the
  "effect attached to nothing" row.

Both are reproduced bit for bit: the reference builds row ``i`` of ``T[i]`` and
row ``S`` of ``U`` by *sequential* float additions of ``A`` (nem.py:30-32,
nem.py:62), which differ from ``A * count`` in the last bits; we replay the
same addition chain through a lookup table instead of an S*S*E Python loop.

The tables are staged to HBM once by :class:`nemo.engine.Engine`; nothing in
this file is on the per-step path.

The true graph's scores (``compute_real_score``, nem.py:88-144; the six
``real_*`` / ``obs_*`` attributes the reference's constructor fills) are made
by :meth:`NEM.real_scores` on request: the host keeps the fit's loop, each of
its sweeps -- every permissible pair's bounded L-BFGS-B solve -- is one GPU
call (``Engine.real_sweep``), and construction itself stays free of GPU work.
"""
from __future__ import annotations

import random

import numpy as np

from . import utils


def _addition_chain(start: float, step: float, count: int) -> np.ndarray:
    """chain[k] = (((start + step) + step) ... + step), k additions (float64)."""
    chain = np.empty(count + 1, dtype=np.float64)
    acc = float(start)
    chain[0] = acc
    for k in range(1, count + 1):
        acc = acc + step
        chain[k] = acc
    return chain


class ScoreTables:
    """Lazy stand-in for the reference's list of S score tables (nem.py:49-54):
    indexable, iterable, sized; T[i] is built on access."""

    def __init__(self, nem, knockdown_mat):
        self._nem = nem
        self._d = knockdown_mat

    def __len__(self):
        return self._nem.num_s

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        i = int(i)
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        return self._nem.build_score_table(i, self._d)

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def __array__(self, dtype=None, copy=None):
        t = self._nem.get_score_tensor(self._d)
        return t if dtype is None else t.astype(dtype, copy=False)

    @property
    def knockdown_mat(self):
        return self._d


class TableModel:
    """A model given by its tables: ``U`` (S+1, E) and ``T`` (S, S, E), real
    valued.  ``NEMOrderMCMC``, ``ChainBatch`` and the replica driver take it in
    place of a ``NEM``: it has the attributes they read (``num_s``, ``num_e``,
    ``U``, ``get_score_tables``) and no knockdown matrix, so its engine is
    staged from the tables (``Engine.for_model``, option ``exact_generic``:
    the reference's bits for max|T| <= 670, max|U| <= 700 and E <= 8192, or E
    <= 524288 for a model of log ratios).

    A sampler built on a ``TableModel`` without an ``engine=`` always takes
    that option.  A table with its own rows per child then runs the exact
    step on stored rows (chains x pairs x plan doubles of device memory: 0.56
    GB at 64 x 2000, 16 chains).  A model of log ratios (``from_log_ratios``)
    is staged from ``R`` alone -- ``T`` is built only when read
    (``tables_built``) -- and runs on per-parent recompute rows (chains x S x
    plan doubles: 18 MB at 64 x 2000, 16 chains, plus 1 MB per staged table).  To run
    a model without the option, stage ``Engine(U, T)`` yourself and pass it as
    ``engine=``."""

    observed_knockdown_mat = None
    R = None   # from_log_ratios: the log ratios (S, E) the model was made from

    def __init__(self, U, T):
        T = np.ascontiguousarray(T, dtype=np.float64)
        U = np.ascontiguousarray(U, dtype=np.float64)
        if T.ndim != 3 or T.shape[0] != T.shape[1]:
            raise ValueError(f"T must be (S, S, E), got {T.shape}")
        if U.shape != (T.shape[0] + 1, T.shape[2]):
            raise ValueError(f"U must be ({T.shape[0] + 1}, {T.shape[2]}), got {U.shape}")
        self.num_s, self.num_e = int(T.shape[0]), int(T.shape[2])
        self.U, self._T = U, T

    @property
    def T(self) -> np.ndarray:
        """The score tables (S, S, E); a model of log ratios builds them on
        first access (the same array from then on)."""
        if self._T is None:
            s, e = self.R.shape
            t = np.empty((s, s, e), dtype=np.float64)
            t[:] = self.R[None, :, :]
            self._T = t
        return self._T

    @property
    def tables_built(self) -> bool:
        """True once ``T`` exists on the host."""
        return self._T is not None

    @classmethod
    def from_log_ratios(cls, R) -> "TableModel":
        """The model of per-effect log-likelihood ratios R (S, E), R[j][e] =
        l1 - l0 of effect e under the knockdown of S-gene j: nem.py:25-64 with
        the two-valued increments replaced by R and the per-effect constant
        sum_j l0 dropped -- every child shares parent j's row, T[i][j] = R[j]
        (the diagonal row T[i][i] = R[i] is U's row i), and U = [R; 0]."""
        R = np.ascontiguousarray(R, dtype=np.float64)
        if R.ndim != 2:
            raise ValueError(f"R must be (S, E), got {R.shape}")
        s, e = R.shape
        self = cls.__new__(cls)
        self.num_s, self.num_e = int(s), int(e)
        self.R, self.U, self._T = R, np.vstack([R, np.zeros((1, e))]), None
        return self

    def get_score_tables(self, _knockdown_mat=None):
        """The tables themselves (the same array on every call)."""
        return self.T


class NEM:
    """Reference: nem.py:8-22.

    ``adj_matrix[a][b] = 1`` is an edge a->b (closure form, as the bundled CSVs
    store it); ``end_nodes[k]`` is the S-gene effect ``k`` hangs off;
    ``errors = (alpha, beta)`` are the false-positive / false-negative rates.

    Construction consumes the global Python ``random`` stream exactly like the
    reference (``random.seed(seed)`` then ``create_observed_knockdown_mat``
    re-seeds with 42 and draws S*E numbers, utils.py:25-35), so a sampler
    started afterwards sees the same proposal stream.

    The reference also runs ``compute_real_score`` twice at construction
    (nem.py:21-22), an L-BFGS-B fit of the *true* graph that does not feed the
    sampler: the yardstick its users read a run against (``obs_ll``).  Here
    construction does no GPU work: its only side effect on shared state --
    zeroing the caller's adjacency diagonal in place (nem.py:90-91) -- is
    reproduced, and the six attributes ``real_order_ll``, ``real_ll``,
    ``real_parent_order``, ``obs_order_ll``, ``obs_ll``, ``obs_parent_order``
    stay ``None`` until :meth:`real_scores` runs the two fits on the GPU
    (``nemo_real_sweep``: every pair's solve of a sweep in one call).
    """

    def __init__(self, adj_matrix, end_nodes, errors, num_s, num_e, seed=42):
        self.num_s = int(num_s)
        self.num_e = int(num_e)
        self.adj_matrix = adj_matrix
        alpha, beta = float(errors[0]), float(errors[1])
        self.real_knockdown_mat = utils.create_real_knockdown_mat(adj_matrix, end_nodes)
        random.seed(seed)
        self.A = np.log(alpha / (1.0 - beta))
        self.B = np.log(beta / (1.0 - alpha))
        self.observed_knockdown_mat = utils.create_observed_knockdown_mat(
            self.real_knockdown_mat, alpha, beta)
        self._tensor_cache = None
        # U without the S*S*E table: the diagonal rows by their closed form
        # (bit-identical to get_node_lr_table(get_score_tables(D)), tested)
        self.U = self._node_lr_table_direct()
        # compute_real_score side effect (nem.py:90-91): diagonal of the
        # caller's adjacency zeroed in place.
        for i in range(self.num_s):
            adj_matrix[i][i] = 0
        self.real_order_ll = self.real_ll = self.real_parent_order = None
        self.obs_order_ll = self.obs_ll = self.obs_parent_order = None

    # -- A1: score tables -------------------------------------------------
    def _chains(self):
        """Addition chains of A from bases 0.0 and B (see module docstring)."""
        return (_addition_chain(0.0, self.A, self.num_s),
                _addition_chain(self.B, self.A, self.num_s))

    def compute_scores(self, node, knockdown_mat):
        """Base row of ``T[node]``: where(D[node]==1, 0, B) + sum_{m != node}
        where(D[m]==1, A, 0), summed in ascending m.  Reference: nem.py:25-34."""
        d = np.asarray(knockdown_mat)
        ones_elsewhere = (d == 1).sum(axis=0) - (d[node] == 1)
        chain0, chainb = self._chains()
        return np.where(d[node] == 1, chain0[ones_elsewhere], chainb[ones_elsewhere])

    def build_score_table(self, node, knockdown_mat):
        """``T[node]``, shape (S, E).  Row ``node`` is :meth:`compute_scores`;
        every other row m is where(D[m]==0, B, -A).  Reference: nem.py:36-47."""
        d = np.asarray(knockdown_mat)
        table = np.where(d == 0, self.B, -self.A).astype(np.float64)
        table[node, :] = self.compute_scores(node, d)
        return table

    def get_score_tables(self, knockdown_mat):
        """The S tables (S, E).  Reference: nem.py:49-54 (a list of arrays).

        Returned as a lazy sequence: ``tables[i]`` builds T[i] on access and
        ``np.asarray(tables)`` the whole tensor, so a sampler that only hands
        the model to the GPU (which builds its tables from D itself,
        ``nemo_stage_knockdown``) never holds the S*S*E table on the host."""
        return ScoreTables(self, knockdown_mat)

    def get_score_tensor(self, knockdown_mat=None) -> np.ndarray:
        """The score tables as one C-contiguous (S, S, E) float64 tensor
        ``T[i, j, e]`` (child i, parent j) -- the layout staged to HBM."""
        d = self.observed_knockdown_mat if knockdown_mat is None else np.asarray(knockdown_mat)
        if (self._tensor_cache is not None and self._tensor_cache[0] is d):
            return self._tensor_cache[1]
        s, e = self.num_s, self.num_e
        off_diag = np.where(d == 0, self.B, -self.A).astype(np.float64)
        ones_total = (d == 1).sum(axis=0)
        chain0, chainb = self._chains()
        tensor = np.empty((s, s, e), dtype=np.float64)
        tensor[:] = off_diag[None, :, :]
        for i in range(s):
            k = ones_total - (d[i] == 1)
            tensor[i, i] = np.where(d[i] == 1, chain0[k], chainb[k])
        self._tensor_cache = (d, tensor)
        return tensor

    # -- A2: node LR table --------------------------------------------------
    def _node_lr_table_direct(self):
        d = np.asarray(self.observed_knockdown_mat)
        chain0, chainb = self._chains()
        k = ((d == 1).sum(axis=0)[None, :] - (d == 1)).astype(np.int64)
        rows = np.where(d == 1, chain0[k], chainb[k])
        null_row = chain0[(d != 0).sum(axis=0)]
        return np.vstack([rows, null_row[None, :]])

    def get_node_lr_table(self, all_score_tables):
        """Rows 0..S-1: diagonal rows ``T[i][i]``; row S: sum over S-genes of
        where(D==0, 0, A), added row by row.  Reference: nem.py:56-64."""
        s = self.num_s
        rows = [np.asarray(all_score_tables[i])[i] for i in range(s)]
        chain0, _ = self._chains()
        null_row = chain0[(self.observed_knockdown_mat != 0).sum(axis=0)]
        return np.vstack(rows + [null_row])

    # -- the true graph's scores (nem.py:88-144) ------------------------------
    def compute_real_score(self, real_knockdown_mat, adj_mat, device: int = 0):
        """Reference: nem.py:88-144, on the GPU.  Returns ``(real_order_ll,
        real_ll, parent_order)`` for the tables of ``real_knockdown_mat``:

        * ``parent_order``: the S-genes by descending row sum of ``adj_mat``
          (diagonal zeroed in place; numpy's argsort, so ties fall as there);
        * the order's parent weights are fitted from 0.5 by sweeps
          (``Engine.real_sweep``: the evaluation, then every permissible
          pair's bounded solve against the whole order-weight matrix) while
          the evaluation's ll rose by more than 1e-4 (signed, at most 1000
          sweeps); the last sweep's weights are kept;
        * ``real_order_ll``: the order score at ``1 * (w > 0.5)``;
        * ``real_ll``: the score with the adjacency's own parent sets at
          weight 1 (i is a parent of j where ``adj_mat[i][j] == 1``).

        The node table's null row comes from ``observed_knockdown_mat``
        whatever ``real_knockdown_mat`` is (nem.py:62).  The host keeps only
        the loop; ``real_score_trace`` holds the last call's per-sweep ll and
        weights.  An edge of ``adj_mat`` that points backwards in
        ``parent_order`` (an adjacency not in closure form) raises
        ``ValueError``: the engine scores permissible parents only."""
        from .engine import Engine
        s = self.num_s
        for i in range(s):
            adj_mat[i][i] = 0
        row_sums = np.sum(adj_mat, axis=1)
        parent_order = np.argsort(row_sums)[::-1]
        pos = np.empty(s, dtype=np.int32)
        pos[parent_order] = np.arange(s, dtype=np.int32)
        adj = np.asarray(adj_mat)
        for i, j in zip(*np.nonzero(adj == 1)):
            if pos[i] >= pos[j]:
                raise ValueError(f"edge {i}->{j} of adj_mat points backwards in parent_order "
                                 f"(positions {pos[i]} and {pos[j]}): the adjacency is not in closure form")
        tables = self.get_score_tables(real_knockdown_mat)
        chain0, _ = self._chains()
        null_row = chain0[(np.asarray(self.observed_knockdown_mat) != 0).sum(axis=0)]
        u_mixed = np.vstack([self.compute_scores(i, real_knockdown_mat) for i in range(s)] + [null_row])
        eng = Engine.for_tables(u_mixed, tables, device=device)
        mask = pos[None, :] < pos[:, None]          # mask[i, j]: j is a permissible parent of i
        w = np.where(mask, 0.5, 0.0)
        ll_diff, old_ll, iter_count = float("inf"), -float("inf"), 0
        ll_list, w_list = [], []
        while ll_diff > 0.0001 and iter_count < 1000:
            w_out, ll, _info = eng.real_sweep(pos, w)
            w = np.where(mask, w_out[0], 0.0)
            ll_diff = float(ll[0]) - old_ll
            old_ll = float(ll[0])
            iter_count += 1
            ll_list.append(old_ll)
            w_list.append(w)
        rounded = np.where(mask, 1.0 * (w > 0.5), 0.0)
        real_order_ll = float(eng.score(pos, rounded)[0])
        real_ll = float(eng.score(pos, (adj == 1).T.astype(np.float64))[0])
        self.real_score_trace = {"sweeps": iter_count, "ll": np.array(ll_list), "weights": np.array(w_list),
                                 "rounded": rounded, "pos": pos}
        return real_order_ll, real_ll, parent_order

    def real_scores(self, device: int = 0):
        """The two calls of the reference's constructor (nem.py:21-22): the
        fit on the real and on the observed knockdown matrix; fills
        ``real_order_ll``, ``real_ll``, ``real_parent_order`` and ``obs_*``
        and returns ``self``."""
        self.real_order_ll, self.real_ll, self.real_parent_order = self.compute_real_score(
            self.real_knockdown_mat, self.adj_matrix, device=device)
        self.real_trace = self.real_score_trace
        self.obs_order_ll, self.obs_ll, self.obs_parent_order = self.compute_real_score(
            self.observed_knockdown_mat, self.adj_matrix, device=device)
        self.obs_trace = self.real_score_trace
        return self
