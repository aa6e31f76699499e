"""Python face of the C-ABI: one :class:`Engine` per (model, device).

An Engine owns a ``nemo_ctx``: the staged tables exp(T) and U in HBM plus the
per-batch scratch.  Host-array methods mirror the reference's numerical
routines batch-wise; ``*_dev`` methods take raw device pointers (e.g. from
``torch.Tensor.data_ptr()``) for callers that keep inputs resident in HBM.
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import _lib
from ._lib import check, f64, i32, ptr

_DTYPES = {"f64": _lib.NEMO_F64, "f32": _lib.NEMO_F32}


class ExactArithmeticWarning(UserWarning):
    """The staged model is outside what the reference-arithmetic kernels
    cover, so the sampler's step runs the fast kernels: log-scores within
    1e-6 of the reference's, not its bits."""


class Engine:
    """Staged model on one GPU.

    ``U`` (S+1, E) and ``T`` (S, S, E) are the reference's node LR table and
    score tables (nem.py:49-64).  ``dtype='f32'`` stores exp(T) and U in fp32
    and runs the per-element products in fp32 (the C5 configuration); logs,
    log-sum-exp and the effect sum stay fp64.

    ``exact_generic=True`` (option ``exact_generic``, set before staging):
    real-valued tables that are not factorable are staged for the
    reference-arithmetic kernels too -- covered for max|T| <= 670, max|U| <=
    700 (``nemo.limits``) and E <= 8192, or E <= 524288 when every child shares
    parent j's row
    (``from_log_ratios``; ``exact_status``); a factorable table is unaffected.
    """

    def __init__(self, U, T, device: int = 0, dtype: str = "f64", exact_generic: bool = False):
        U = f64(U)
        T = f64(T)
        if T.ndim != 3 or T.shape[0] != T.shape[1]:
            raise ValueError(f"T must be (S, S, E), got {T.shape}")
        S, _, E = T.shape
        if U.shape != (S + 1, E):
            raise ValueError(f"U must be ({S + 1}, {E}), got {U.shape}")
        self._create(S, E, device, dtype)
        if exact_generic:
            self.set_option("exact_generic", 1)
        check(_lib.load().nemo_stage_tables(self._ctx, ptr(U), ptr(T)))

    def _create(self, S, E, device, dtype):
        lib = _lib.load()
        self.S, self.E, self.device, self.dtype = S, E, device, dtype
        self._ctx = C.c_void_p()
        check(lib.nemo_ctx_create(device, S, E, _DTYPES[dtype], C.byref(self._ctx)))
        self._fin = weakref.finalize(self, lib.nemo_ctx_destroy, self._ctx)

    @classmethod
    def from_knockdown(cls, D, A, B, device: int = 0, dtype: str = "f64") -> "Engine":
        """The model built on the GPU from the observed knockdown matrix D
        (S, E) with entries 0/1 and the NEM's A, B (nem.py:17-18, 25-64):
        the same staged tables as ``Engine(U, T)`` with the reference's U and
        T, without the S*S*E host table."""
        D = np.asarray(D)
        if D.ndim != 2:
            raise ValueError(f"D must be (S, E), got {D.shape}")
        if not np.isin(D, (0, 1)).all():
            raise ValueError("D must hold only 0 and 1")
        d8 = np.ascontiguousarray(D, dtype=np.uint8)
        self = cls.__new__(cls)
        self._create(d8.shape[0], d8.shape[1], device, dtype)
        check(_lib.load().nemo_stage_knockdown(self._ctx, d8.ctypes.data_as(_lib._u8p),
                                               float(A), float(B)))
        return self

    @classmethod
    def from_log_ratios(cls, R, U=None, device: int = 0, dtype: str = "f64",
                        exact_generic: bool = True) -> "Engine":
        """The model of per-effect log-likelihood ratios R (S, E), T[i][j] =
        R[j] for every child i (``TableModel.from_log_ratios``), staged from R
        alone (``nemo_stage_log_ratios``): the same staged tables as
        ``Engine(U, T, exact_generic=...)`` with the broadcast T, without the
        S*S*E host table.  ``U`` defaults to ``[R; 0]``."""
        R = f64(R)
        if R.ndim != 2:
            raise ValueError(f"R must be (S, E), got {R.shape}")
        s, e = R.shape
        U = np.vstack([R, np.zeros((1, e))]) if U is None else f64(U)
        if U.shape != (s + 1, e):
            raise ValueError(f"U must be ({s + 1}, {e}), got {U.shape}")
        self = cls.__new__(cls)
        self._create(s, e, device, dtype)
        if exact_generic:
            self.set_option("exact_generic", 1)
        check(_lib.load().nemo_stage_log_ratios(self._ctx, ptr(U), ptr(R)))
        return self

    # -- cached engines per model -----------------------------------------
    @classmethod
    def for_nem(cls, nem, device: int = 0, dtype: str = "f64") -> "Engine":
        """The model's engine (one per device and dtype), staged from its
        knockdown matrix on the GPU (``from_knockdown``).  A model that holds
        tables and no knockdown matrix (``nemo.nem.TableModel``) is staged
        from its tables (``for_model``)."""
        if getattr(nem, "observed_knockdown_mat", None) is None:
            return cls.for_model(nem, device=device, dtype=dtype)
        cache = nem.__dict__.setdefault("_nemo_engines", {})
        key = (device, dtype)
        eng = cache.get(key)
        if eng is None:
            eng = cls.from_knockdown(nem.observed_knockdown_mat, nem.A, nem.B, device=device,
                                     dtype=dtype)
            cache[key] = eng
        return eng

    @classmethod
    def for_model(cls, model, device: int = 0, dtype: str = "f64", exact_generic: bool = True) -> "Engine":
        """The engine of a table model (``nemo.nem.TableModel``: ``U`` and
        ``get_score_tables``), one per device, dtype and ``exact_generic``,
        cached on the model as ``for_nem`` caches a NEM's.  A model that
        holds its log ratios (``TableModel.from_log_ratios``: ``R``) is staged
        from them (``from_log_ratios``), its tables never built."""
        cache = model.__dict__.setdefault("_nemo_engines", {})
        key = (device, dtype, bool(exact_generic))
        eng = cache.get(key)
        if eng is None:
            if getattr(model, "R", None) is not None:
                eng = cls.from_log_ratios(model.R, model.U, device=device, dtype=dtype,
                                          exact_generic=exact_generic)
            else:
                t = np.asarray(model.get_score_tables(None), dtype=np.float64)
                eng = cls(model.U, t, device=device, dtype=dtype, exact_generic=exact_generic)
            cache[key] = eng
        return eng

    @classmethod
    def for_tables(cls, U, score_tables, device: int = 0, dtype: str = "f64",
                   exact_generic: bool = False) -> "Engine":
        """Engine for the (U, score_tables) pair a caller of methods.py holds:
        the model's cached engine, staged from D, when the tables are a NEM's
        lazy tables and U is its U; else a new engine on the given tables
        (``exact_generic``: as ``Engine``)."""
        from .nem import ScoreTables
        if isinstance(score_tables, ScoreTables):
            nem = score_tables._nem
            if score_tables.knockdown_mat is nem.observed_knockdown_mat and np.array_equal(U, nem.U):
                return cls.for_nem(nem, device=device, dtype=dtype)
        return cls(U, np.asarray(score_tables, dtype=np.float64), device=device, dtype=dtype,
                   exact_generic=exact_generic)

    @property
    def handle(self):
        return self._ctx

    def close(self):
        self._fin()

    def reserve(self, max_batch: int, max_chains: int = 0):
        check(_lib.load().nemo_reserve(self._ctx, int(max_batch), int(max_chains)))

    # -- A4 + A5 -----------------------------------------------------------
    def score(self, pos, w01, cap: int = 0, want_cs=False, want_cells=False, want_ow=False):
        """Batched order scores.  pos (B, S) int, w01 (B, S, S) mapped weights.
        Returns ll (B,) or a dict with the requested extras."""
        pos = i32(np.atleast_2d(pos))
        b = pos.shape[0]
        w01 = f64(w01).reshape(b, self.S, self.S)
        ll = np.empty(b)
        cs = np.empty((b, self.E)) if want_cs else None
        cells = np.empty((b, self.S + 1, self.E)) if want_cells else None
        ow = np.empty((b, self.S + 1, self.E)) if want_ow else None
        a = _lib.addr  # plain addresses (~0.4 us each against ~4 for ctypes.data_as)
        check(_lib.load().nemo_score(self._ctx, b, a(pos), a(w01), int(cap), a(ll),
                                     None if cs is None else a(cs), None if cells is None else a(cells),
                                     None if ow is None else a(ow)))
        if not (want_cs or want_cells or want_ow):
            return ll
        return {"ll": ll, "cs": cs, "cells": cells, "ow": ow}

    def score_dev(self, batch, d_pos, d_w01, d_ll, cap=0, stream=None, group=1):
        """Enqueue a batched evaluation on device pointers (no sync)."""
        lib = _lib.load()
        if group == 1:
            check(lib.nemo_score_dev(self._ctx, int(batch), d_pos, d_w01, int(cap), d_ll,
                                     None, None, None, stream))
        else:
            check(lib.nemo_score_group_dev(self._ctx, int(batch), int(group), d_pos, d_w01,
                                           int(cap), d_ll, stream))

    # -- d ll / d w01 ---------------------------------------------------------
    def score_grad(self, pos, w01, cap: int = 0):
        """Order scores and their gradient in the mapped weights: (ll (B,),
        grad (B, S, S)), grad[b, i, j] = d ll[b] / d w01[b, i, j] at the
        permissible pairs and exactly 0 elsewhere (fp64 engines only)."""
        pos = i32(np.atleast_2d(pos))
        b = pos.shape[0]
        w01 = f64(w01).reshape(b, self.S, self.S)
        ll = np.empty(b)
        grad = np.empty((b, self.S, self.S))
        a = _lib.addr
        check(_lib.load().nemo_score_grad(self._ctx, b, a(pos), a(w01), int(cap), a(ll), a(grad)))
        return ll, grad

    def score_grad_dev(self, batch, d_pos, d_w01, d_ll, d_grad, cap=0, stream=None):
        """Enqueue ``score_grad`` on device pointers (no sync; ``reserve``
        the batch first)."""
        check(_lib.load().nemo_score_grad_dev(self._ctx, int(batch), d_pos, d_w01, int(cap), d_ll, d_grad, stream))

    # -- the exact score change of every single-weight move ---------------------
    def score_moves(self, pos, w01, w_alt, cap: int = 0):
        """Order scores and the exact change of each under every single-weight
        move: (ll (B,), dll (B, S, S)), dll[b, i, j] = ll[b] with w01[b, i, j]
        replaced by w_alt[b, i, j] alone, minus ll[b], at the permissible pairs
        and exactly 0 elsewhere (fp64 engines only).  ``w_alt`` is read only at
        the permissible pairs and must lie in [0, 1] there."""
        pos = i32(np.atleast_2d(pos))
        b = pos.shape[0]
        w01 = f64(w01).reshape(b, self.S, self.S)
        w_alt = f64(w_alt).reshape(b, self.S, self.S)
        ll = np.empty(b)
        dll = np.empty((b, self.S, self.S))
        a = _lib.addr
        check(_lib.load().nemo_score_moves(self._ctx, b, a(pos), a(w01), a(w_alt), int(cap), a(ll), a(dll)))
        return ll, dll

    def score_moves_dev(self, batch, d_pos, d_w01, d_w_alt, d_ll, d_dll, cap=0, stream=None):
        """Enqueue ``score_moves`` on device pointers (no sync; ``reserve``
        the batch first)."""
        check(_lib.load().nemo_score_moves_dev(self._ctx, int(batch), d_pos, d_w01, d_w_alt, int(cap), d_ll, d_dll,
                                               stream))

    # -- the exact score change of every single-node relocation of an order -------
    def score_relocations(self, pos, w01, cap: int = 0):
        """Order scores and the exact change of each under every single-node
        relocation at a fixed FULL weight matrix: (ll (B,), dll (B, S, S)),
        dll[b, a, q] = the score after moving node a to position q (everything
        else keeps its relative order), minus ll[b]; dll[b, a, pos[b, a]] is
        exactly 0 (fp64 engines only).  ``w01`` is read at every off-diagonal
        entry: w01[b, i, j] is the weight pair (i, j) carries whenever j
        precedes i.  ``cap`` must cut nothing (0 or >= S - 1)."""
        pos = i32(np.atleast_2d(pos))
        b = pos.shape[0]
        w01 = f64(w01).reshape(b, self.S, self.S)
        ll = np.empty(b)
        dll = np.empty((b, self.S, self.S))
        a = _lib.addr
        check(_lib.load().nemo_score_relocations(self._ctx, b, a(pos), a(w01), int(cap), a(ll), a(dll)))
        return ll, dll

    def score_relocations_dev(self, batch, d_pos, d_w01, d_ll, d_dll, cap=0, stream=None):
        """Enqueue ``score_relocations`` on device pointers (no sync;
        ``reserve`` the batch first)."""
        check(_lib.load().nemo_score_relocations_dev(self._ctx, int(batch), d_pos, d_w01, int(cap), d_ll, d_dll,
                                                     stream))

    # -- one sweep over the single-weight moves, each taken or not in turn --------
    def edge_sweep(self, pos, w01, w_alt, thr, cap: int = 0):
        """One sequential sweep over the permissible pairs of every order
        (children by order position, then parents by order position): each
        pair's move w01[b, i, j] -> w_alt[b, i, j] is scored exactly at the
        CURRENT state and taken iff its gain exceeds thr[b, i, j] (+inf never,
        -inf always).  -> (w_out, alt_out, ll0 (B,), ll (B,), gain (B, S, S),
        nacc (B,)): w_out holds w_alt where the move was taken, alt_out the
        value it replaced (a call on (w_out, alt_out) proposes the reverse
        moves), ll0 / ll the scores of w01 / w_out, gain each pair's gain at
        its visit (exactly 0 off the permissible pairs), nacc the moves taken.
        ``w_alt`` must lie in [0, 1] and ``thr`` must not be NaN at the
        permissible pairs; neither is read elsewhere (fp64 engines only)."""
        pos = i32(np.atleast_2d(pos))
        b = pos.shape[0]
        w01 = f64(w01).reshape(b, self.S, self.S)
        w_alt = f64(w_alt).reshape(b, self.S, self.S)
        thr = f64(thr).reshape(b, self.S, self.S)
        w_out = np.empty((b, self.S, self.S))
        alt_out = np.empty((b, self.S, self.S))
        ll0, ll = np.empty(b), np.empty(b)
        gain = np.empty((b, self.S, self.S))
        nacc = np.empty(b, dtype=np.int32)
        a = _lib.addr
        check(_lib.load().nemo_edge_sweep(self._ctx, b, a(pos), a(w01), a(w_alt), a(thr), int(cap), a(w_out),
                                          a(alt_out), a(ll0), a(ll), a(gain), a(nacc)))
        return w_out, alt_out, ll0, ll, gain, nacc

    def edge_sweep_dev(self, batch, d_pos, d_w01, d_w_alt, d_thr, d_w_out, d_alt_out, d_ll, d_ll0=None, d_gain=None,
                       d_nacc=None, cap=0, stream=None):
        """Enqueue ``edge_sweep`` on device pointers (no sync; ``reserve`` the
        batch first).  ``d_w_out`` may be ``d_w01`` and ``d_alt_out`` may be
        ``d_w_alt`` (in place); a NaN threshold never takes its move."""
        check(_lib.load().nemo_edge_sweep_dev(self._ctx, int(batch), d_pos, d_w01, d_w_alt, d_thr, int(cap), d_w_out,
                                              d_alt_out, d_ll0, d_ll, d_gain, d_nacc, stream))

    # -- relocations walked in sequence, each drawn or taken in turn ----------------
    def order_sweep(self, pos, w01, visit, u=None, beta: float = 1.0, min_gain: float = 0.0, cap: int = 0):
        """A list of node visits per order walked in ONE call at a fixed FULL
        weight matrix: at visit k node ``visit[b, k]`` has its S positions
        scored exactly at the CURRENT order (``score_relocations``' row), one is
        chosen and the move is applied.  ``beta`` finite: a Gibbs draw from
        ``u[b, k]`` by inverse CDF over exp(beta row), positions ascending (u =
        0: position 0, u >= 1: position S - 1).  ``beta = inf``: the best
        position, ties to the lowest, taken only if it gains more than
        ``min_gain``; ``u`` is not read.  -> (pos_out (B, S), ll0 (B,), ll
        (B,), q (B, nvisit), dll (B, nvisit, S), ll_vis (B, nvisit), nmoved
        (B,)): the final orders, the scores of the initial and final states, the
        position each visited node took, each visit's row (exactly 0 at the
        node's own position), the score held after each visit and the number of
        moves taken (fp64 engines only; ``cap`` must cut nothing)."""
        pos = i32(np.atleast_2d(pos))
        b = pos.shape[0]
        w01 = f64(w01).reshape(b, self.S, self.S)
        visit = i32(np.asarray(visit))
        nv = visit.size // max(b, 1)
        visit = visit.reshape(b, nv)
        if u is not None:
            u = f64(u).reshape(b, nv)
        pos_out = np.empty((b, self.S), dtype=np.int32)
        ll0, ll = np.empty(b), np.empty(b)
        q = np.empty((b, nv), dtype=np.int32)
        dll = np.empty((b, nv, self.S))
        ll_vis = np.empty((b, nv))
        nmoved = np.empty(b, dtype=np.int32)
        a = _lib.addr
        check(_lib.load().nemo_order_sweep(self._ctx, b, a(pos), a(w01), nv, a(visit), None if u is None else a(u),
                                           float(beta), float(min_gain), int(cap), a(pos_out), a(ll0), a(ll), a(q),
                                           a(dll), a(ll_vis), a(nmoved)))
        return pos_out, ll0, ll, q, dll, ll_vis, nmoved

    def order_sweep_dev(self, batch, d_pos, d_w01, nvisit, d_visit, d_u, d_pos_out, d_ll, d_ll0=None, d_q=None,
                        d_dll=None, d_ll_vis=None, d_nmoved=None, beta=1.0, min_gain=0.0, cap=0, stream=None):
        """Enqueue ``order_sweep`` on device pointers (no sync; ``reserve`` the
        batch first).  ``d_pos_out`` may be ``d_pos`` (in place); a row that
        holds a NaN leaves its node where it is."""
        check(_lib.load().nemo_order_sweep_dev(self._ctx, int(batch), d_pos, d_w01, int(nvisit), d_visit, d_u,
                                               float(beta), float(min_gain), int(cap), d_pos_out, d_ll0, d_ll, d_q,
                                               d_dll, d_ll_vis, d_nmoved, stream))

    # -- the error rates as parameters ------------------------------------------
    def score_rates(self, pos, w01, A, B, cap: int = 0, want_grad_w: bool = True):
        """Order scores at per-gene error rates, with their derivatives, on an
        engine made by ``from_knockdown`` (fp64, S <= 64): nothing is restaged.

        ``A``, ``B``: A_k = log(alpha_k / (1 - beta_k)) and B_k = log(beta_k /
        (1 - alpha_k)), each a scalar, (S,) or (batch, S).  Returns (ll (B,),
        dA (B, S), dB (B, S), grad (B, S, S) or None): d ll / d A_k, d ll /
        d B_k and d ll / d w01 (exactly 0 off the permissible pairs; w01 is
        not read there).  ``nemo.rates.absolute_ll`` adds the baseline that
        makes ll comparable across rates."""
        pos = i32(np.atleast_2d(pos))
        b = pos.shape[0]
        w01 = f64(w01).reshape(b, self.S, self.S)
        rates = np.empty((b, 2, self.S))
        rates[:, 0] = np.broadcast_to(np.asarray(A, dtype=np.float64), (b, self.S))
        rates[:, 1] = np.broadcast_to(np.asarray(B, dtype=np.float64), (b, self.S))
        ll = np.empty(b)
        dr = np.empty((b, 2, self.S))
        grad = np.empty((b, self.S, self.S)) if want_grad_w else None
        a = _lib.addr
        check(_lib.load().nemo_score_rates(self._ctx, b, a(pos), a(w01), a(rates), int(cap), a(ll), a(dr),
                                           None if grad is None else a(grad)))
        return ll, dr[:, 0].copy(), dr[:, 1].copy(), grad

    def score_rates_dev(self, batch, d_pos, d_w01, d_rates, d_ll, d_drates, d_grad=None, cap=0, stream=None):
        """Enqueue ``score_rates`` on device pointers (no sync; ``reserve`` the
        batch first): rates and drates are (batch, 2, S), the A row then the B
        row; ``d_grad`` may be None."""
        check(_lib.load().nemo_score_rates_dev(self._ctx, int(batch), d_pos, d_w01, d_rates, int(cap), d_ll,
                                               d_drates, d_grad, stream))

    # -- utils.compute_ll / calculate_ll on a given cell matrix ------------
    def lse(self, cells, want_ow=False):
        cells = f64(cells)
        rows = cells.shape[0]
        ll = np.empty(1)
        cs = np.empty(self.E)
        ow = np.empty_like(cells) if want_ow else None
        check(_lib.load().nemo_lse(self._ctx, rows, ptr(cells), ptr(ll), ptr(cs), ptr(ow)))
        return float(ll[0]), cs, ow

    # -- A8 core -------------------------------------------------------------
    def local_opt(self, c, anc, x0):
        c = f64(np.atleast_2d(c))
        n = c.shape[0]
        anc = f64(np.broadcast_to(anc, (n,)))
        x0 = f64(np.broadcast_to(x0, (n,)))
        xs, fs = np.empty(n), np.empty(n)
        nit, nfev, st = (np.empty(n, dtype=np.int32) for _ in range(3))
        check(_lib.load().nemo_local_opt(self._ctx, n, ptr(c), ptr(anc), ptr(x0), ptr(xs), ptr(fs),
                                         ptr(nit, _lib._i32p), ptr(nfev, _lib._i32p),
                                         ptr(st, _lib._i32p)))
        return xs, fs, nit, nfev, st

    # -- A6 fused step -------------------------------------------------------
    def optimal_weights(self, pos, w01, anc, w_prev, sig0, sig1, cap: int = 0, raise_on_fail=True):
        """One get_optimal_weights(init=True, max_iter=1) per chain.

        Returns (w_new, ll1, ll_dag, info): w_new is ``w_prev`` with every
        permissible entry replaced by expit(x*)."""
        call = self.bind_optimal_weights(pos, w01, anc, w_prev, sig0, sig1, cap=cap)
        call.run()
        return call.result(raise_on_fail)

    def bind_optimal_weights(self, pos, w01, anc, w_prev, sig0, sig1, cap: int = 0):
        """``optimal_weights`` in parts: the arguments are converted here;
        ``run()`` is the library call, or ``begin()`` queues it on the library's
        own step thread and ``end()`` waits for it (no Python thread, so no GIL
        hand-over); ``result(raise_on_fail)`` returns what ``optimal_weights``
        returns."""
        return _OptimalWeightsCall(self, pos, w01, anc, w_prev, sig0, sig1, cap)

    @property
    def device_ancestor(self) -> bool:
        """True when the fused step can start from W itself: W~ and
        ancestor_x made on the device in scipy's bits (S <= 64).  The device
        restates scipy's OpenBLAS with its SkylakeX kernels:
        on a host whose scipy selects other kernels, its own inv gives other
        bits, so the sampler inverts on the host there (with a warning)."""
        return self.S <= 64 and host_blas_is_restated()

    def optimal_weights_w(self, pos, w, sig0, sig1, cap: int = 0, raise_on_fail=True, want_prep=True):
        """``optimal_weights`` from the weights themselves: the device makes
        W~ and ancestor_x (nem_order_mcmc.py:98-103, :185) as scipy does.
        Returns (w01, anc, w_new, ll1, ll_dag, info); w01 / anc None with
        ``want_prep=False`` (they stay on the device)."""
        call = self.bind_optimal_weights_w(pos, w, sig0, sig1, cap=cap, want_prep=want_prep)
        call.run()
        try:
            res = call.result(raise_on_fail)
        except AncestorRecompute:
            call.recompute()
            res = call.result(raise_on_fail)
        return (call.w01, call.anc) + res

    def bind_optimal_weights_w(self, pos, w, sig0, sig1, cap: int = 0, want_prep=True):
        """``optimal_weights_w`` in parts, as ``bind_optimal_weights``; the
        call's ``w01`` / ``anc`` hold W~ and ancestor_x once it has ended
        (``want_prep=False``: None, neither leaves the device)."""
        return _OptimalWeightsWCall(self, pos, w, sig0, sig1, cap, want_prep)

    # -- fixed-order optimizers (methods.py) --------------------------------
    def _sweep(self, fn, pos, w, *extra, raise_on_fail=True):
        pos = i32(np.atleast_2d(pos))
        n = pos.shape[0]
        w = f64(w).reshape(n, self.S, self.S)
        w_out = np.empty_like(w)
        ll = np.empty(n)
        info = np.empty((n, self.S, self.S), dtype=np.int32)
        rc = fn(self._ctx, n, ptr(pos, _lib._i32p), ptr(w), *extra, ptr(w_out), ptr(ll),
                ptr(info, _lib._i32p))
        if rc == _lib.NEMO_ERR_OPT and raise_on_fail:
            # the reference raises a plain Exception (methods.py:115, :394)
            raise Exception(_lib.load().nemo_last_error().decode())
        if rc != _lib.NEMO_ERR_OPT:
            check(rc)
        return w_out, ll, info

    def gamma_sweep(self, pos, w, cap: int = 0, raise_on_fail=True):
        """``Method.opt_γ`` (methods.py:397-405) per problem: (w_out, ll, info)."""
        return self._sweep(_lib.load().nemo_gamma_sweep, pos, w, int(cap), raise_on_fail=raise_on_fail)

    def inverse_sweep(self, pos, w, raise_on_fail=True):
        """``InverseMethod.opt_b`` (methods.py:117-129) per problem: (w_out, ll, info)."""
        return self._sweep(_lib.load().nemo_inverse_sweep, pos, w, raise_on_fail=raise_on_fail)

    def real_sweep(self, pos, w):
        """One sweep of ``NEM.compute_real_score``'s fit (nem.py:112-125) per
        problem: the evaluation on ``w``, then every permissible pair's
        bounded solve from 0.5 against the whole order-weight matrix:
        (w_out, ll, info).  A solve's status is in ``info`` only (the
        reference keeps ``res.x`` unchecked).  fp64 engines only."""
        return self._sweep(_lib.load().nemo_real_sweep, pos, w)

    def inverse_ancestral(self, pos, w):
        """unorder_arr(order, B/(1+B)), B = (I - order_arr(order, exp(w)))^-1 lower
        (methods.py:118-121, :160-164), per problem."""
        pos = i32(np.atleast_2d(pos))
        n = pos.shape[0]
        w = f64(w).reshape(n, self.S, self.S)
        out = np.empty_like(w)
        check(_lib.load().nemo_inverse_ancestral(self._ctx, n, ptr(pos, _lib._i32p), ptr(w), ptr(out)))
        return out

    def order_weights(self, chain: int = 0) -> np.ndarray:
        out = np.empty((self.S + 1, self.E))
        check(_lib.load().nemo_fetch_order_weights(self._ctx, int(chain), ptr(out)))
        return out

    def set_option(self, name: str, value: int):
        check(_lib.load().nemo_set_option(self._ctx, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_int32(0)
        check(_lib.load().nemo_get_option(self._ctx, name.encode(), C.byref(v)))
        return v.value

    def set_option_f64(self, name: str, value: float):
        check(_lib.load().nemo_set_option_f64(self._ctx, name.encode(), float(value)))

    def get_option_f64(self, name: str) -> float:
        v = C.c_double(0.0)
        check(_lib.load().nemo_get_option_f64(self._ctx, name.encode(), C.byref(v)))
        return v.value

    def score_kernel(self, cap: int = 0, ll_only: bool = True):
        """(fact_kernel, worst-case |ll error| bound) a factored score call
        with this cap takes; fact_kernel -1 = the streaming kernel."""
        fk = C.c_int32(0)
        b = C.c_double(0.0)
        check(_lib.load().nemo_score_kernel(self._ctx, int(cap), 1 if ll_only else 0, C.byref(fk),
                                            C.byref(b)))
        return fk.value, b.value

    def exact_limits(self, cap: int = 0):
        """The reference-arithmetic path's limits for this model
        (``nemo.limits``: one row per limit, the model's value, whether it is
        covered and what the sampler does outside it)."""
        from .limits import exact_limits
        return exact_limits(self.S, self.E, self.factored, cap, host_blas_arch(),
                            exact_option=bool(self.get_option("exact")),
                            exact_generic=bool(self.get_option("exact_generic")),
                            row_shared=bool(self.get_option("exact_shared")))

    def exact_status(self, cap: int = 0):
        """(True, "") when the fused step and the sampler's score calls run in
        the reference's own arithmetic (option ``exact``, the default, on a
        model the exact kernels cover); else (False, the limit that breaks it
        and what runs instead) -- the rows of ``exact_limits``."""
        from .limits import exact_status_from
        ok, why = exact_status_from(self.exact_limits(cap))
        # the library's own verdict on the staging (the wave plan it built)
        if ok and not self.get_option("exact_ok"):
            if not self.factored:
                from .limits import MAX_ABS_T_EXACT_GENERIC, MAX_ABS_U_EXACT_GENERIC
                return False, ("table form: the staged generic table is outside option exact_generic's bounds "
                               f"(max|T| <= {MAX_ABS_T_EXACT_GENERIC:g} and max|U| <= {MAX_ABS_U_EXACT_GENERIC:g}); "
                               "the fast kernels")
            return False, f"E={self.E}: the staging found no wave plan for numpy's pairwise sum; the fast kernels"
        return ok, why

    @property
    def factored(self) -> bool:
        """True when the staged table has the NEM structure the MFMA kernel uses."""
        return bool(self.get_option("factored"))

    # -- timing of the score kernel ------------------------------------------
    def timing(self, enable: bool):
        check(_lib.load().nemo_timing_enable(self._ctx, 1 if enable else 0))

    def timing_read(self):
        ms = C.c_double(0.0)
        n = C.c_int32(0)
        check(_lib.load().nemo_timing_read(self._ctx, C.byref(ms), C.byref(n)))
        return ms.value, n.value


_HOST_BLAS = None


def host_blas_arch():
    """The architecture of the OpenBLAS kernels scipy.linalg runs on this
    host (threadpoolctl), or None when it cannot be told."""
    global _HOST_BLAS
    if _HOST_BLAS is None:
        arch = ""
        try:
            import scipy.linalg  # noqa: F401  (loads its OpenBLAS)
            from threadpoolctl import threadpool_info
            for p in threadpool_info():
                if p.get("internal_api") == "openblas" and "scipy" in p.get("filepath", ""):
                    arch = p.get("architecture") or ""
                    break
        except Exception:  # threadpoolctl absent: cannot tell
            arch = ""
        _HOST_BLAS = arch
    return _HOST_BLAS or None


def host_blas_is_restated() -> bool:
    """True when scipy's OpenBLAS on this host runs the SkylakeX kernels the
    device's getrf / getri restate (csrc/nemo_ancestor.hip), or when the host
    cannot be told (then with a warning: the device's bits are SkylakeX's)."""
    import warnings
    arch = host_blas_arch()
    if arch == "SkylakeX":
        return True
    if arch is None:
        warnings.warn("cannot tell which OpenBLAS kernels scipy runs on this host (threadpoolctl): the device's "
                      "ancestor_x has the bits of scipy's SkylakeX kernels", ExactArithmeticWarning, stacklevel=3)
        return True
    warnings.warn(f"scipy's OpenBLAS runs {arch} kernels on this host, not the SkylakeX kernels the device's "
                  "ancestor_x restates: ancestor_x is made on the host (scipy.linalg.inv)",
                  ExactArithmeticWarning, stacklevel=3)
    return False


_LSE_ENGINES = {}


def lse_ll(cells: np.ndarray, device: int = 0) -> float:
    """sum_e logsumexp over rows, on the GPU (utils.compute_ll)."""
    cells = f64(cells)
    rows, e = cells.shape
    eng = _LSE_ENGINES.get((e, device))
    if eng is None:
        eng = _LseEngine(e, device)
        _LSE_ENGINES[(e, device)] = eng
    return eng.ll(cells)


class _LseEngine:
    """A table-less context used only for the LSE kernel."""

    def __init__(self, E, device):
        lib = _lib.load()
        self.E = E
        self._ctx = C.c_void_p()
        check(lib.nemo_ctx_create(device, 2, E, _lib.NEMO_F64, C.byref(self._ctx)))
        self._fin = weakref.finalize(self, lib.nemo_ctx_destroy, self._ctx)

    def ll(self, cells, want=False):
        rows = cells.shape[0]
        ll = np.empty(1)
        cs = np.empty(self.E)
        ow = np.empty_like(cells) if want else None
        check(_lib.load().nemo_lse(self._ctx, rows, ptr(cells), ptr(ll), ptr(cs), ptr(ow)))
        if want:
            return float(ll[0]), cs, ow
        return float(ll[0])


def lse_full(cells: np.ndarray, device: int = 0):
    """(ll, cs, order_weights) of a given cell matrix, on the GPU."""
    cells = f64(cells)
    e = cells.shape[1]
    eng = _LSE_ENGINES.get((e, device))
    if eng is None:
        eng = _LseEngine(e, device)
        _LSE_ENGINES[(e, device)] = eng
    return eng.ll(cells, want=True)


class _OptimalWeightsCall:
    __slots__ = ("w_new", "ll1", "lld", "info", "_keep", "_fn", "_args", "rc")

    def __init__(self, eng: Engine, pos, w01, anc, w_prev, sig0, sig1, cap):
        pos = i32(np.atleast_2d(pos))
        n, s = pos.shape[0], eng.S
        w01 = f64(w01).reshape(n, s, s)
        anc = f64(anc).reshape(n, s, s)
        self.w_new = np.array(w_prev, dtype=np.float64, copy=True).reshape(n, s, s)
        self.ll1, self.lld = np.empty(n), np.empty(n)
        self.info = np.empty((n, s, s), dtype=np.int32)
        self._keep = (pos, w01, anc)
        self._fn = _lib.load().nemo_optimal_weights
        # (the arrays stay referenced by this object for the call's lifetime)
        a = _lib.addr
        self._args = (eng._ctx, n, a(pos), a(w01), a(anc), float(sig0), float(sig1),
                      int(cap), a(self.w_new), a(self.ll1), a(self.lld), a(self.info))
        self.rc = None

    def run(self):
        self.rc = self._fn(*self._args)

    def begin(self):
        """Queue the call on the library's step thread and return at once."""
        check(_lib.load().nemo_optimal_weights_begin(*self._args))

    def end(self):
        """Wait for the oldest queued call (this one, when begun and ended in order)."""
        self.rc = _lib.load().nemo_optimal_weights_end(self._args[0])

    def result(self, raise_on_fail=True):
        rc = self.rc
        if rc == _lib.NEMO_ERR_OPT and not raise_on_fail:
            return self.w_new, self.ll1, self.lld, self.info
        if rc == _lib.NEMO_ERR_OPT:
            # the reference raises a plain Exception (nem_order_mcmc.py:168-169)
            raise Exception(_lib.load().nemo_last_error().decode())
        check(rc)
        return self.w_new, self.ll1, self.lld, self.info


class AncestorRecompute(_lib.NemoError):
    """The device's ancestor_x met a non-finite intermediate value, where its
    restatement is not held to scipy's bits: the step is to be recomputed with
    the host's W~ / ancestor_x (``_OptimalWeightsWCall.recompute``)."""


class _OptimalWeightsWCall:
    """``nemo_optimal_weights_w``: W in; W~, ancestor_x and the step out."""
    __slots__ = ("eng", "pos", "w", "w01", "anc", "flag", "w_new", "ll1", "lld", "info", "cap", "sig",
                 "_args", "rc", "ended")

    def __init__(self, eng: Engine, pos, w, sig0, sig1, cap, want_prep=True):
        self.eng = eng
        self.pos = i32(np.atleast_2d(pos))
        n, s = self.pos.shape[0], eng.S
        self.w = f64(w).reshape(n, s, s)
        self.w_new = np.array(self.w, copy=True)
        self.w01, self.anc = (np.empty((n, s, s)), np.empty((n, s, s))) if want_prep else (None, None)
        self.flag = np.zeros(n, dtype=np.int32)
        self.ll1, self.lld = np.empty(n), np.empty(n)
        self.info = np.empty((n, s, s), dtype=np.int32)
        self.cap, self.sig = int(cap), (float(sig0), float(sig1))
        a = _lib.addr
        self._args = (eng._ctx, n, a(self.pos), a(self.w), float(sig0), float(sig1), int(cap),
                      None if self.w01 is None else a(self.w01), None if self.anc is None else a(self.anc),
                      a(self.w_new), a(self.ll1), a(self.lld), a(self.info), a(self.flag))
        self.rc, self.ended = None, False

    def run(self):
        self.rc = _lib.load().nemo_optimal_weights_w(*self._args)
        self.ended = True

    def begin(self):
        check(_lib.load().nemo_optimal_weights_w_begin(*self._args))

    def end(self):
        if not self.ended:
            self.rc = _lib.load().nemo_optimal_weights_end(self._args[0])
            self.ended = True

    def recompute(self):
        """The step again with W~ and ancestor_x made on the host (scipy's
        expit and inv: chains.inv_stack), synchronously -- no other call may
        be queued on the engine."""
        from .chains import inv_stack
        sig = self.host_w01()
        eye = np.identity(self.eng.S)
        self.w01 = sig
        self.anc = np.clip(inv_stack(eye - sig) - eye, 0, 1)
        self.flag[:] = 0
        call = _OptimalWeightsCall(self.eng, self.pos, self.w01, self.anc, self.w, *self.sig, self.cap)
        call.run()
        self.w_new, self.ll1, self.lld, self.info, self.rc = call.w_new, call.ll1, call.lld, call.info, call.rc

    def host_w01(self):
        """W~ as the host makes it (scipy's expit on the permissible entries)."""
        from scipy.special import expit

        from .nem_order_mcmc import permissible_batch
        mask = permissible_batch(self.pos, self.cap)
        sig = self.w.copy()
        sig[mask] = expit(self.w[mask])
        return sig

    def result(self, raise_on_fail=True):
        if self.rc == _lib.NEMO_ERR_LINALG:
            from scipy.linalg import inv
            eye = np.identity(self.eng.S)
            w01 = self.w01 if self.w01 is not None else self.host_w01()
            for k in np.nonzero(self.flag)[0]:
                if self.flag[k] & 3:   # scipy.linalg.inv's own error (LinAlgError / ValueError)
                    inv(eye - w01[k])
            raise AncestorRecompute(self.rc, _lib.load().nemo_last_error().decode())
        rc = self.rc
        if rc == _lib.NEMO_ERR_OPT and not raise_on_fail:
            return self.w_new, self.ll1, self.lld, self.info
        if rc == _lib.NEMO_ERR_OPT:
            raise Exception(_lib.load().nemo_last_error().decode())
        check(rc)
        return self.w_new, self.ll1, self.lld, self.info
