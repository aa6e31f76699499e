"""numpy / scipy statement of the true-graph fit (``NEM.compute_real_score``).

Written from the description of the procedure, on plain tables: ``U`` (S+1, E),
``T`` (S, S, E) and the S-genes' order.  It is the CPU reference of
``nemo_real_sweep`` for models the reference programme cannot take (a generic
table), and ``test_real_score_cpu.py`` holds it to the recorded sweeps of the
reference programme bit for bit, so the elementwise operations below keep
that programme's order of operations:

* cells[i] = U[i] + sum over the parents j of i, in order, of
  log(1 - w + w exp(T[i][j])); cs = logaddexp.reduce(cells); order weights
  exp(cells - cs); ll = the sequential sum of cs;
* per permissible pair: a = (exp(T[i][j]) - 1) * order_weights (the whole
  matrix), b = 1 - w a + w (exp(T[i][j]) - 1), c = a / b, then
  minimize(-sum log(c x + 1), 0.5, bounds [(0, 1)], L-BFGS-B, tol 0.1);
* sweeps while ll - old_ll > 1e-4 (signed), at most 1000; the weights kept
  are the last sweep's.
"""
from __future__ import annotations

import numpy as np
from scipy.optimize import minimize


def neg_log_sum(x, c):
    return -np.sum(np.log(c * x + 1.0))


def positions(order):
    order = np.asarray(order)
    pos = np.empty(len(order), dtype=np.int32)
    pos[order] = np.arange(len(order), dtype=np.int32)
    return pos


def pair_list(order):
    """The permissible (child, parent) pairs in solve order: children 0..S-1,
    each with the S-genes before it in ``order``, in ``order``'s order."""
    order = np.asarray(order)
    pos = positions(order)
    return [(i, int(j)) for i in range(len(order)) for j in order[:pos[i]]]


def evaluate(U, T, order, W):
    """(ll, order_weights) at the weights W[i][j] of the permissible pairs."""
    cells = np.array(U, dtype=np.float64, copy=True)
    for i, j in pair_list(order):
        w = W[i, j]
        cells[i, :] += np.log(1.0 - w + w * np.exp(T[i][j]))
    cs = np.logaddexp.reduce(cells, axis=0)
    ow = np.exp(cells - cs)
    return sum(cs), ow


def initial_gradient(c, objective=neg_log_sum):
    """scipy's forward difference at x0 = 0.5 (step 1e-8, inside [0, 1])."""
    x0 = 0.5
    x1 = x0 + 1e-8
    return (objective(np.array([x1]), c) - objective(np.array([x0]), c)) / (x1 - x0)


def sweep(U, T, order, W, objective=neg_log_sum):
    """One sweep from the weights W: (ll, W_out, nit, g0, status) with nit /
    g0 / status per pair in ``pair_list`` order (status 0 = success)."""
    ll, ow = evaluate(U, T, order, W)
    out = np.array(W, dtype=np.float64, copy=True)
    nit, g0, status = [], [], []
    for i, j in pair_list(order):
        lv = np.exp(T[i][j])
        w = W[i, j]
        a = (lv - 1.0) * ow
        b = 1.0 - w * a + w * (lv - 1.0)
        c = a / b
        res = minimize(objective, x0=0.5, bounds=[(0.0, 1.0)], args=(c,), method="L-BFGS-B", tol=0.1)
        out[i, j] = res.x[0]
        nit.append(res.nit)
        status.append(res.status)
        g0.append(float(initial_gradient(c, objective)))
    return float(ll), out, np.array(nit), np.array(g0), np.array(status)


def start_weights(order):
    pos = positions(order)
    return np.where(pos[None, :] < pos[:, None], 0.5, 0.0)


def fit(U, T, order, max_iter=1000, objective=neg_log_sum):
    """The sweeps from 0.5: dict of ``ll`` (n,), ``w`` (n, S, S) weights after
    each sweep, ``nit`` / ``g0`` (n, pairs)."""
    W = start_weights(order)
    lls, ws, nits, g0s = [], [], [], []
    ll_diff, old_ll, count = float("inf"), -float("inf"), 0
    while ll_diff > 0.0001 and count < max_iter:
        ll, W, nit, g0, _ = sweep(U, T, order, W, objective)
        ll_diff = ll - old_ll
        old_ll = ll
        count += 1
        lls.append(ll)
        ws.append(W)
        nits.append(nit)
        g0s.append(g0)
    return {"ll": np.array(lls), "w": np.array(ws), "nit": np.array(nits), "g0": np.array(g0s)}


def parent_order_of(adj):
    adj = np.array(adj, copy=True)
    np.fill_diagonal(adj, 0)
    return np.argsort(np.sum(adj, axis=1))[::-1]


def real_score(U, T, adj, max_iter=1000):
    """(real_order_ll, real_ll, parent_order, fit) for the adjacency ``adj``
    (adj[i][j] == 1: i is a parent of j)."""
    adj = np.array(adj, copy=True)
    np.fill_diagonal(adj, 0)
    order = parent_order_of(adj)
    f = fit(U, T, order, max_iter)
    pos = positions(order)
    mask = pos[None, :] < pos[:, None]
    rounded = np.where(mask, 1.0 * (f["w"][-1] > 0.5), 0.0)
    order_ll, _ = evaluate(U, T, order, rounded)
    # the adjacency's own parent sets at weight 1, parents in ascending index
    cells = np.array(U, dtype=np.float64, copy=True)
    for i in range(adj.shape[0]):
        for j in range(adj.shape[0]):
            if adj[i][j] == 1:
                cells[j, :] += np.log(1.0 - 1.0 + 1.0 * np.exp(T[j][i]))
    real_ll = sum(np.logaddexp.reduce(cells, axis=0))
    return float(order_ll), float(real_ll), order, f
