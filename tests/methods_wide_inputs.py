"""Inputs of the wide fixed-order optimizer fixtures (methods_wide_*.npz),
shared by the maker (golden/make_methods_wide_goldens.py), the CPU fixture
test and the GPU tests: the fixture table, the starting weights rebuilt from
their seeds, the coverage conditions every fixture must meet, and the
``minimize`` spy that records each pair's (nit, nfev).

A fixture model is ``generator.synthetic_nem(S, E, model_seed)``; it is the
smallest that reaches an instantiation of nemo_methods.hip no other test runs:

    65 x 70    column_solve<2> at its lower edge (S = 65), NPL = 4
    96 x 600   column_solve<2> with columns longer than one 64-row slot, NPL = 16
    160 x 600  column_solve<4> with rows in the third slot, NPL = 16

Names: ``order[p]`` = the node at position p (what methods.py takes),
``pos = argsort(order)``.  order_arr (utils.py:173) puts node ``pos[a]`` at
matrix index a, so node i sits at index ``order[i]``: the column solve of pair
(i, k) runs over the indices order[k] .. order[i].  Two spans are counted per
moved pair: ``pos[i] - pos[k]`` (the distance in the order) and
``order[i] - order[k]`` (the length of the device's column solve).
"""
from __future__ import annotations

import numpy as np

# name -> S, E, model seed, order seed, gamma start seed, inverse start seed, inverse start density
FIXTURES = {
    "65x70": dict(S=65, E=70, model_seed=3, order_seed=13, gamma_seed=23, inverse_seed=33, density=0.1),
    "96x600": dict(S=96, E=600, model_seed=4, order_seed=16, gamma_seed=24, inverse_seed=42, density=0.1),
    "160x600": dict(S=160, E=600, model_seed=5, order_seed=18, gamma_seed=25, inverse_seed=53, density=0.06),
}

# moved inverse pairs a fixture must hold: (at all, span >= 64, span >= 128)
INVERSE_MOVED_MIN = {"65x70": (30, 0, 0), "96x600": (30, 20, 0), "160x600": (30, 50, 10)}
GAMMA_MOVED_SHARE_MIN = 0.5


def positions(order):
    order = np.asarray(order)
    pos = np.empty(len(order), dtype=np.int32)
    pos[order] = np.arange(len(order))
    return pos


def pair_list(order):
    """The permissible pairs (i, k) in the loop order of opt_γ / opt_b
    (methods.py:401-403, :125-127): i ascending, k along the order prefix."""
    order = np.asarray(order)
    pos = positions(order)
    ii = np.concatenate([np.full(pos[i], i, dtype=np.int64) for i in range(len(order))])
    kk = np.concatenate([order[:pos[i]].astype(np.int64) for i in range(len(order))])
    return ii, kk


def draw_order(s, seed):
    return np.random.default_rng(seed).permutation(s)


def gamma_start(order, seed):
    """uniform(0, 1) on the permissible pairs (drawn in loop order), 0 elsewhere."""
    s = len(order)
    ii, kk = pair_list(order)
    w = np.zeros((s, s))
    w[ii, kk] = np.random.default_rng(seed).uniform(0.0, 1.0, len(ii))
    return w


def inverse_start(order, seed, density, lo=-3.0, hi=0.0):
    """A sparse DAG of log-weights: every permissible pair is set with
    probability ``density`` to uniform(lo, hi); the rest stay at -5000."""
    s = len(order)
    ii, kk = pair_list(order)
    rng = np.random.default_rng(seed)
    on = rng.random(len(ii)) < density
    val = rng.uniform(lo, hi, len(ii))
    w = np.full((s, s), -5000.0)
    w[ii[on], kk[on]] = val[on]
    return w


def fixture_starts(name, order):
    f = FIXTURES[name]
    return gamma_start(order, f["gamma_seed"]), inverse_start(order, f["inverse_seed"], f["density"])


def moved_spans(order, start, new):
    """(pos[i] - pos[k], order[i] - order[k]) of the permissible pairs whose
    weight the sweep changed."""
    order = np.asarray(order).astype(np.int64)
    pos = positions(order).astype(np.int64)
    ii, kk = pair_list(order)
    mv = start[ii, kk] != new[ii, kk]
    return pos[ii[mv]] - pos[kk[mv]], order[ii[mv]] - order[kk[mv]], len(ii)


def check_coverage(name, order, gamma_w0, gamma_w, inverse_w0, inverse_w):
    """The conditions on a fixture's captured reference output; raises
    AssertionError with the counts when one fails.  Returns the counts."""
    g_span, _, npairs = moved_spans(order, gamma_w0, gamma_w)
    g_moved = len(g_span)
    assert g_moved >= GAMMA_MOVED_SHARE_MIN * npairs, (name, "gamma moved", g_moved, npairs)
    span, kspan, _ = moved_spans(order, inverse_w0, inverse_w)
    n_all, n64, n128 = INVERSE_MOVED_MIN[name]
    counts = dict(gamma_moved=g_moved, pairs=npairs, inverse_moved=len(span),
                  span64=int((span >= 64).sum()), span128=int((span >= 128).sum()),
                  solve64=int((kspan >= 64).sum()), solve128=int((kspan >= 128).sum()))
    assert counts["inverse_moved"] >= n_all, (name, counts)
    # the issue's condition (distance in the order) and the same counts on the
    # length of the device's column solve, which is what crosses the slots
    assert counts["span64"] >= n64 and counts["span128"] >= n128, (name, counts)
    assert counts["solve64"] >= n64 and counts["solve128"] >= n128, (name, counts)
    return counts


class MinimizeSpy:
    """Wraps scipy's ``minimize``: the calls' (nit, nfev, success) in call
    order, which is the loop order of ``pair_list``."""

    def __init__(self, real):
        self.real = real
        self.nit, self.nfev, self.ok = [], [], []

    def __call__(self, fun, x0, *a, **kw):
        r = self.real(fun, x0, *a, **kw)
        self.nit.append(int(r.nit))
        self.nfev.append(int(r.nfev))
        self.ok.append(bool(r.success))
        return r

    def dense(self, order):
        """(nit, nfev) as (S, S) arrays, -1 off the permissible pairs."""
        s = len(order)
        ii, kk = pair_list(order)
        assert len(self.nit) == len(ii)
        nit = np.full((s, s), -1, dtype=np.int32)
        nfev = np.full((s, s), -1, dtype=np.int32)
        nit[ii, kk] = self.nit
        nfev[ii, kk] = self.nfev
        return nit, nfev
