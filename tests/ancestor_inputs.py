"""Inputs for the device inverse (ancestor_kernel, csrc/nemo_ancestor.hip):
(pos, W, cap) batches for every S from 2 to 64, from fixed seeds.

The kernel's control flow is a function of S (panel widths, trsm row blocks,
gemm accumulation classes, the ``rows & 3`` tails of dgemv_n), and its
branch-free phases and its pivot search rest on properties of the values
(ties, exact zeros and ones, subnormals, the sign of a zero).  So per S the
list holds these families of ``CHAINS`` chains each, at cap 0 and, from
S >= 5, at cap 3:

* ``sat``: permissible W from {-800, 0, 40, 40}: expit gives exactly 0, 1/2
  and 1; nothing stale, zero diagonal.  I - W~ is a permuted unit triangle of
  0 / -1/2 / -1: always invertible, full of pivot ties;
* ``few``: permissible W from {0, 40, log(1/3)};
* ``edge``: permissible W from {-745, -720, -709, 36.7, 37, 1}: subnormal W~,
  the last value below 1 and exactly 1;
* ``wide``: permissible W uniform(-40, 40);
* ``sat_stale``: ``sat`` plus stale entries from {1, 1/2} on 15 % of the
  other places (some of these are singular, which is wanted);
* ``signed_stale``: permissible W uniform(-4, 4), stale entries uniform(-3, 3)
  and a diagonal of uniform(-0.5, 0.5);
* ``orders``: the identity and the reversed order with every permissible W
  40, and with every one -800 (four chains).  The caps 1, S - 2, S - 1 and
  S + 5 run on these four chains only.

``overflow(s)`` is one chain whose inverse overflows: the identity order,
every permissible W -800 (W~ exactly 0) and stale entries of 1e200 at (0, 1)
and (1, 2), so inv(U) holds 1e400.

``singular(s)`` holds three chains with a zero column in I - W~ (a node
that is last in its order, so nobody's parent, with a stale 1 on its own
diagonal entry) at columns 1, S // 2 + 1 and S - 1: getrf meets its zero pivot
at exactly that column, in the first, a middle and the last panel.

``tiny_pivot(s)`` holds eight chains, at cap 0 of every S, whose factorisation
meets a non-zero pivot below DBL_MIN: ``edge`` weights, and a node that is
first in its order with a stale 1 on its own diagonal entry and weights of
-709 / -720 to all its children, so its column of I - W~ holds 0 on the
diagonal and -1.2e-308 / -2e-313 elsewhere.  OpenBLAS's getf2 records such a
pivot but neither swaps it in nor scales by it; the inverse that follows is
finite, overflows, or ends in getri's LinAlgError (a zero left on U's
diagonal), chain by chain.  The node is label 0, S // 2, S - 1 and five random ones; it has stale
entries of 1 / 1/2 in its own row, which put a non-zero value below DBL_MIN
on its diagonal place as the earlier columns are eliminated.

Plain numpy, no GPU and no library: tests/test_ancestor_inputs_cpu.py checks
what the list covers, tests/test_gpu_ancestor.py runs the kernel on it.
"""
from __future__ import annotations

import functools

import numpy as np
from scipy.linalg import inv

SIZES = tuple(range(2, 65))
CHAINS = 8
FAMILIES = ("sat", "few", "edge", "wide", "sat_stale", "signed_stale", "orders")
OVERFLOW_SIZES = (3, 33, 64)
SINGULAR_SIZES = (7, 40, 64)
SEED = 20251

_SAT = np.array([-800.0, 0.0, 40.0, 40.0])
_FEW = np.array([0.0, 40.0, np.log(1.0 / 3.0)])
_EDGE = np.array([-745.0, -720.0, -709.0, 36.7, 37.0, 1.0])
_STALE = np.array([1.0, 0.5])


def caps(s):
    """The caps every family runs under."""
    return (0, 3) if s >= 5 else (0,)


def order_caps(s):
    """The caps of the ``orders`` family alone (beside ``caps``)."""
    return tuple(c for c in dict.fromkeys((1, s - 2, s - 1, s + 5)) if c > 0 and c not in caps(s))


def all_caps(s):
    return caps(s) + order_caps(s)


def mask(pos, cap=0):
    """mask[c, i, k]: k is a permissible parent of i in order c."""
    p = np.asarray(pos, dtype=np.int64)
    gap = p[:, :, None] - p[:, None, :]
    return (gap > 0) & (gap <= cap) if cap else gap > 0


def _orders(s, cap):
    ident = np.arange(s, dtype=np.int32)
    pos = np.stack([ident, ident[::-1], ident, ident[::-1]])
    m = mask(pos, cap)
    w = np.zeros((4, s, s))
    w[:2][m[:2]] = 40.0
    w[2:][m[2:]] = -800.0
    return pos, w


def _family(name, s, cap):
    rng = np.random.default_rng([SEED, s, cap, FAMILIES.index(name)])
    n = CHAINS
    pos = np.array([rng.permutation(s) for _ in range(n)], dtype=np.int32)
    m = mask(pos, cap)
    shape = (n, s, s)
    if name in ("sat", "sat_stale"):
        w = np.where(m, _SAT[rng.integers(_SAT.size, size=shape)], 0.0)
        if name == "sat_stale":
            stale = ~m & (rng.random(shape) < 0.15)
            w = np.where(stale, _STALE[rng.integers(_STALE.size, size=shape)], w)
            for k in range(n):
                np.fill_diagonal(w[k], 0.0)
    elif name == "few":
        w = np.where(m, _FEW[rng.integers(_FEW.size, size=shape)], 0.0)
    elif name == "edge":
        w = np.where(m, _EDGE[rng.integers(_EDGE.size, size=shape)], 0.0)
    elif name == "wide":
        w = np.where(m, rng.uniform(-40.0, 40.0, shape), 0.0)
    elif name == "signed_stale":
        w = np.where(m, rng.uniform(-4.0, 4.0, shape), 0.0)
        w = np.where(~m & (rng.random(shape) < 0.15), rng.uniform(-3.0, 3.0, shape), w)
        for k in range(n):
            np.fill_diagonal(w[k], rng.uniform(-0.5, 0.5, s))
    else:
        raise KeyError(name)
    return pos, w


def overflow(s):
    """(pos (1, S), W (1, S, S)) of the overflowing chain."""
    pos = np.arange(s, dtype=np.int32)[None]
    w = np.where(mask(pos), -800.0, 0.0)
    w[0, 0, 1] = w[0, 1, 2] = 1e200
    return pos, w


def singular_columns(s):
    return (1, s // 2 + 1, s - 1)


def singular(s):
    """(pos (3, S), W (3, S, S)): ``sat`` weights with column k of I - W~ zero."""
    rng = np.random.default_rng([SEED, s, 0, 99])
    cols = singular_columns(s)
    pos = np.array([rng.permutation(s) for _ in cols], dtype=np.int32)
    for c, k in enumerate(cols):   # node k goes last
        pos[c, np.argmax(pos[c])] = pos[c, k]
        pos[c, k] = s - 1
    w = np.where(mask(pos), _SAT[rng.integers(_SAT.size, size=(len(cols), s, s))], 0.0)
    for c, k in enumerate(cols):
        w[c, k, k] = 1.0
    return pos, w


def tiny_pivot(s):
    """(pos (8, S), W (8, S, S)) of the chains with a pivot below DBL_MIN."""
    rng = np.random.default_rng([SEED, s, 0, 98])
    nodes = (0, s // 2, s - 1) + tuple(int(v) for v in rng.integers(s, size=CHAINS - 3))
    pos = np.array([rng.permutation(s) for _ in nodes], dtype=np.int32)
    for c, k in enumerate(nodes):   # node k goes first
        pos[c, np.argmin(pos[c])] = pos[c, k]
        pos[c, k] = 0
    w = np.where(mask(pos), _EDGE[rng.integers(_EDGE.size, size=(len(nodes), s, s))], 0.0)
    for c, k in enumerate(nodes):
        w[c, k, :] = np.where(rng.random(s) < 0.5, rng.choice(_STALE, size=s), 0.0)   # stale: k has no parents
        w[c, :, k] = np.where(np.arange(s) == k, 1.0, rng.choice([-709.0, -720.0], size=s))
    return pos, w


@functools.lru_cache(maxsize=None)
def batch(s, cap):
    """(pos (n, S) int32, W (n, S, S), labels): every chain that runs at
    (S, cap) in one stack; labels[k] = (family, index in the family).  The
    overflowing chain rides at cap 0 of ``OVERFLOW_SIZES`` as ("overflow", 0), the
    zero-column chains at cap 0 of ``SINGULAR_SIZES`` as ("singular", j), the
    chains with a pivot below DBL_MIN at cap 0 of every S as ("tiny_pivot", j)."""
    parts, labels = [], []
    if cap in caps(s):
        for name in FAMILIES[:-1]:
            parts.append(_family(name, s, cap))
            labels += [(name, k) for k in range(CHAINS)]
    parts.append(_orders(s, cap))
    labels += [("orders", k) for k in range(4)]
    if cap == 0 and s in OVERFLOW_SIZES:
        parts.append(overflow(s))
        labels.append(("overflow", 0))
    if cap == 0:
        parts.append(tiny_pivot(s))
        labels += [("tiny_pivot", j) for j in range(CHAINS)]
    if cap == 0 and s in SINGULAR_SIZES:
        parts.append(singular(s))
        labels += [("singular", j) for j in range(3)]
    pos = np.ascontiguousarray(np.concatenate([p for p, _ in parts]), dtype=np.int32)
    w = np.ascontiguousarray(np.concatenate([x for _, x in parts]))
    pos.setflags(write=False)
    w.setflags(write=False)
    return pos, w, tuple(labels)


def family(name, s, cap):
    """(pos, W) of one family's chains at (S, cap)."""
    pos, w, labels = batch(s, cap)
    idx = [k for k, (f, _) in enumerate(labels) if f == name]
    return pos[idx], w[idx]


def classify(host, pos, w, cap):
    """Every chain through ``host(pos, W, cap)`` (the reference's own calls) on
    its own: a list of (class, W~, ancestor_x) with class "a" when inv raises
    LinAlgError (W~ and ancestor_x None), "b" when the inverse is finite, "c"
    when it is not and nothing is raised."""
    out = []
    for k in range(pos.shape[0]):
        try:
            with np.errstate(all="ignore"):
                sig, anc = host(pos[k:k + 1], w[k:k + 1].copy(), cap)
        except np.linalg.LinAlgError:
            out.append(("a", None, None))
            continue
        # clip hides an infinity: the class is that of the inverse itself
        with np.errstate(all="ignore"):
            fin = bool(np.isfinite(inv(np.identity(w.shape[-1]) - sig[0])).all())
        out.append(("b" if fin else "c", sig[0], anc[0]))
    return out


@functools.lru_cache(maxsize=None)
def classified(host, s, cap):
    """``classify`` of ``batch(s, cap)``, computed once."""
    pos, w, _ = batch(s, cap)
    return tuple(classify(host, pos, w, cap))


def lu_stats(a):
    """A plain partial-pivot LU (first largest |.|, as idamax) of one matrix:
    (ties, negative_swaps, zero_col): the columns whose pivot search met two or
    more equal maxima, the row swaps whose chosen pivot is negative, and the
    first column with a zero pivot (None when there is none; the elimination
    goes on past it, as getrf's does)."""
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    ties = neg = 0
    zero_col = None
    with np.errstate(all="ignore"):
        for j in range(n):
            col = np.abs(a[j:, j])
            p = int(np.argmax(col))
            if col[p] > 0 and int((col == col[p]).sum()) >= 2:
                ties += 1
            if col[p] == 0:
                if zero_col is None:
                    zero_col = j
                continue
            if p:
                neg += a[j + p, j] < 0
                a[[j, j + p]] = a[[j + p, j]]
            a[j + 1:, j] /= a[j, j]
            a[j + 1:, j + 1:] -= np.outer(a[j + 1:, j], a[j, j + 1:])
    return ties, int(neg), zero_col
