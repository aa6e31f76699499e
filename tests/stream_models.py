"""Inputs and the long-double reference for the streaming and grouped score
kernels (score_kernel<TT, RENORM>, score_group_kernel<TT, CB, GW, RENORM>,
prep_kernel, prep_group_kernel, finalize_kernel; csrc/nemo_kernels.hip).

Every table here is real-valued (not factorable), in the two kinds of
tests/golden/generic_tables.py -- "shared": T[i][j] = R[j] for every child,
U = [R; 0]; "own": every row its own -- and made from a seed:

* amplitude tables: entries uniform in [-a, a] with one entry equal to a, the
  amplitudes on each side of every threshold of the launchers' dispatch
  (``needs_renorm``, ``wide_table``, restated here as ``renorm``);
* range tables (S = 64, E = 130, |T| <= 15): in columns 0..39 every T is in
  [10, 15], in columns 40..79 in [-15, -10], so that the child with 63
  parents has a product past e^710 and below e^-745; in the negative band its
  own U cancels the sum of its row, so that at weights 1 under the identity
  order its cell is within 20 of its column's maximum -- a product that is
  not renormalised loses a cell that decides cs and ll.

``CASES`` names a (dtype, kind, S, E, a) with the caps it runs under, the way
the table reaches the streaming kernel and the RENORM it must select.  The
evaluations of a case (``evals``) are fixed_point_models.inputs' nine (random
orders, the identity and its reverse against soft, saturated, all 0, all 1
and coin-flip weights) plus three with "edge mix" weights drawn from {0, 2^-60,
0.5, 1 - 1e-6, 1 - 1e-9, 1 - 2^-53, 1}; ``refs`` is their reference
(fixed_point_models.reference, full), computed once per (case, cap).

No GPU and no library here: tests/test_stream_models_cpu.py checks the
coverage of the list, tests/test_gpu_stream.py runs the kernels on it.
"""
from __future__ import annotations

import functools
import os
import sys
from dataclasses import dataclass

import numpy as np

import fixed_point_models as fm

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from generic_tables import KINDS  # noqa: E402

# the reference has to be far more precise than fp64: 80-bit long doubles
assert np.finfo(np.longdouble).eps < 2e-19, "np.longdouble is not the 80-bit extended format here"

EPS = 2.0 ** -53
U32 = 2.0 ** -24
PRODUCT_RANGE = {"f64": 170.0, "f32": 20.0}   # kProductRangeF64 / kProductRangeF32
WIDE_MAX = 705.0                              # kWideTableMax
MAX_S = 256                                   # kMaxS
TILE = 64                                     # kTileCols
EDGE_WEIGHTS = np.array([0.0, 2.0 ** -60, 0.5, 1.0 - 1e-6, 1.0 - 1e-9, 1.0 - 2.0 ** -53, 1.0])
RANGE_POS, RANGE_NEG = slice(0, 40), slice(40, 80)   # the one-signed column bands of a range table


def renorm(dtype, s, amax):
    """score_kernel's RENORM for a staged table (launch_score): 2 a wide table
    (fp64, |T| > 170), else 1 when needs_renorm holds (|T|max (S - 1) > 600 for
    fp64, > 80 for fp32), else 0."""
    if dtype == "f64" and amax > PRODUCT_RANGE["f64"]:
        return 2
    return int(amax * (s - 1) > (600.0 if dtype == "f64" else 80.0))


def group_renorm(dtype, s, amax):
    """score_group_kernel's RENORM (launch_group_t): needs_renorm; a wide table
    is refused (None)."""
    r = renorm(dtype, s, amax)
    return None if r == 2 else r


@dataclass(frozen=True)
class Case:
    name: str
    dtype: str       # "f64" / "f32"
    kind: str        # "shared" / "own"
    s: int
    e: int
    a: float         # amplitude; 0: a range table
    caps: tuple
    generic: bool    # staged with exact_generic=True (option exact 0 either way)
    renorm: int      # the RENORM score_kernel must select
    nevals: int      # the first ``nevals`` of ``evals`` (all 12 below S = 130)
    seed: int

    @property
    def is_range(self):
        return self.a == 0.0


def _caps(s, full=True):
    c = (0, 1, 3, s - 2, s - 1, s + 5) if full else (0, 3, s - 2, s + 5)
    return tuple(dict.fromkeys(v for v in c if v >= 0))


def _case(dtype, kind, s, e, a, caps=None, generic=False, nevals=12, seed=None):
    name = f"{dtype}-{kind}-S{s}-E{e}-" + (f"a{a:g}" if a else "range") + ("-generic" if generic else "")
    amax = a if a else 15.0
    return Case(name, dtype, kind, s, e, float(a), caps if caps is not None else _caps(s), generic,
                renorm(dtype, s, amax), nevals, seed if seed is not None else 7 + s + e)


def _build_cases():
    out = []
    # fp64 thresholds at S = 9: bound 560 (RENORM 0), 640 (1), kProductRangeF64 itself (1), wide (2)
    for k, kind in enumerate(KINDS):
        out += [_case("f64", kind, 9, (65, 64)[k], 70), _case("f64", kind, 9, (63, 65)[k], 80),
                _case("f64", kind, 9, (64, 130)[k], 170),
                _case("f64", kind, 9, (130, 63)[k], 171, generic=True),
                _case("f64", kind, 9, (63, 64)[k], 705, generic=True)]
        # fp32: bound 76 (RENORM 0), 95 (1), kProductRangeF32 itself at S = 18
        out += [_case("f32", kind, 5, (65, 63)[k], 19), _case("f32", kind, 6, (64, 65)[k], 19),
                _case("f32", kind, 18, (130, 64)[k], 20)]
        # the one-signed range tables
        out += [_case("f64", kind, 64, 130, 0, caps=(0, 3, 62)), _case("f32", kind, 64, 130, 0, caps=(0, 62))]
    # shapes: list lengths 0..17 at S = 18 under the identity order; S = 2; one, two and three
    # children per wave round (S = 64, 65, 130); kMaxS; every E class; 65 tiles
    for dtype in ("f64", "f32"):
        out += [_case(dtype, "own", 18, 130, 3), _case(dtype, "shared", 18, 1, 3, generic=dtype == "f64"),
                _case(dtype, "own", 2, 1, 3), _case(dtype, "shared", 2, 63, 3),
                _case(dtype, "shared", 64, 64, 3, caps=_caps(64, False)),
                _case(dtype, "own", 65, 65, 3, caps=_caps(65, False)),
                _case(dtype, "shared", 5, 4100, 3, caps=(0, 1, 3, 10))]
    out += [_case("f64", "own", 130, 130, 3, caps=_caps(130, False), nevals=6),
            _case("f32", "shared", 130, 63, 3, caps=(0, 3), nevals=6),
            _case("f64", "shared", MAX_S, 70, 2, caps=(0, 3, MAX_S + 5), nevals=5),
            _case("f32", "own", MAX_S, 70, 0.07, caps=(0, 3), nevals=5)]
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}


def case_ids():
    return [c.name for c in CASES]


@functools.lru_cache(maxsize=2)
def tables(name):
    """(U (S + 1, E), T (S, S, E)) of a case, fp64."""
    c = BY_NAME[name]
    rng = np.random.default_rng(c.seed)
    s, e = c.s, c.e
    if c.is_range:
        shape = (s, e) if c.kind == "shared" else (s, s, e)
        r = rng.uniform(-15.0, 15.0, shape)
        r[..., RANGE_POS] = rng.uniform(10.0, 15.0, shape[:-1] + (40,))
        r[..., RANGE_NEG] = rng.uniform(-15.0, -10.0, shape[:-1] + (40,))
        t = np.empty((s, s, e))
        t[:] = r[None] if c.kind == "shared" else r
        u = rng.uniform(-15.0, 15.0, (s + 1, e))
        # the deep child of the identity order: U cancels its row's sum in the negative band
        deep = t[s - 1, :s - 1, RANGE_NEG].sum(axis=0)
        u[s - 1, RANGE_NEG] = -deep + rng.uniform(-5.0, 5.0, deep.shape)
        return u, t
    if c.kind == "shared":
        r = rng.uniform(-c.a, c.a, (s, e))
        r[rng.integers(s), rng.integers(e)] = c.a
        t = np.empty((s, s, e))
        t[:] = r[None]
        return np.vstack([r, np.zeros((1, e))]), t
    t = rng.uniform(-c.a, c.a, (s, s, e))
    t[1, 0, rng.integers(e)] = c.a     # an off-diagonal entry: the staging's range reads those
    return rng.uniform(-c.a, c.a, (s + 1, e)), t


def table_absmax(t):
    """The staging's range: max |T| over the off-diagonal rows."""
    s = t.shape[0]
    off = ~np.eye(s, dtype=bool)
    return float(np.abs(t[off]).max())


@functools.lru_cache(maxsize=None)
def evals(s, nevals=12):
    """(perms, pos (n, S) int32, w01 (n, S, S)): fixed_point_models.inputs' nine
    evaluations, then the identity, its reverse and a random order with edge-mix
    weights.  ``nevals`` < 12 keeps the identity and the reverse at weights 1,
    the three edge mixes, then the saturated and the soft random order."""
    perms, pos, w01 = fm.inputs(s)
    rng = np.random.default_rng(977 + s)
    extra = [np.arange(s), np.arange(s)[::-1].copy(), rng.permutation(s)]
    epos = np.empty((3, s), dtype=np.int32)
    for k, p in enumerate(extra):
        epos[k, p] = np.arange(s)
    edge = EDGE_WEIGHTS[rng.integers(EDGE_WEIGHTS.size, size=(3, s, s))]
    perms, pos, w01 = list(perms) + extra, np.vstack([pos, epos]), np.concatenate([w01, edge])
    if nevals < 12:
        keep = [2, 3, 9, 10, 11, 1, 0][:nevals]
        perms, pos, w01 = [perms[k] for k in keep], pos[keep], w01[keep]
    return perms, np.ascontiguousarray(pos), np.ascontiguousarray(w01)


def list_lengths(perm, cap=0):
    """Parents per child (by node) of an order under a cap."""
    s = len(perm)
    pos = np.empty(s, dtype=np.int64)
    pos[np.asarray(perm)] = np.arange(s)
    return np.minimum(pos, cap) if 0 < cap < s - 1 else pos


@dataclass
class Ref:
    ll: np.ndarray      # (n,)
    cs: np.ndarray      # (n, E) long double
    cells: np.ndarray   # (n, S + 1, E) long double
    ow: np.ndarray      # (n, S + 1, E) long double
    nmax: np.ndarray    # (n,) the longest parent list of the evaluation


@functools.lru_cache(maxsize=2)
def _exp_table(name):
    return np.exp(tables(name)[1].astype(np.longdouble))


def _ref(u, t, et, perms, w01, cap):
    r = [fm.reference(u, t, p, w, cap, full=True, et=et) for p, w in zip(perms, w01)]
    return Ref(np.array([x[0] for x in r]), np.stack([x[1] for x in r]), np.stack([x[2] for x in r]),
               np.stack([x[3] for x in r]), np.array([int(list_lengths(p, cap).max()) for p in perms]))


@functools.lru_cache(maxsize=None)
def refs(name, cap):
    """The reference of every evaluation of a case under ``cap``, computed once."""
    c = BY_NAME[name]
    u, t = tables(name)
    perms, _, w01 = evals(c.s, c.nevals)
    return _ref(u, t, _exp_table(name), perms, w01, cap)


@functools.lru_cache(maxsize=None)
def ladder_refs(name, cap):
    """The reference of fixed_point_models.inputs on one of its models."""
    m = fm.get_model(name)
    perms, _, w01 = fm.inputs(m.S)
    return _ref(m.U, m.T, None, perms, w01, cap)


def ladder_ids():
    """The NEM rungs at S = 16 and 33 (c from -1 to 7) and the table-built models, E = 40."""
    return [n for n in fm.model_ids() if n.endswith("-E40") and (n.startswith("table") or "-S16-" in n or "-S33-" in n)]


# --------------------------------------------------------------------------
# tolerances (derived in tests/test_gpu_stream.py's docstring)
# --------------------------------------------------------------------------
def tol_cell(n, big, dtype="f64", umax=0.0, group=False):
    """|cell - ref| and |cs - ref| allowed for a list of n parents in an
    evaluation whose largest |cell| is ``big``."""
    tol = 32.0 * EPS * max(big, 1.0) + 4.0 * n * EPS
    if dtype == "f32":
        tol += 2.0 * (n * U32 + umax * U32) if group else 8.0 * n * U32 + 2.0 * umax * U32
    return tol


def tol_ll(cs, tcs):
    """E times the cs tolerance plus the summation noise every kernel shares."""
    cs = np.asarray(cs, dtype=np.float64)
    return cs.size * tcs + fm.noise(cs)


def tile_batch(n, batch):
    """Indices that fill a batch from n evaluations, cyclically."""
    return np.arange(batch) % n
