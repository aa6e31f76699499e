"""Models that walk the fixed-point score kernels' staging gates, a numpy
restatement of those gates, and a long-double reference of the order score.

The int8 kernels (score_i8_kernel, score_i8o_kernel, score_i8l_kernel,
score_i8w_kernel) and the capped lookup-table kernel rest on range arguments
checked once at staging (stage_factored in nemo_abi.cpp, stage_i8o in
nemo_factored_i8.hip, stage_window in nemo_window.hip).  This module builds

* a ladder of NEMs over the error rates (alpha, beta): |Delta| = |A + B| runs
  from 0.24 to 55, the scale exponent c from -1 to 7, and every gate is met
  open and closed as S grows;
* table-built models ``Engine(U, T)``, ``T[i][j] = R[j]`` two-valued per row,
  for the gates a NEM cannot reach;
* ``predict``: c and the gates from (U, T) alone (no library call);
* ``resolve``: nemo_fact_kernels.h's resolve_fact on those gates;
* ``reference``: cell_ratios + column log-sum-exp in np.longdouble.

No GPU and no library here: tests/test_fixed_point_ranges.py checks the
coverage of the list on the CPU, tests/test_gpu_fixed_point_ranges.py runs
the kernels on it.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field

import numpy as np
from scipy.special import expit

LN2 = 0.69314718055994530942
L2_SCALE = 1512775.3951951857   # kL2Scale = 2^20 / ln 2
BIAS = 32 * (1 + 64 + 4096)     # the balancing bias of a 4-digit base-64 expansion
# stage_i8o's log2 digit gate: rint(v) + BIAS must stay below 2^25
L2_VMAX = 2.0 ** 25 - 2.0 ** 17 - 2.0 ** 11 - 64.0
WIN_MAX_CAP = 6
ERR_BUDGET = 1e-7

# (alpha, beta) of the NEM ladder, |Delta| ascending
LADDER = [(0.47, 0.47), (0.45, 0.40), (0.4, 0.3), (0.2, 0.2), (0.05, 0.10), (0.01, 0.02), (1e-3, 1e-3),
          (1e-4, 2e-4), (2e-5, 2e-5), (1e-5, 1e-5), (1e-7, 1e-3), (1e-9, 1e-9), (1e-12, 1e-12)]
NEM_S = (16, 33, 60, 64, 128)
EFFECTS = (40, 130)
SEED = 5

# the variants of nemo_fact_kernels.h by what they need
FP64 = (1, 2, 3)
MAX_OFFSET = (4, 5, 6)
OFFSET = (7, 8)
LOG2 = (10, 11, 12, 13, 14, 16, 17, 20)
WIDE = (18, 19)
WINDOW = (9, 15)
FAMILY = {**{k: "fp64" for k in FP64}, **{k: "max-offset" for k in MAX_OFFSET}, **{k: "offset" for k in OFFSET},
          **{k: "log2" for k in LOG2}, **{k: "log2-wide" for k in WIDE}, **{k: "window" for k in WINDOW}}


# --------------------------------------------------------------------------
# the gates
# --------------------------------------------------------------------------
@dataclass
class Gates:
    c: int          # i8_cexp
    i8o: int        # option "i8o": 0 closed, 1 reads U - U[S], 2 diagonal form
    i8l: int        # option "i8l"
    i8w: int        # option "i8w"
    win: int        # option "win"
    dmax: float     # max_j |hi_j - lo_j|
    top_digit: float   # |v| + bias in units of the log2 top digit (2^18)
    why: dict = field(default_factory=dict)   # each condition, open (True) or closed


def spad(s):
    """factored_spad: S rounded up to the MFMA row blocking."""
    for v in (16, 32, 64, 128, 256):
        if s <= v:
            return v
    return -1


def rows_of(t):
    """detect_factored: parent j's shared row, its (lo, hi) with lo the row's
    first value, and the bits "not lo"."""
    s = t.shape[0]
    r = np.stack([t[1 if j == 0 else 0, j] for j in range(s)])
    for j in range(s):
        for i in range(s):
            assert i == j or np.array_equal(t[i, j], r[j]), "row not shared"
    lo = r[:, 0].copy()
    bits = r != lo[:, None]
    hi = lo.copy()
    for j in range(s):
        if bits[j].any():
            v = np.unique(r[j][bits[j]])
            assert v.size == 1, "row not two-valued"
            hi[j] = v[0]
    return r, lo, hi, bits


def _two_valued(uo, bits):
    """U - U[S] two-valued per row by the row's bit, each value within 1e-11
    of the first one seen (stage_i8o's diagonal form, stage_window): (ok, the
    two values per row with a missing one taken from the other)."""
    s = uo.shape[0]
    vals = np.zeros((s, 2))
    have = np.zeros((s, 2), dtype=bool)
    for i in range(s):
        for b in (0, 1):
            v = uo[i][bits[i] == bool(b)]
            if v.size:
                have[i, b] = True
                vals[i, b] = v[0]
                if np.max(np.abs(v - v[0])) > 1e-11:
                    return False, vals, have
    return True, vals, have


def predict(u, t) -> Gates:
    """c and the options i8o / i8l / i8w / win of the model (U, T), by the
    conditions of stage_factored, stage_i8o and stage_window."""
    u = np.asarray(u, dtype=np.float64)
    s, e = t.shape[0], t.shape[2]
    _, lo, hi, bits = rows_of(np.asarray(t, dtype=np.float64))
    why = {}
    # stage_factored: 2^(c - 1) >= max |hi - lo| (1 + 1e-9); c = 0 for Delta = 0
    dmax = float(np.max(np.abs(hi - lo)))
    c = math.frexp(dmax * (1.0 + 1e-9))[1] + 1 if dmax > 0.0 else 0
    sp = spad(s)
    uo = u[:s] - u[s]
    finite = bool(np.isfinite(uo).all())
    umin, umax = min(0.0, float(uo.min())), max(0.0, float(uo.max()))
    # stage_i8o: every parent's log factor lies between 0 and lo_j or hi_j
    fmin = float(np.sum(np.minimum(0.0, np.minimum(lo, hi))))
    fmax = float(np.sum(np.maximum(0.0, np.maximum(lo, hi))))
    gabs = float(np.sum(np.abs(lo)))
    glim = 0.9 * (2.0 ** 30 - 2.0 ** 20) * 2.0 ** (c - 24)
    padg = -min(500.0, glim)
    why["range"] = finite and umin + fmin >= -690.0 and umax + fmax <= 690.0
    why["gabs"] = gabs <= glim
    why["padg"] = padg <= -40.0
    i8o_ok = s <= 128 and 0 < sp <= 128 and why["range"] and why["gabs"] and why["padg"]
    diag = i8l_ok = False
    top = 0.0
    two, vals, have = _two_valued(uo, bits) if finite else (False, None, None)
    if i8o_ok:
        u0 = du = None
        why["two-valued"] = two
        if two:
            u0 = np.where(have[:, 0], vals[:, 0], vals[:, 1])
            du = np.where(have[:, 0] & have[:, 1], vals[:, 1] - vals[:, 0], 0.0)
            why["du"] = bool(np.all(np.abs(du) < 2.0 ** (c - 1) * (1.0 - 1e-9)))
            diag = why["du"]
        if diag:
            d2 = max(dmax, float(np.max(np.abs(du))))
            top = (d2 * L2_SCALE + BIAS) / 2.0 ** 18
            why["top digit"] = d2 * L2_SCALE < L2_VMAX
            why["T0"] = (gabs + float(np.max(np.abs(u0)))) / LN2 + 1023.0 < 2000.0
            why["pad"] = -padg / LN2 < 1000.0
            i8l_ok = why["top digit"] and why["T0"] and why["pad"]
    i8w = int(sp == 128 and i8l_ok)
    # stage_window: two-valued U - U[S]; at most 6 parents per child
    win = False
    if two:
        vv = np.where(have, vals, vals[:, ::-1])
        wmin, wmax = min(0.0, float(vv.min())), max(0.0, float(vv.max()))
        neg = np.sort(np.minimum(0.0, np.minimum(lo, hi)))[:WIN_MAX_CAP]
        pos = np.sort(np.maximum(0.0, np.maximum(lo, hi)))[::-1][:WIN_MAX_CAP]
        win = wmin + float(neg.sum()) >= -690.0 and wmax + float(pos.sum()) <= 690.0
    why["win"] = win
    return Gates(c, 0 if not i8o_ok else 2 if diag else 1, int(i8l_ok and sp <= 64), i8w, int(win), dmax, top, why)


# --------------------------------------------------------------------------
# the resolver and the bounds (nemo_fact_kernels.h, nemo_host.h)
# --------------------------------------------------------------------------
def fixed_point_bound(kind, c, bits, cap=0):
    """fixed_point_bound: kind "log2" or "natural"; bits = the staged D1 (S, E)."""
    s, e = bits.shape
    k = min(cap + 1, s) if 0 < cap < s - 1 else s
    terms = float(np.minimum(bits.sum(axis=0), k).sum()) + e
    if kind == "log2":
        return math.ldexp(LN2, -39) * (1.0 + 2.0 ** -10) * terms + 3.0e-13 * e
    return 2.0 ** (c - 49) * (1.0 + 2.0 ** -10) * terms + 1.0e-16 * e


def bound_kind(fk):
    return {"log2": "log2", "log2-wide": "log2", "offset": "natural", "max-offset": "natural"}.get(FAMILY[fk])


def _unmet(fk, g: Gates, s, cap, ll_only=True):
    """fact_unmet: 0 the row serves the call, 1 the chunked kernel runs in its
    place (a soft need unmet), -1 refused (a hard one)."""
    cap = 0 if cap >= s - 1 else cap
    sp = spad(s)
    fam = FAMILY[fk]
    int8 = ll_only and sp <= 64 and s <= 128          # kNeedInt8 (B8 is staged for S <= 128)
    if fk == 1:
        return 0
    if fam == "fp64":
        return 0 if ll_only and sp <= 64 else 1
    if fam == "max-offset":
        return 0 if int8 else 1
    if fam == "offset":
        return 1 if not int8 else 0 if g.i8o else -1
    if fam == "log2":
        return 1 if not int8 else 0 if g.i8o and g.i8l else -1
    if fam == "log2-wide":
        return 1 if not (ll_only and sp == 128) else 0 if g.i8w else -1
    return 0 if ll_only and g.win and 1 <= cap <= WIN_MAX_CAP else -1   # window


def resolve(g: Gates, bits, option, cap, ll_only=True, budget=ERR_BUDGET):
    """resolve_fact: (fact_kernel a call runs, its bound); -1 = refused."""
    s = bits.shape[0]
    ecap = 0 if cap >= s - 1 else cap

    def bnd(fk):
        kind = bound_kind(fk)
        return fixed_point_bound(kind, g.c, bits, ecap) if kind else 0.0

    def ok(fk):
        return _unmet(fk, g, s, cap, ll_only) == 0

    def within(fk):
        return bnd(fk) <= budget

    fk = option
    if option == 0:
        if ok(9):
            fk = 9
        elif ok(18) and within(18):
            fk = 18
        elif not ok(4):
            fk = 1
        elif ok(10) and within(10):
            fk = 10
        elif ok(8) and within(8):
            fk = 8
        elif within(4):
            fk = 4
        else:
            fk = 2
    else:
        un = _unmet(fk, g, s, cap, ll_only)
        if un:
            fk = 1 if un > 0 else -1
    return fk, (bnd(fk) if fk >= 0 else 0.0)


# --------------------------------------------------------------------------
# the models
# --------------------------------------------------------------------------
@dataclass
class Model:
    name: str
    U: np.ndarray
    T: np.ndarray
    nem: object = None     # the NEM of a ladder rung (staged from its knockdown matrix)

    @property
    def S(self):
        return self.T.shape[0]

    @property
    def E(self):
        return self.T.shape[2]


def _table_model(name, s, e, v0, v1, a, b, seed):
    """T[i][j] = R[j], R[j][e] = v1_j where bit_j(e) else v0_j; U[S][e] = n_e,
    U[i][e] = n_e + (a_i where bit_i(e) else b_i)."""
    rng = np.random.default_rng(seed)
    bits = rng.random((s, e)) < 0.35
    bits[:, 0] = False   # lo_j (the row's first value) = v0_j
    bits &= (np.asarray(v1) != np.asarray(v0))[:, None]   # a constant row stages no bits
    r = np.where(bits, np.asarray(v1, dtype=np.float64)[:, None], np.asarray(v0, dtype=np.float64)[:, None])
    t = np.empty((s, s, e))
    t[:] = r[None]
    n = rng.normal(-4.0, 2.0, e)
    u = np.vstack([n[None] + np.where(bits, np.asarray(a, dtype=np.float64)[:, None],
                                      np.asarray(b, dtype=np.float64)[:, None]), n[None]])
    return Model(name, u, t)


def _table(kind, s, e):
    rng = np.random.default_rng(1000 + s)
    name = f"table-{kind}-S{s}-E{e}"
    a, b = rng.uniform(-0.2, 0.2, s), rng.uniform(-0.2, 0.2, s)
    if kind == "const":        # (a) every row constant: Delta = 0, c = 0
        v = rng.uniform(-2, 2, s)
        return _table_model(name, s, e, v, v, a, b, s)
    if kind == "mixed":        # (b) mixed sign and magnitude, some Delta = 0, either order
        lo = rng.choice([-1.0, 1.0], s) * np.exp(rng.uniform(math.log(1e-3), math.log(20.0), s))
        dl = rng.choice([-1.0, 1.0], s) * np.exp(rng.uniform(math.log(1e-3), math.log(20.0), s))
        dl[::5] = 0.0
        dl[1], lo[2] = 20.0, 20.0
        return _table_model(name, s, e, lo, lo + dl, rng.uniform(-3, 3, s), rng.uniform(-3, 3, s), s)
    if kind == "gabs":         # (c) c = 0 and sum |lo| past glim = 57.5
        return _table_model(name, s, e, np.full(s, -9.0) + rng.uniform(-0.01, 0.01, s),
                            np.full(s, -9.4) + rng.uniform(-0.01, 0.01, s), a, b, s)
    if kind == "ugap":         # (d) |Delta| = 0.5, U's own gap 3 >= 2^(c - 1): no diagonal form
        lo = rng.uniform(-1, 1, s)
        return _table_model(name, s, e, lo, lo + 0.5 * rng.choice([-1.0, 1.0], s), b + 3.0, b, s)
    if kind == "deep":         # (e) six parents at -120: no lookup tables, no offset form
        lo = rng.uniform(-1, 1, s)
        lo[:6] = -120.0
        return _table_model(name, s, e, lo, lo + 0.5, a, b, s)
    if kind == "t0":           # sum |lo| past (2000 - 1023) ln 2 = 677 with every cell inside 690
        lo = 20.8 * np.where(np.arange(s) % 2, -1.0, 1.0)
        return _table_model(name, s, e, lo, lo - 20.0 * np.sign(lo), a, b, s)
    if kind == "genu":         # U - U[S] not two-valued: the offset form that reads it per cell
        m = _table_model(name, s, e, rng.uniform(-2, 2, s), rng.uniform(-2, 2, s), a, b, s)
        m.U[:s] += rng.uniform(-0.5, 0.5, (s, e))
        return m
    # the log2 top digit's edge: rint(v) + bias = 2^25 - 1 is the last value whose top
    # digit is 127; "edge" sits 300 units below it (open), "past" 500 above (closed;
    # inside the old gate 2^25 - 2^17 - 128, where the digit wrapped to -128)
    v = 2.0 ** 25 - BIAS + (-300.0 if kind == "edge" else 500.0)
    lo = rng.uniform(-1, 1, s)
    dl = rng.choice([-1.0, 1.0], s) * rng.uniform(0.5, 12.0, s)
    lo[1], dl[1] = -11.0, v / L2_SCALE
    return _table_model(name, s, e, lo, lo + dl, a, b, s)


TABLES = [("const", 16), ("mixed", 16), ("mixed", 33), ("gabs", 8), ("gabs", 16), ("ugap", 16), ("deep", 8),
          ("t0", 33), ("genu", 16), ("edge", 8), ("past", 8)]


def model_ids():
    """nemKK-S*-E*: rung KK of LADDER; table-<kind>-S*-E*: a table-built model."""
    ids = [f"nem{k:02d}-S{s}-E{e}" for k in range(len(LADDER)) for s in NEM_S for e in EFFECTS]
    return ids + [f"table-{k}-S{s}-E{e}" for k, s in TABLES for e in EFFECTS]


@functools.lru_cache(maxsize=4)
def get_model(name) -> Model:
    parts = name.split("-")
    s, e = int(parts[-2][1:]), int(parts[-1][1:])
    if parts[0] == "table":
        return _table(parts[1], s, e)
    from nemo import generator
    m = generator.synthetic_nem(s, e, SEED, errors=LADDER[int(parts[0][3:])])
    return Model(name, m.U, m.get_score_tensor(), m)


# --------------------------------------------------------------------------
# inputs and the reference
# --------------------------------------------------------------------------
def inputs(s, seed=0):
    """About 8 evaluations: random orders, the identity and its reverse (one
    child with all S - 1 parents) against weights expit(U(-3, 3)),
    expit(U(-30, 30)), all 0, all 1 and random 0/1.  -> (perms, pos, w01)."""
    rng = np.random.default_rng(seed + 31 * s)
    ident, rev = np.arange(s), np.arange(s)[::-1].copy()
    soft, hard = expit(rng.uniform(-3, 3, (2, s, s))), expit(rng.uniform(-30, 30, (2, s, s)))
    zero, one = np.zeros((s, s)), np.ones((s, s))
    coin = (rng.random((2, s, s)) < 0.5).astype(np.float64)
    evals = [(rng.permutation(s), soft[0]), (rng.permutation(s), hard[0]), (ident, one), (rev, one),
             (ident, zero), (rng.permutation(s), coin[0]), (rev, hard[1]), (ident, coin[1]), (rev, soft[1])]
    perms = [np.asarray(p) for p, _ in evals]
    pos = np.empty((len(evals), s), dtype=np.int32)
    for k, p in enumerate(perms):
        pos[k, p] = np.arange(s)
    return perms, pos, np.stack([w for _, w in evals])


def reference(u, t, perm, w01, cap=0, full=False, et=None):
    """The oracle's operation in np.longdouble: cell[i] = U[i] + sum over the
    permissible parents j of log(1 - w + w exp(T[i][j])) (nemo_oracle.cell_ratios;
    with a cap the last ``cap`` predecessors), then the column log-sum-exp with
    a max shift and its sum.  -> (ll, cs, min over i, e of cell - U[S]);
    ``full``: (ll, cs, cells (S + 1, E), order weights exp(cell - cs)), the
    last three in long double.  ``et``: exp(T) in long double, when the caller
    keeps it across evaluations."""
    ld = np.longdouble
    s = t.shape[0]
    perm = np.asarray(perm)
    cell = np.array(u, dtype=ld)
    one = ld(1)
    for p in range(s):
        i = perm[p]
        pa = perm[max(0, p - cap) if cap else 0:p]
        if pa.size:
            w = w01[i, pa].astype(ld)[:, None]
            v = np.exp(t[i, pa].astype(ld)) if et is None else et[i, pa]
            cell[i] += np.log(one - w + w * v).sum(axis=0)
    m = cell.max(axis=0)
    cs = m + np.log(np.exp(cell - m).sum(axis=0))
    if full:
        return float(cs.sum()), cs, cell, np.exp(cell - cs)
    return float(cs.sum()), cs.astype(np.float64), float((cell[:s] - cell[s]).min())


def noise(cs):
    """The fp64 rounding every kernel shares: (E + 4) 2^-53 sum_e |cs_e| (the
    left-fold summation bound over E columns plus a few ulps per column)."""
    return (cs.size + 4) * 2.0 ** -53 * float(np.abs(cs).sum())
