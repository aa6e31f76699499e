"""Edge shapes and inputs for the exact (reference-arithmetic) path.

The exact kernels (csrc/nemo_exact.hip) take other code paths at small and
edge E and S than at the workload shapes: no whole word group, no summation
chain, one leaf with a remainder, the 128 / 129 leaf and 1024 / 1025 slot
boundaries of numpy's pairwise sum, a last numpy buffer of fewer than 8 terms,
fold blocks of exactly 16 / 32 / 33 rows.  This module holds those shapes and
the deterministic models, orders and weights the tests run on them.

No GPU and no library here: tests/test_exact_edges_cpu.py runs the host
restatement on these inputs, tests/test_gpu_exact_edges.py the kernels.
"""
from __future__ import annotations

import functools

import numpy as np
from scipy.linalg import inv
from scipy.special import expit

import nemo_oracle as no

MODEL_SEED = 3

# E: below one chain of 8 (sum from 0.0), around 8 / 16, below and at one wave
# (64), one leaf with and without a remainder, the 128 / 129 leaf boundary and
# its 8-term splits (130, 136, 137), whole D1 word groups (256: one group of 4
# words, 192: none, 320: one group and a word), the 1024 / 1025 slot boundary,
# 2048 / 2049 (two / three slots), 8192 (the largest plan, one numpy buffer)
# and a second buffer of 1 / 7 / 8 / 9 terms
E_LIST = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 130, 136, 137, 191, 192, 193, 255, 256, 257, 264,
          320, 1023, 1024, 1025, 1032, 2047, 2048, 2049, 8191, 8192, 8193, 8199, 8200, 8201)
# S: R = S + 1 rows in the fold's register blocks of 16 (R = 16, 17, 32, 33,
# 34, 64, 65, 66, 129), the smallest models.  nemo_ctx_create refuses S = 1
# (NEMO_ERR_ARG: a model of one S-gene has no parent pair), so the engine
# shapes start at 2
S_LIST = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128)
S_MIN_ENGINE = 2
WEIGHT_KINDS = ("u3", "u40", "p800", "m800")
ORDER_KINDS = ("identity", "reverse", "random")
NUMPY_BUFSIZE = 8192
# refmath::svml_exp's fast-path bound as written in csrc/refmath.h: at or past
# it the restatement returns 0.0 / inf where numpy's rare path is tiny / huge
SVML_EXP_BOUND = float.fromhex("0x1.61da04cbafe44p+9")


def shapes(s_list=S_LIST, smin=S_MIN_ENGINE):
    """(S, E): the E list at S in {3, 17}, the S list at E in {65, 257}."""
    out = [(s, e) for s in (3, 17) for e in E_LIST]
    out += [(s, e) for e in (65, 257) for s in s_list if s >= smin and (s, e) not in out]
    return out


def shape_id(se):
    return f"S{se[0]}-E{se[1]}"


def bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@functools.lru_cache(maxsize=4)
def model(s, e, seed=MODEL_SEED):
    """(NEM, U (S + 1, E), T (S, S, E)) of generator.synthetic_nem."""
    from nemo import generator
    m = generator.synthetic_nem(s, e, seed)
    return m, np.ascontiguousarray(m.U, dtype=np.float64), np.ascontiguousarray(m.get_score_tensor(),
                                                                              dtype=np.float64)


def order(kind, s, rng):
    if kind == "identity":
        return np.arange(s)
    if kind == "reverse":
        return np.arange(s)[::-1].copy()
    return rng.permutation(s)


def raw_weights(kind, s, rng):
    """Raw (pre-expit) W: U(-3, 3), U(-40, 40), all +800 (expit exactly 1.0),
    all -800 (expit exactly 0.0)."""
    if kind == "u3":
        return rng.uniform(-3, 3, (s, s))
    if kind == "u40":
        return rng.uniform(-40, 40, (s, s))
    return np.full((s, s), 800.0 if kind == "p800" else -800.0)


def pos_of(perm):
    pos = np.empty(len(perm), dtype=np.int32)
    pos[np.asarray(perm)] = np.arange(len(perm), dtype=np.int32)
    return pos


def evals(s, e):
    """13 evaluations: every order kind against every weight kind, then one
    more random order with U(-3, 3) -- a batch of 7, one of 5 and a single
    one.  -> (perms, pos (13, S), raw W (13, S, S), kinds)."""
    rng = np.random.default_rng(1000 * s + e)
    perms, ws, kinds = [], [], []
    for ok in ORDER_KINDS:
        for wk in WEIGHT_KINDS:
            perms.append(order(ok, s, rng))
            ws.append(raw_weights(wk, s, rng))
            kinds.append((ok, wk))
    perms.append(order("random", s, rng))
    ws.append(raw_weights("u3", s, rng))
    kinds.append(("random", "u3"))
    return perms, np.stack([pos_of(p) for p in perms]), np.stack(ws), kinds


def caps(s):
    """Parent caps 0 (none), 1, 3 and S - 2, the ones below S - 1 (from S - 1
    on a cap cuts nothing)."""
    return sorted({c for c in (0, 1, 3, s - 2) if 0 <= c < max(s - 1, 1)})


def oracle_eval(u, t, perm, w01, cap=0):
    """The oracle's evaluation -> (ll, cs, cells, ow)."""
    cells = no.cell_ratios(u, t, no.parents_of(perm, cap), w01)
    ow, ll, cs = no.calculate_ll(cells)
    return float(ll), cs, cells, ow


def tail_mask(cells, cs):
    """Where the reference's order-weight argument cell - cs lies below the
    SVML exp's fast path (numpy: 5e-324 .. 4.6e-308; the restatement: 0.0)."""
    return (np.asarray(cells) - np.asarray(cs)) < -SVML_EXP_BOUND


def ow_mismatch(got, cells, cs, ow):
    """The documented order weights: the reference's bits wherever its argument
    cell - cs >= -SVML_EXP_BOUND, exactly 0.0 below (the reference at most
    4.7e-308 there).  -> "" or what differs."""
    got = np.asarray(got, dtype=np.float64)
    tail = tail_mask(cells, cs)
    if got.shape != ow.shape:
        return f"shape {got.shape} != {ow.shape}"
    if not np.array_equal(got[~tail].view(np.uint64), np.ascontiguousarray(ow[~tail]).view(np.uint64)):
        return f"{int((got[~tail] != ow[~tail]).sum())} order weights differ on the fast path"
    if tail.any() and not (np.array_equal(got[tail].view(np.uint64), np.zeros(int(tail.sum()), dtype=np.uint64))
                           and ow[tail].max() <= 4.7e-308):
        return "a tail order weight is not +0.0 (or the reference's is not tiny)"
    return ""


# --------------------------------------------------------------------------
# fused steps
# --------------------------------------------------------------------------
def step_inputs(s, e, chains):
    """Orders and raw weights of `chains` chains from default_rng(7 E + S);
    chain 0 is the one-chain case."""
    rng = np.random.default_rng(7 * e + s)
    perms, ws = [], []
    for _ in range(chains):
        perms.append(rng.permutation(s))
        ws.append(rng.uniform(-3, 3, (s, s)))
    return perms, np.stack(ws)


def host_prep(pos, w, cap=0):
    """W~ = expit(W) and ancestor_x as the sampler's host path makes them
    (nem_order_mcmc.py:98-103, :185: expit on the permissible entries)."""
    gap = pos[:, None] - pos[None, :]
    mask = (gap > 0) & ((gap <= cap) if cap else True)
    mapped = w.copy()
    mapped[mask] = expit(w[mask])
    eye = np.identity(len(pos))
    return expit(w), np.clip(inv(eye - mapped) - eye, 0, 1)


def oracle_step(u, t, perm, w_raw, cap=0):
    """One OracleSampler.optimal_weights (numpy / scipy) -> dict: ll1, the new
    weights, dag ll, the order weights and the local optima's records
    (i, k, c, anc, x0, x*, nit, nfev).  Raises where the reference raises."""
    ora = no.OracleSampler(u, t, perm, record_local=True, cap=cap)
    ora.w = np.array(w_raw, dtype=np.float64, copy=True)
    dag = ora.optimal_weights()
    return {"ll1": ora.ll1, "w": ora.w, "dag": dag, "ow": ora.ow, "anc": ora.anc, "local": ora.local_log}


def plan_slots(e):
    """Slots of the wave plan of one numpy buffer of E terms: 8 leaf blocks of
    numpy's pairwise sum per slot (csrc/nemo_host.h build_pairwise_plan)."""
    from nemo import limits
    return (limits.pairwise_leaves(min(e, NUMPY_BUFSIZE)) + 7) // 8


def exact_covered(e):
    """True where every numpy buffer of E terms splits into at most 64 leaf
    blocks, the wave plan's capacity (nemo.limits, the "E (effects)" row): of
    E_LIST every size but 8191, whose recursion reaches 65 -- there the staging
    builds no plan, exact_ok is 0 and the fast kernels run, loudly."""
    from nemo import limits
    parts = limits.pairwise_parts(e)
    return parts is not None and all(limits.pairwise_leaves(n) <= limits.MAX_LEAVES for n in parts)


def form_expected(form, cform, e):
    """The form an exact local-optimum launch runs after its documented
    fall-backs (include/nemo.h, option exact_form_used) on a factored model
    with the persistent launch (the default): past one numpy buffer the
    throughput form over the plan's parts (6); the pair form needs two slots
    (else 2); the dual form recomputed c rows and at most two slots (else 1);
    the slot form recomputed c rows (else 2)."""
    ns = plan_slots(e)
    if e > NUMPY_BUFSIZE:
        return 6
    if form == 3:
        return 3 if ns >= 2 else 2
    if form == 5:
        return 5 if cform == 1 and ns <= 2 else 1
    if form == 7:
        return 7 if cform == 1 else 2
    return form
