"""The model list of tests/fixed_point_models.py covers what the fixed-point
score kernels' staging decides (CPU only), and the two digit expansions hold
at their gates' own edges.

The GPU tests (test_gpu_fixed_point_ranges.py) run the kernels on that list;
this file keeps the list from thinning out unnoticed: every staging gate is
met open and closed, the scale exponent c takes every value from -1 to 7, the
log2 top digit reaches 120 of 127 and a cell reaches 600 below the null row."""
import math
from fractions import Fraction

import numpy as np
import pytest

import fixed_point_models as fm

LN2 = Fraction("0.693147180559945309417232121458176568075500134360255254120680009")


@pytest.fixture(scope="module")
def gates():
    out = {}
    for name in fm.model_ids():
        m = fm.get_model(name)
        g = fm.predict(m.U, m.T)
        perms, _, w01 = fm.inputs(m.S)
        # evaluations 2 and 3: the identity and its reverse under all-one weights
        xmin = min(fm.reference(m.U, m.T, perms[k], w01[k])[2] for k in (2, 3)) if name.endswith("E40") else 0.0
        out[name] = (g, xmin)
    return out


def _rung(gates, k, s, e=40):
    return gates[f"nem{k:02d}-S{s}-E{e}"][0]


def test_predictor_reproduces_the_ladder(gates):
    """|Delta| = |A + B| and c per rung, and where each gate opens and closes
    along S (DESIGN.md 3.5a-1's table, recomputed here from (U, T))."""
    want = [(0.24, -1), (0.61, 1), (1.25, 2), (2.77, 3), (5.14, 4), (8.49, 5), (13.8, 5), (17.7, 6), (21.64, 6),
            (23.03, 6), (23.03, 6), (41.4, 7), (55.3, 7)]
    for k, (d, c) in enumerate(want):
        for s in fm.NEM_S:
            g = _rung(gates, k, s)
            assert abs(g.dmax - d) <= 0.006 * max(d, 1.0) and g.c == c, (k, s, g)
    for s in fm.NEM_S:   # glim = 28.8 < 40: no offset form at c = -1, at any S
        g = _rung(gates, 0, s)
        assert (g.i8o, g.i8l, g.i8w) == (0, 0, 0) and not g.why["padg"] and g.why["gabs"] and g.why["range"]
    assert _rung(gates, 5, 128).i8w == 1
    assert _rung(gates, 6, 64).i8l == 1 and _rung(gates, 6, 128).i8o == 0
    assert _rung(gates, 7, 64).i8l == 1 and 102 <= _rung(gates, 7, 64).top_digit < 103
    g = _rung(gates, 8, 60)
    assert (g.i8o, g.i8l) == (2, 1) and 124.5 <= g.top_digit < 127 and _rung(gates, 8, 64).i8o == 0
    for k in (9, 10):
        assert (_rung(gates, k, 33).i8o, _rung(gates, k, 33).i8l) == (2, 0)
        assert not _rung(gates, k, 33).why["top digit"] and _rung(gates, k, 60).i8o == 0
    assert _rung(gates, 11, 16).i8o == 2 and _rung(gates, 11, 33).i8o == 0
    assert _rung(gates, 12, 16).i8o == 2
    # the table-built models
    t = lambda kind, s: gates[f"table-{kind}-S{s}-E40"][0]
    assert (t("const", 16).c, t("const", 16).dmax, t("const", 16).i8l) == (0, 0.0, 1)
    assert (t("mixed", 33).i8o, t("mixed", 33).i8l, t("mixed", 33).win) == (2, 1, 1)
    for s in (8, 16):
        assert t("gabs", s).c == 0 and t("gabs", s).i8o == 0
        assert [k for k, v in t("gabs", s).why.items() if not v] == ["gabs"]
    assert (t("ugap", 16).c, t("ugap", 16).i8o) == (1, 1) and not t("ugap", 16).why["du"]
    assert (t("deep", 8).win, t("deep", 8).i8o) == (0, 0)
    assert (t("edge", 8).i8l, t("past", 8).i8l, t("past", 8).i8o) == (1, 0, 2)


def test_model_list_covers_every_gate_and_scale(gates):
    gs = [g for g, _ in gates.values()]
    # "pad" (-padg / ln 2 < 1000) cannot close: padg >= -500 by construction
    for cond in ("range", "gabs", "padg", "two-valued", "du", "top digit", "T0", "win"):
        seen = {g.why[cond] for g in gs if cond in g.why}
        assert seen == {True, False}, cond
    assert all(g.why.get("pad", True) for g in gs)
    assert {g.i8o for g in gs} == {0, 1, 2}
    for opt in ("i8l", "i8w", "win"):
        assert {getattr(g, opt) for g in gs} == {0, 1}, opt
    assert {g.c for g in gs} == set(range(-1, 8))
    # per effect count too (the GPU cases are the same list)
    for e in fm.EFFECTS:
        ge = [g for n, (g, _) in gates.items() if n.endswith(f"E{e}")]
        assert {g.c for g in ge} == set(range(-1, 8)) and {g.i8o for g in ge} == {0, 1, 2}
    assert any(g.i8l and g.top_digit >= 120 for g in gs)
    # a cell 600 below the null row on a model the offset kernels take
    assert any(g.i8o and g.i8l and x <= -600.0 for g, x in gates.values())
    assert len(set(gates)) == len(fm.model_ids())


def test_resolver_order():
    """fm.resolve is nemo_fact_kernels.h's resolve_fact: auto's order and the
    soft (chunked) / hard (refused) answers."""
    bits = np.zeros((16, 40), dtype=bool)
    g = fm.Gates(4, 2, 1, 0, 1, 5.0, 30.0)
    assert fm.resolve(g, bits, 0, 0)[0] == 10 and fm.resolve(g, bits, 0, 3)[0] == 9
    assert fm.resolve(g, bits, 0, 15)[0] == 10          # a cap that cuts nothing is no cap
    assert fm.resolve(g, bits, 9, 0) == (-1, 0.0) and fm.resolve(g, bits, 18, 0) == (1, 0.0)
    assert fm.resolve(g, bits, 0, 0, ll_only=False) == (1, 0.0)
    assert fm.resolve(g, bits, 0, 0, budget=0.0)[0] == 2
    g = fm.Gates(6, 2, 0, 0, 0, 23.0, 0.0)
    assert fm.resolve(g, bits, 0, 0)[0] == 8 and fm.resolve(g, bits, 10, 0)[0] == -1
    assert fm.resolve(g, bits, 0, 6)[0] == 8
    g = fm.Gates(-1, 0, 0, 0, 1, 0.24, 0.0)
    assert fm.resolve(g, bits, 0, 0)[0] == 4 and fm.resolve(g, bits, 7, 0)[0] == -1
    wide = np.zeros((128, 40), dtype=bool)
    assert fm.resolve(fm.Gates(4, 2, 0, 1, 1, 5.0, 30.0), wide, 0, 0)[0] == 18
    assert fm.resolve(fm.Gates(6, 0, 0, 0, 1, 17.0, 0.0), wide, 0, 0)[0] == 1
    assert fm.resolve(fm.Gates(6, 0, 0, 0, 1, 17.0, 0.0), wide, 19, 0)[0] == -1
    assert fm.resolve(fm.Gates(4, 2, 0, 1, 1, 5.0, 30.0), wide, 10, 0)[0] == 1


# --- the digit expansions at their gates' edges -----------------------------
def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def l2_digits(d):
    """i8l_digits (nemo_factored_i8.hip), the top digit as the int8 store leaves it."""
    hd = float(np.rint(d * fm.L2_SCALE))
    h = int(hd)
    l = int(np.rint(fma(d, fm.L2_SCALE, -hd) * 262144.0))
    hb, lb = h + fm.BIAS, l + 32 * (1 + 64)
    hd4 = [hb >> 18, ((hb >> 12) & 63) - 32, ((hb >> 6) & 63) - 32, (hb & 63) - 32]
    ld3 = [lb >> 12, ((lb >> 6) & 63) - 32, (lb & 63) - 32]
    return h, l, hd4, ld3


def test_log2_digit_expansion_exact_to_the_gate():
    """test_numerics.py::test_log2_digit_expansion_exact up to the gate itself:
    every |d| with |d| kL2Scale < vmax (stage_i8o) has its top digit in
    [-128, 127] -- the last values below the gate on both sides included -- and
    the first value whose digit would wrap is 32 units past the gate."""
    edge = fm.L2_VMAX / fm.L2_SCALE
    below = edge
    while below * fm.L2_SCALE >= fm.L2_VMAX:
        below = math.nextafter(below, 0.0)
    rng = np.random.default_rng(5)
    ds = np.concatenate([[below, -below, math.nextafter(below, 0.0), 22.0, -22.0, 22.09, -22.09],
                         below * (1.0 - rng.uniform(0, 1e-4, 200)), -below * (1.0 - rng.uniform(0, 1e-4, 200)),
                         rng.uniform(-below, below, 200)])
    for d in ds:
        d = float(d)
        assert abs(d) * fm.L2_SCALE < fm.L2_VMAX
        h, l, hd4, ld3 = l2_digits(d)
        assert -128 <= hd4[0] <= 127 and all(-32 <= q <= 31 for q in hd4[1:]), (d, hd4)
        assert -32 <= ld3[0] <= 32 and all(-32 <= q <= 31 for q in ld3[1:]), (d, ld3)
        assert (64 * hd4[0] + hd4[1]) * 4096 + (64 * hd4[2] + hd4[3]) == h
        assert ld3[0] * 4096 + (64 * ld3[1] + ld3[2]) == l
        back = Fraction(h) / 2 ** 20 + Fraction(l) / 2 ** 38
        assert abs(back - Fraction(d) / LN2) <= Fraction(2) ** -39 + Fraction(abs(d)) * Fraction(2) ** -52
    # the gate is tight: the top digit leaves int8 32 units above it (h + bias
    # = 2^25), which a gate at 2^25 - 2^17 - 2^7 (the bias's 2^11 forgotten) lets through
    wrap = (fm.L2_VMAX + 40.0) / fm.L2_SCALE
    assert l2_digits(wrap)[2][0] == 128 and wrap * fm.L2_SCALE < 2.0 ** 25 - 2.0 ** 17 - 128.0
    assert l2_digits(-wrap)[2][0] >= -128


@pytest.mark.parametrize("c", [-1, 0, 1, 2, 5, 6, 7])
def test_natural_digit_expansion_in_range_at_the_scale_edge(c):
    """i8o_digits / stage_i8o's natural-scale expansion at |d| = 2^(c-1) (1 - 1e-9),
    the largest entry stage_factored's c and the diagonal gate admit: x = d 2^(6-c)
    in (-32, 32), four balanced base-64 digits of h = rint(x 2^18) and of
    l = rint((x 2^18 - h) 2^24), the top ones in [-32, 32]; h and l rebuild from
    the MFMA pairs and the value is within 2^(c-49) of d."""
    rng = np.random.default_rng(c + 8)
    edge = 2.0 ** (c - 1) * (1.0 - 1e-9)
    for d in np.concatenate([[edge, -edge, 0.0], rng.uniform(-edge, edge, 100), edge * (1 - rng.uniform(0, 1e-6, 50))]):
        d = float(d)
        x = math.ldexp(d, 6 - c)
        hd = float(np.rint(x * 262144.0))
        h = int(hd)
        l = int(np.rint(fma(x, 262144.0, -hd) * 16777216.0))
        assert abs(h) <= 2 ** 23 and abs(l) <= 2 ** 23
        digs = []
        for v in (h, l):
            vb = v + fm.BIAS
            q = [vb >> 18, ((vb >> 12) & 63) - 32, ((vb >> 6) & 63) - 32, (vb & 63) - 32]
            assert -32 <= q[0] <= 32 and all(-32 <= t <= 31 for t in q[1:]), (c, d, q)
            assert (64 * q[0] + q[1]) * 4096 + (64 * q[2] + q[3]) == v
            digs.append(q)
        back = (Fraction(h) / 2 ** 18 + Fraction(l) / 2 ** 42) * Fraction(2) ** (c - 6)
        assert abs(back - Fraction(d)) <= Fraction(2) ** (c - 49)


def test_weight_term_keeps_small_table_values():
    """The kernels' factor 1 - s + s e^t as fma(s, e^t, 1 - s) (delta_row,
    nemo_factored.hip): within 2^-52 relative for every weight, s = 1 and its
    neighbours included, down to e^t = e^-120.  fma(s, e^t - 1, 1) is not: the
    rounding of e^t - 1 (2^-53) is 1e-4 of e^-27.6 and all of e^-120."""
    ts = [-120.0, -55.3, -27.6, -13.8, -2.25, 0.0, 2.94, 27.6]
    ws = [0.0, 1e-300, 1e-13, 1e-3, 0.5, 0.999, 1.0 - 1e-13, float(np.nextafter(1.0, 0.0)), 1.0]
    worst_old = 0.0
    for t in ts:
        e = math.exp(t)
        for s in ws:
            true = 1 - Fraction(s) + Fraction(s) * Fraction(e)
            new = fma(s, e, 1.0 - s)
            assert abs(Fraction(new) - true) <= true * Fraction(2) ** -52, (t, s)
            worst_old = max(worst_old, float(abs(Fraction(fma(s, e - 1.0, 1.0)) - true) / true))
    assert worst_old == 1.0   # (e^-120 - 1 rounds to -1: the old factor is 0 at s = 1)
