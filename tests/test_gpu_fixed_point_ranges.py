"""The fixed-point score kernels across the model space (GPU).

Every other GPU test of score_i8_kernel, score_i8o_kernel, score_i8l_kernel,
score_i8w_kernel and the capped lookup-table kernel builds its model with the
generator's default error rates: c = 4, |Delta| = 5.14, every staging gate
open and far from its edge.  Here the same kernels run on the models of
tests/fixed_point_models.py -- a ladder of error rates with c from -1 to 7,
the log2 top digit up to 127 and cells down to 690 below the null row, and
table-built models for the gates a NEM cannot reach -- under orders and
weights at their extremes (the identity and its reverse; weights 0, 1,
saturated).  Per model:

1. the options i8o / i8l / i8w / win equal the numpy restatement of staging;
2. score_kernel for auto and for every variant equals resolve_fact's answer on
   those gates (a closed variant is not run: chunked for a soft need, refused
   with a RuntimeError for a hard one);
3. every variant the gates allow is within its own bound + noise of the
   long-double reference, uncapped and under caps 3, 6 and S - 2;
4. the variants that share a walk give one another's bits, and a
   one-evaluation call the batch's.

noise = (E + 4) 2^-53 sum_e |cs_e|: the fp64 rounding every kernel shares.
Each case prints its observed errors (pytest -s) for DESIGN.md 3.5a."""
import numpy as np
import pytest

import fixed_point_models as fm
from nemo.engine import Engine

pytestmark = pytest.mark.gpu

# (fact_kernel, i8o_nodiag)
VARIANTS = ([(k, 0) for k in fm.FP64 + fm.MAX_OFFSET + fm.OFFSET] + [(7, 1), (8, 1)] +
            [(k, 0) for k in fm.LOG2 + fm.WIDE + fm.WINDOW])
SAME_BITS = [(10, 17, 20), (11, 12, 14, 16), (7, 8), (4, 6)]
CAP_TAIL = (0, 1, 3)   # under cap S - 2: random soft, random saturated, the reverse order with all-one weights


def _engine(m):
    if m.nem is not None:
        return Engine.from_knockdown(m.nem.observed_knockdown_mat, m.nem.A, m.nem.B)
    return Engine(m.U, m.T)


@pytest.mark.parametrize("name", fm.model_ids())
def test_fixed_point_kernels_on_model(name):
    m = fm.get_model(name)
    g = fm.predict(m.U, m.T)
    bits = fm.rows_of(m.T)[3]
    eng = _engine(m)
    try:
        _check_model(m, g, bits, eng)
    finally:
        eng.close()


def _check_model(m, g, bits, eng):
    s, e = m.S, m.E
    assert eng.factored
    eng.set_option("exact", 0)   # the fixed-point kernels (the exact path: test_gpu_exact.py)
    # 1. the gates
    got = {o: eng.get_option(o) for o in ("i8o", "i8l", "i8w", "win")}
    assert got == {"i8o": g.i8o, "i8l": g.i8l, "i8w": g.i8w, "win": g.win}, (got, g)
    assert eng.get_option_f64("i8o_bound") == pytest.approx(fm.fixed_point_bound("natural", g.c, bits), rel=1e-12)
    assert eng.get_option_f64("i8l_bound") == pytest.approx(fm.fixed_point_bound("log2", g.c, bits), rel=1e-12)
    # 2. auto
    auto = {}
    caps = list(dict.fromkeys((0, 3, 6, s - 2)))
    for cap in caps:
        fk, b = eng.score_kernel(cap)
        want, wb = fm.resolve(g, bits, 0, cap)
        assert fk == want and b == pytest.approx(wb, rel=1e-12), (cap, fk, want)
        auto[cap] = fk
    if g.i8o == 0 and s <= 64:
        assert auto[0] == 4      # no offset form: the max-offset kernel
    assert eng.score_kernel(0, ll_only=False) == (1, 0.0)
    perms, pos, w01 = fm.inputs(s)
    worst, bad = {}, []
    for cap in caps:
        idx = list(range(len(perms))) if cap in (0, 3, 6) else list(CAP_TAIL)
        p, w = np.ascontiguousarray(pos[idx]), np.ascontiguousarray(w01[idx])
        refs = [fm.reference(m.U, m.T, perms[k], w01[k], cap) for k in idx]
        ref = np.array([r[0] for r in refs])
        nz = np.array([fm.noise(r[1]) for r in refs])
        lls = {}
        for fk, nodiag in VARIANTS:
            eng.set_option("fact_kernel", fk)
            eng.set_option("i8o_nodiag", nodiag)
            kk, b = eng.score_kernel(cap)
            want, wb = fm.resolve(g, bits, fk, cap)
            assert kk == want, (fk, cap, kk, want)
            if want != fk:
                # 5. a closed gate: chunked (1) for a soft need, refused (-1) for a hard one
                if want == -1:
                    with pytest.raises(RuntimeError):
                        eng.score(p[:1], w[:1], cap=cap)
                continue
            assert b == pytest.approx(wb, rel=1e-12), (fk, cap)
            ll = eng.score(p, w, cap=cap)
            err = np.abs(ll - ref)
            k = int(np.argmax(err - nz))
            fam = fm.FAMILY[fk]
            if err[k] >= worst.get(fam, (-1.0,))[0]:
                worst[fam] = (float(err[k]), b, float(nz[k]), fk, cap)
            print(f"FXR {m.name} fk={fk} nodiag={nodiag} cap={cap} err={err.max():.3e} bound={b:.3e} "
                  f"noise={nz[k]:.3e}")
            # 3. the variant's own bound (every variant is run before the case fails on one)
            if not np.all(err <= b + nz):
                bad.append((fk, nodiag, cap, float(err[k]), b, float(nz[k])))
            # 4. a one-evaluation call returns the batch's bits
            for one in (0, len(idx) - 1):
                assert eng.score(p[one:one + 1], w[one:one + 1], cap=cap)[0] == ll[one], (fk, nodiag, cap, one)
            lls[(fk, nodiag)] = ll
        eng.set_option("i8o_nodiag", 0)
        eng.set_option("fact_kernel", 0)
        for group in SAME_BITS:
            have = [lls[(k, 0)] for k in group if (k, 0) in lls]
            assert len(have) in (0, len(group)), (group, cap)
            for other in have[1:]:
                assert np.array_equal(other, have[0]), (group, cap)
        if (7, 1) in lls:
            assert np.array_equal(lls[(7, 1)], lls[(8, 1)]), cap
        # auto runs what score_kernel names (4 with 8 waves below batch 384: 6's bits, which are 4's)
        assert np.array_equal(eng.score(p, w, cap=cap), lls[(auto[cap], 0)]), (cap, auto[cap])
    for fam, (err, b, nz, fk, cap) in sorted(worst.items()):
        print(f"FXRSUM {m.name} c={g.c} i8o={g.i8o} i8l={g.i8l} i8w={g.i8w} win={g.win} top={g.top_digit:.1f} "
              f"family={fam} err={err:.3e} bound={b:.3e} noise={nz:.3e} fk={fk} cap={cap}")

    assert not bad, ("(fact_kernel, nodiag, cap, |ll - ref|, bound, noise)", bad)

def test_natural_bound_scales_with_c():
    """The 8-slice kernels' bound is 2^(c - 49) per rounding: between models of
    equal S, E and D (one knockdown matrix under each rung's A, B) i8o_bound
    less its series term scales as 2^c, and the log2 bound does not move."""
    base = fm.get_model("nem04-S16-E40").nem
    d = base.observed_knockdown_mat
    e = d.shape[1]
    unit, l2 = None, None
    seen = set()
    for al, be in fm.LADDER:
        a, b = np.log(al / (1.0 - be)), np.log(be / (1.0 - al))
        dmax = abs(a + b)
        c = int(np.frexp(dmax * (1.0 + 1e-9))[1]) + 1
        eng = Engine.from_knockdown(d, a, b)
        u = (eng.get_option_f64("i8o_bound") - 1.0e-16 * e) / 2.0 ** c
        unit = u if unit is None else unit
        l2 = eng.get_option_f64("i8l_bound") if l2 is None else l2
        assert u == pytest.approx(unit, rel=1e-9), (al, be, c)
        assert eng.get_option_f64("i8l_bound") == l2
        seen.add(c)
        eng.close()
    assert seen == {-1, 1, 2, 3, 4, 5, 6, 7}
