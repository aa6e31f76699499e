"""The reference, the tolerances and the restatement of tests/rates_ref.py, and
nemo.rates' absolute likelihood and chain rules, on the CPU (no GPU, no library).

* the long-double dA, dB against central differences of the long-double ll;
* the fp64 restatement of the kernel's assembly (rates_numpy) within a quarter
  of every tolerance, over S in {2, 7, 16, 33} x E in {1, 17, 65, 130}, scalar
  rates from (0.47, 0.47) down to (1e-12, 1e-12), per-gene log-uniform rates,
  and fixed_point_models.inputs' soft / saturated / all-0 / all-1 / coin
  weights, and on every input tests/test_gpu_score_rates.py runs at S <= 17;
* absolute_ll against the directly computed mixture likelihood at 0/1 weights;
* the chain rule to (alpha, beta) and to the sigmoid parameters;
* scipy's L-BFGS-B on the restatement for the fit case (the figures
  tests/test_gpu_rates_autograd.py compares the GPU fit with)."""
import numpy as np
import pytest

import fixed_point_models as fm
import rates_ref as rr

LD = np.longdouble
SHAPES_S = (2, 7, 16, 33)
SHAPES_E = (1, 17, 65, 130)
RUNGS = (0, 3, 6, 9, 12)     # (0.47, 0.47), (0.2, 0.2), (1e-3, 1e-3), (1e-5, 1e-5), (1e-12, 1e-12)


def _ratios(got, ref):
    """Worst error / tolerance of (ll, grad, dA, dB); an entry whose tolerance is 0 must be exact."""
    ll, g, da, db = got
    out = [abs(float(LD(ll) - ref.cs.sum())) / ref.tol_ll]
    for x, want, tol in ((g, ref.g, ref.tol), (da, ref.da, ref.tol_a), (db, ref.db, ref.tol_b)):
        err = np.abs(x.astype(LD) - want).astype(np.float64)
        assert (err[tol == 0.0] == 0.0).all()
        if (tol > 0.0).any():
            out.append(float((err[tol > 0.0] / tol[tol > 0.0]).max()))
    return max(out)


def _seeded_d(s, e):
    d = (np.random.default_rng(50 * s + e).random((s, e)) < 0.4).astype(np.uint8)
    d[0] = 1                  # an all-ones row
    if s > 2:
        d[1] = 0              # an all-zeros row
    return d


def test_reference_derivatives_against_central_differences():
    """h = 1e-5 in long double: the truncation h^2 / 6 |ll'''| stays below 1e-10 (E + 1) here
    (each effect's term has derivatives of order 1), the rounding 2^-63 |ll| / h below 1e-12."""
    s, e = 7, 23
    d = _seeded_d(s, e)
    d[2, 0], d[3, 0] = 0, 1
    perms, _, w01 = fm.inputs(s)
    a, b = rr.per_gene_rates(s, 3)
    h = LD(1e-5)
    for k in (0, 1, 5):
        for cap in (0, 2):
            ref = rr.rates_reference(d, a, b, perms[k], w01[k], cap)
            for gene in range(s):
                for which, want in ((0, ref.da[gene]), (1, ref.db[gene])):
                    hi, lo = [np.array(a, dtype=LD), np.array(b, dtype=LD)], [np.array(a, dtype=LD), np.array(b, dtype=LD)]
                    hi[which][gene] += h
                    lo[which][gene] -= h
                    fd = (rr.ll_longdouble(d, *hi, perms[k], w01[k], cap) - rr.ll_longdouble(d, *lo, perms[k], w01[k], cap)) / (2 * h)
                    assert abs(float(fd - want)) <= 1e-10 * (e + 1), (k, cap, gene, which)


@pytest.mark.parametrize("s", SHAPES_S)
def test_restatement_within_a_quarter_of_every_tolerance(s):
    worst = 0.0
    perms, _, w01 = fm.inputs(s)
    for e in SHAPES_E:
        d = _seeded_d(s, e)
        rates = [rr.log_ratios(*fm.LADDER[k]) for k in RUNGS] + [rr.per_gene_rates(s, 11 * s + e)]
        for a, b in rates:
            for cap in (0, 2):
                for k in range(len(perms)):
                    ref = rr.rates_reference(d, a, b, perms[k], w01[k], cap)
                    r = _ratios(rr.rates_numpy(d, a, b, perms[k], w01[k], cap), ref)
                    worst = max(worst, r)
                    assert r <= 0.25, (s, e, cap, k, r)
    print(f"RATES restatement S={s} worst err/tol {worst:.4f}")


@pytest.mark.parametrize("name", [n for n in rr.small_ids() if "E1040" not in n])
def test_restatement_on_the_small_gpu_inputs(name):
    worst = 0.0
    for setting in rr.SETTINGS:
        d, perms, _, w01, a, b = rr.case_inputs(name, setting)
        for cap in (0, 3):
            refs = rr.case_refs(name, setting, cap)
            for k in range(len(perms)):
                r = _ratios(rr.rates_numpy(d, a[k], b[k], perms[k], w01[k], cap), refs[k])
                worst = max(worst, r)
                assert r <= 0.25, (name, setting, cap, k, r)
    print(f"RATES restatement {name} worst err/tol {worst:.4f}")


def test_scalar_rates_reproduce_the_model_tables():
    """tables() at a NEM's scalar rates: the staged U and T up to the rounding of the
    reference's addition chains ((S + 1) additions of |A|, |B|-sized terms)."""
    m = fm.get_model("nem04-S16-E40")
    d, (a, b) = rr.model_d("nem04-S16-E40")
    u, t, _ = rr.tables(d, a, b)
    tol = (m.S + 2) * 2.0 ** -52 * m.S * max(abs(a), abs(b))
    assert np.abs(u.astype(np.float64) - m.U).max() <= tol
    off = ~np.eye(m.S, dtype=bool)
    assert np.array_equal(t.astype(np.float64)[off], m.T[off])


def test_absolute_ll_is_the_mixture_likelihood_at_hard_weights():
    from nemo.rates import absolute_ll
    s, e = 7, 23
    d = _seeded_d(s, e)
    rng = np.random.default_rng(9)
    for trial in range(4):
        perm = rng.permutation(s)
        w = (rng.random((s, s)) < 0.5).astype(np.float64)
        if trial % 2:
            al, be = rng.uniform(0.01, 0.4, s), rng.uniform(0.01, 0.4, s)
        else:
            al, be = 0.07, 0.2
        a, b = rr.log_ratios(al, be)
        ll = rr.rates_numpy(d, a, b, perm, w)[0]
        want = rr.mixture_ll(d, al, be, perm, w) + e * np.log(s + 1.0)
        got = float(absolute_ll(ll, d, al, be))
        # ll and L are sums of E terms of size <= |L| each, formed in fp64
        assert abs(got - want) <= (e + s + 8) * 2.0 ** -52 * (abs(want) + abs(ll)), trial
        assert got == pytest.approx(ll + rr.baseline(d, al, be), rel=1e-15)


def test_absolute_ll_in_torch_matches_numpy_and_differentiates():
    import torch

    from nemo.rates import absolute_ll
    d = _seeded_d(5, 17)
    al = np.array([0.1, 0.2, 0.05, 0.3, 0.01])
    be = np.array([0.2, 0.02, 0.15, 0.4, 0.3])
    want = float(absolute_ll(-12.5, d, al, be))
    ta, tb = torch.tensor(al, requires_grad=True), torch.tensor(be, requires_grad=True)
    got = absolute_ll(torch.tensor(-12.5, dtype=torch.float64), d, ta, tb)
    assert float(got.detach()) == pytest.approx(want, rel=1e-15)
    got.backward()
    n = d.sum(axis=1).astype(np.float64)
    assert np.allclose(ta.grad.numpy(), -(17 - n) / (1 - al), rtol=1e-14)
    assert np.allclose(tb.grad.numpy(), -n / (1 - be), rtol=1e-14)
    assert float(absolute_ll(-12.5, d, 0.1, 0.2)) == pytest.approx(-12.5 + rr.baseline(d, 0.1, 0.2), rel=1e-15)


def test_chain_rule_to_rates_and_to_sigmoid_parameters():
    """dL/d(alpha, beta) of big_l_numpy, and through rate = lo + (hi - lo) sigmoid(u), against
    central differences of L (h = 1e-6: truncation ~1e-12 |L'''|, rounding ~2^-52 |L| / h ~ 1e-7)."""
    from scipy.special import expit
    d, order, w = rr.fit_case()
    lo, hi = 1e-12, 0.5
    for al, be in ((0.2, 0.2), (0.05, 0.1), (0.3, 0.01)):
        big_l, gal, gbe = rr.big_l_numpy(d, order, w, al, be)
        h = 1e-6
        fa = (rr.big_l_numpy(d, order, w, al + h, be)[0] - rr.big_l_numpy(d, order, w, al - h, be)[0]) / (2 * h)
        fb = (rr.big_l_numpy(d, order, w, al, be + h)[0] - rr.big_l_numpy(d, order, w, al, be - h)[0]) / (2 * h)
        tol = 1e-6 * (1.0 + abs(big_l))
        assert abs(fa - gal) <= tol and abs(fb - gbe) <= tol, (al, be, fa, gal, fb, gbe)
        u = np.log(((al - lo) / (hi - lo)) / (1 - (al - lo) / (hi - lo)))
        sig = expit(u)
        hu = 1e-5
        fu = (rr.big_l_numpy(d, order, w, lo + (hi - lo) * expit(u + hu), be)[0]
              - rr.big_l_numpy(d, order, w, lo + (hi - lo) * expit(u - hu), be)[0]) / (2 * hu)
        assert abs(fu - gal * (hi - lo) * sig * (1 - sig)) <= tol


def test_scipy_fit_of_the_restatement():
    l_fit, al, be, nit, l_start, l_truth = rr.cpu_fit()
    print(f"RATES cpu fit: L_start {l_start:.2f} L_truth {l_truth:.2f} L_fit {l_fit:.2f} alpha {al:.3f} beta {be:.3f} "
          f"in {nit} iterations")
    assert l_fit >= l_truth >= l_start
    assert 1e-12 < al < 0.5 and 1e-12 < be < 0.5
