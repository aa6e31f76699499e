"""The order-score gradient's reference and tolerance (tests/score_grad_ref.py),
checked on the CPU: the closed form against central differences of the
long-double ll, a plain numpy fp64 restatement inside a quarter of the tolerance
on every input tests/test_gpu_score_grad.py runs (so the inputs and the
tolerance are sound and no case needs excluding), and the reference's zeros
and parent counts."""
import numpy as np
import pytest

import fixed_point_models as fm
import score_grad_ref as gr
import stream_models as sm

LD = np.longdouble


def _central(u, t, perm, w, cap, et):
    """Central differences (h = 1e-6) of the long-double ll at the permissible pairs."""
    h = 1e-6
    ok = gr.permissible(perm, cap)
    g = np.zeros(w.shape, dtype=LD)
    for i, j in zip(*np.nonzero(ok)):
        wp, wm = w.copy(), w.copy()
        wp[i, j] += h
        wm[i, j] -= h
        cp = fm.reference(u, t, perm, wp, cap, full=True, et=et)[1]
        cm = fm.reference(u, t, perm, wm, cap, full=True, et=et)[1]
        g[i, j] = (cp.sum() - cm.sum()) / (LD(wp[i, j]) - LD(wm[i, j]))
    return g


@pytest.mark.parametrize("cap", [0, 2])
@pytest.mark.parametrize("kind", ["factored", "generic"])
def test_closed_form_equals_central_differences(kind, cap):
    if kind == "factored":
        m = gr.get_model("small-S6-E37")
        u, t = m.U, m.T
    else:
        rng = np.random.default_rng(11)
        t = rng.uniform(-3.0, 3.0, (6, 6, 37))
        u = rng.uniform(-3.0, 3.0, (7, 37))
    et = np.exp(t.astype(LD))
    perms, _, w01 = fm.inputs(6)
    for k in (0, 8):   # the two soft-weight evaluations: w +- h stays inside (0, 1)
        ref = gr.grad_reference(u, t, perms[k], w01[k], cap, et=et)
        fd = _central(u, t, perms[k], w01[k], cap, et)
        err = np.abs(fd - ref.g).astype(np.float64)
        assert (err <= 1e-8 * np.maximum(1.0, np.abs(ref.g).astype(np.float64))).all(), (k, float(err.max()))


def _check_numpy(tag, u, t, perms, w01, refs, cap, assemblies):
    worst = 0.0
    for k, (perm, w) in enumerate(zip(perms, w01)):
        ref = refs[k]
        ok = gr.permissible(perm, cap)
        for asm in assemblies:
            ll, g = gr.grad_numpy(u, t, perm, w, cap, assembly=asm)
            assert np.isfinite(g).all() and np.isfinite(ref.tol).all(), (tag, cap, k, asm)
            assert (g[~ok] == 0.0).all()
            err = np.abs(g.astype(LD) - ref.g).astype(np.float64)
            bad = err[ok] > 0.25 * ref.tol[ok]
            assert not bad.any(), (tag, cap, k, asm, float((err[ok] / ref.tol[ok]).max()))
            if ok.any():
                worst = max(worst, float((err[ok] / ref.tol[ok]).max()))
            assert abs(ll - ref.ll) <= ref.tol_ll, (tag, cap, k, asm)
    return worst


@pytest.mark.parametrize("name", gr.factored_ids() + [gr.WIDE_MODEL])
def test_numpy_restatement_within_a_quarter_of_the_tolerance_factored(name):
    m, perms, _, w01 = gr.factored_inputs(name)
    worst = 0.0
    for cap in gr.factored_caps(m.S):
        worst = max(worst, _check_numpy(name, m.U, m.T, perms, w01, gr.factored_refs(name, cap), cap,
                                        ("direct", "factored")))
    print(f"GRADREF {name} numpy fp64 worst err/tol = {worst:.3f}")


@pytest.mark.parametrize("name", gr.GENERIC)
def test_numpy_restatement_within_a_quarter_of_the_tolerance_generic(name):
    c, u, t, perms, _, w01 = gr.generic_inputs(name)
    worst = 0.0
    for cap in gr.generic_caps(c.s):
        worst = max(worst, _check_numpy(name, u, t, perms, w01, gr.generic_refs(name, cap), cap, ("direct",)))
    print(f"GRADREF {name} numpy fp64 worst err/tol = {worst:.3f}")


@pytest.mark.parametrize("name", ["nem04-S33-E40", "small-S17-E65", "f64-own-S18-E130-a3"])
def test_reference_zero_off_the_permissible_set_and_parent_counts(name):
    if name in gr.GENERIC:
        c, _, _, perms, _, _ = gr.generic_inputs(name)
        s, caps, refs = c.s, gr.generic_caps(c.s), gr.generic_refs
    else:
        m, perms, _, _ = gr.factored_inputs(name)
        s, caps, refs = m.S, gr.factored_caps(m.S), gr.factored_refs
    for cap in caps:
        for perm, ref in zip(perms, refs(name, cap)):
            ok = gr.permissible(perm, cap)
            assert (ref.g[~ok] == 0).all() and (ref.tol[~ok] == 0).all()
            assert (ref.tol[ok] > 0).all()
            assert np.array_equal(ref.n, sm.list_lengths(perm, cap))
            assert np.array_equal(ref.n, ok.sum(axis=1))
    assert s == len(perms[0])
