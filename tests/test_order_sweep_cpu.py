"""nemo_order_sweep without a GPU: the numpy fp64 restatement (the device's form)
within half of order_sweep_ref's tolerances, the reference's orders and scores
against brute-force long-double rescoring of the order held, the decision margins of
every margined input positive at every visit, the forced inputs, the fused
gibbs_orders against the unfused one and the enumeration, sweep_relocations, the
symbols and bindings, and the two host-side checks under the host sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fixed_point_models as fm
import order_sweep_ref as osr
import reloc_ref as rr

LD = np.longdouble
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_numpy(tag, ref, got, forced=None, factor=0.5):
    """The restatement against the reference at ``factor`` of every tolerance -> worst err / tol."""
    pos_out, ll0, ll, q, dll, vis, nmoved = got
    want_q = ref.q if forced is None else forced
    assert np.array_equal(q, want_q), tag
    assert np.array_equal(np.argsort(pos_out), ref.perms[-1]) and nmoved == ref.nmoved, tag
    worst = 0.0
    for k in range(len(q)):
        p = ref.p[k]
        assert dll[k, p] == 0.0 and not np.signbit(dll[k, p]), (tag, k, "exact +0.0")
        assert np.isfinite(dll[k]).all(), (tag, k)
        ok = np.arange(dll.shape[1]) != p
        assert (ref.tols[k][ok] > 0.0).all() and ref.tols[k][p] == 0.0
        err = np.abs(dll[k].astype(LD) - ref.rows[k]).astype(np.float64)
        ratio = err[ok] / ref.tols[k][ok]
        if ok.any():
            worst = max(worst, float(ratio.max()))
            assert (ratio <= factor).all(), (tag, k, float(ratio.max()))
        assert abs(float(LD(vis[k]) - ref.ll[k + 1])) <= factor * ref.tol_ll[k + 1], (tag, k, "ll_vis")
    assert abs(float(LD(ll0) - ref.ll[0])) <= factor * ref.tol_ll[0], tag
    assert abs(float(LD(ll) - ref.ll[-1])) <= factor * ref.tol_ll[-1], tag
    return worst


# ---- the margined inputs --------------------------------------------------------------
@pytest.mark.parametrize("name", osr.MARGINED + osr.SHAPES + (rr.WIDE_MODEL,))
def test_margins_positive_at_every_visit_and_numpy_within_half(name):
    worst, least = 0.0, np.inf
    for k in osr.evals_of(name):
        m, perm, _, w, visit, us = osr.factored_sweep_case(name, k)
        ref = osr.factored_sweep_ref(name, k)
        assert ref.margin.shape == (len(visit),)
        assert (ref.margin > 0.0).all(), (name, k, int(np.argmin(ref.margin)), float(ref.margin.min()))
        least = min(least, float(ref.margin.min()))
        worst = max(worst, _check_numpy((name, k), ref, osr.sweep_numpy(m.U, m.T, perm, w, visit, us)))
        if 2 < m.S <= 64:
            assert ref.nmoved > 0 and (ref.drift[-1] > 0.0)      # the second sweep runs on a drifted state
    print(f"ORDER-SWEEP {name}: numpy worst err/tol {worst:.4f}, least Gibbs margin {least:.3g} of the CDF total")


@pytest.mark.parametrize("name", osr.GENERIC_MARGINED)
def test_margins_positive_at_every_visit_and_numpy_within_half_generic(name):
    _, u, t, perm, _, w, visit, us = osr.generic_sweep_case(name, 0, forced=False)
    ref = osr.generic_sweep_ref(name, 0, False)
    assert (ref.margin > 0.0).all(), (name, int(np.argmin(ref.margin)), float(ref.margin.min()))
    _check_numpy(name, ref, osr.sweep_numpy(u, t, perm, w, visit, us))


@pytest.mark.parametrize("name", ("small-S2-E17", "nem08-S16-E40", "table-deep-S8-E40"))
def test_reference_against_brute_force_rescoring(name):
    """The orders replayed from q with nemo.methods.apply_relocation, each rescored from scratch in long
    double: the reference's ll after every visit, and ll before + row[q] = ll after within the entry's
    tolerance plus the rounding of the two sums over E."""
    from nemo.methods import apply_relocation
    m, perms, pos, w = rr.factored_case(name)
    et = np.exp(m.T.astype(LD))
    visit = osr.label_sweeps(m.S, 2)
    for k in (0, 1, 5):
        us = osr.seeded_u(len(visit), k)
        ref = osr.sweep_reference(m.U, m.T, perms[k], w[k], visit, us, et=et)
        held = pos[k].copy()
        assert abs(float(ref.ll[0] - fm.reference(m.U, m.T, perms[k], w[k], 0, full=True, et=et)[1].sum())) == 0.0
        for v, a in enumerate(visit):
            assert ref.p[v] == held[a]
            held = apply_relocation(held, int(a), int(ref.q[v]))
            assert np.array_equal(np.argsort(held), ref.perms[v + 1])
            cs = fm.reference(m.U, m.T, np.argsort(held), w[k], 0, full=True, et=et)[1]
            slack = 8.0 * m.E * 2.0 ** -63 * float(np.abs(cs).max())
            assert abs(float(cs.sum() - ref.ll[v + 1])) <= slack, (name, k, v)
            step = abs(float((ref.ll[v] + ref.rows[v][ref.q[v]]) - ref.ll[v + 1]))
            assert step <= ref.tols[v][ref.q[v]] + slack, (name, k, v, step)
            if ref.q[v] == ref.p[v]:
                assert ref.ll[v + 1] == ref.ll[v]


# ---- the forced inputs -----------------------------------------------------------------
@pytest.mark.parametrize("name", osr.FORCED)
def test_forced_decisions_factored(name):
    """u alternating 0 and 2.0: position 0, then S - 1 -- the longest walks in both directions -- on the
    models whose tolerance is too wide for a margin."""
    for k in osr.evals_of(name, True):
        m, perm, _, w, visit, us = osr.factored_sweep_case(name, k, forced=True)
        ref = osr.factored_sweep_ref(name, k, True)
        want = osr.forced_q(len(visit), m.S)
        assert np.array_equal(ref.q, want)
        worst = _check_numpy((name, k), ref, osr.sweep_numpy(m.U, m.T, perm, w, visit, us), forced=want)
        print(f"ORDER-SWEEP {name} [{k}] forced: numpy worst err/tol {worst:.4f}")


@pytest.mark.parametrize("name", rr.GENERIC)
def test_forced_decisions_generic(name):
    for k in ((0, 1, 5) if rr.generic_case(name)[0].s <= 18 else (0,)):
        _, u, t, perm, _, w, visit, us = osr.generic_sweep_case(name, k)
        ref = osr.generic_sweep_ref(name, k)
        want = osr.forced_q(len(visit), t.shape[0])
        assert np.array_equal(ref.q, want)
        _check_numpy((name, k), ref, osr.sweep_numpy(u, t, perm, w, visit, us), forced=want)


def test_decision_rules():
    row = np.array([-1.0, 0.0, 0.5, -3.0])
    assert osr.gibbs_draw(row, 0.0, 1.0)[0] == 0 and osr.gibbs_draw(row, 1.0, 1.0)[0] == 3
    assert osr.gibbs_draw(row, 2.0, 1.0)[0] == 3
    assert osr.greedy_pick(row, 1, 0.0)[0] == 2 and osr.greedy_pick(row, 1, 0.5)[0] == 1      # strictly
    assert osr.greedy_pick(np.array([0.5, 0.0, 0.5]), 1, 0.0)[0] == 0                          # ties: the lowest


def test_rows_that_hold_a_nan_move_nothing():
    """The decision rule of a row the walk could not score: q* = p in both modes, for a NaN anywhere in
    the row and for an infinite entry (its CDF total is inf - inf); a NaN uniform still lands in range."""
    nan, inf = np.nan, np.inf
    clean = np.array([-1.0, 0.0, 0.5, -3.0])
    for p in range(4):
        for at in range(4):
            for bad in (nan, inf):
                row = clean.copy()
                row[at] = bad
                if np.isnan(bad):
                    assert osr.decide(row, p, 0.3, 1.0, 0.0) == p and osr.decide(row, p, None, inf, 0.0) == p
                else:
                    assert osr.decide(row, p, 0.3, 1.0, 0.0) == p           # Gibbs: no CDF
        assert 0 <= osr.decide(clean, p, nan, 1.0, 0.0) <= 3
    assert osr.decide(clean, 1, 0.0, 1.0, 0.0) == 0 and osr.decide(clean, 1, 2.0, 1.0, 0.0) == 3
    assert osr.decide(clean, 1, None, inf, 0.0) == 2 and osr.decide(clean, 1, None, inf, 0.5) == 1


# ---- the samplers and the search ---------------------------------------------------------
def test_rng_matrix_draw_is_the_stream_of_successive_draws():
    a, b = np.random.default_rng(7), np.random.default_rng(7)
    assert np.array_equal(a.random((5, 9)), np.stack([b.random(9) for _ in range(5)]))


def test_fused_gibbs_orders_gives_the_unfused_chains():
    from nemo.methods import gibbs_orders
    u, t, w = rr.gibbs_model()
    b = rr.GIBBS_CHAINS
    pos = osr.gibbs_start()
    wb = np.broadcast_to(w, (b, 4, 4))
    least, want_pos = osr.gibbs_margins()
    assert least > 0.0, least                       # no uniform within rounding of a CDF step
    e1, e2 = osr.NumpyEngine(u, t), osr.NumpyEngine(u, t)
    p1, l1, b1 = gibbs_orders(e1, pos, wb, rr.GIBBS_SWEEPS, burn_in=rr.GIBBS_BURN, rng=rr.GIBBS_SEED)
    p2, l2, b2 = gibbs_orders(e2, pos, wb, rr.GIBBS_SWEEPS, burn_in=rr.GIBBS_BURN, rng=rr.GIBBS_SEED, fused=True)
    assert e2.sweeps == rr.GIBBS_SWEEPS and not e2.calls          # one order_sweep call per sweep, nothing else
    assert len(e1.calls) == rr.GIBBS_SWEEPS * 4
    assert np.array_equal(p1, p2) and np.array_equal(p2, want_pos)
    assert l1.shape == l2.shape and np.abs(l1 - l2).max() <= 1e-9
    assert np.abs(b1 - b2).max() <= 1e-9
    z = rr.gibbs_z(b2, rr.gibbs_enumeration())
    print(f"ORDER-SWEEP gibbs_orders fused (numpy engine): least margin {least:.3g}, worst z-score {z:.2f}")
    assert z <= 3.0, z


def test_sweep_relocations_on_the_numpy_engine():
    from nemo.methods import sweep_relocations
    m, pos, w = rr.greedy_inputs()
    refs = osr.greedy_sweep_refs()
    assert min(float(r.margin.min()) for r in refs) > 0.0          # the first sweep's decisions are clear
    eng = osr.NumpyEngine(m.U, m.T)
    trace = []
    out, ll, n, sweeps = sweep_relocations(eng, pos, w, ll_trace=trace)
    assert eng.sweeps == sweeps and len(trace) == sweeps + 1 and sweeps >= 2
    assert (n >= [r.nmoved for r in refs]).all() and np.array_equal(trace[-1], trace[-2])
    assert (np.diff(np.stack(trace), axis=0) >= -1e-9).all()
    for k in range(len(pos)):
        assert sorted(out[k]) == list(range(m.S))
        l0, dll = rr.reloc_numpy(m.U, m.T, np.argsort(out[k]), w[k])
        assert abs(l0 - ll[k]) <= 1e-9 and dll.max() <= 1e-9 + 1e-9          # no single relocation still gains
    # the input is not touched, and max_sweeps cuts the search short
    out1, _, n1, s1 = sweep_relocations(osr.NumpyEngine(m.U, m.T), pos, w, max_sweeps=1)
    assert s1 == 1 and list(n1) == [r.nmoved for r in refs]
    assert all(np.array_equal(np.argsort(out1[k]), refs[k].perms[-1]) for k in range(len(pos)))
    out0, ll0, n0, s0 = sweep_relocations(osr.NumpyEngine(m.U, m.T), pos, w, max_sweeps=0)
    assert s0 == 0 and not n0.any() and np.array_equal(out0, pos) and np.allclose(ll0, trace[0], atol=1e-9)


# ---- the symbols and the bindings -----------------------------------------------------------
NAMES = ("nemo_order_sweep", "nemo_order_sweep_dev")


@pytest.fixture(scope="module")
def lib():
    from nemo import _lib, build
    build.build()
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    from nemo import _lib
    bound = {name: args for name, _, args in _lib.SIGNATURES}
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in bound
    assert len(bound["nemo_order_sweep"]) == 17 and len(bound["nemo_order_sweep_dev"]) == 18


def test_engine_and_package_expose_the_feature():
    import inspect
    import nemo
    from nemo import methods
    from nemo.engine import Engine
    assert callable(Engine.order_sweep) and callable(Engine.order_sweep_dev)
    assert nemo.sweep_relocations is methods.sweep_relocations
    assert "sweep_relocations" in methods.__all__ and "sweep_relocations" in nemo.__all__
    assert inspect.signature(methods.gibbs_orders).parameters["fused"].default is False


def test_null_context_is_refused(lib):
    from nemo import _lib
    buf = np.zeros(8)
    a = _lib.addr(buf)
    assert lib.nemo_order_sweep(None, 1, a, a, 1, a, a, 1.0, 0.0, 0, a, a, a, a, a, a, a) == _lib.NEMO_ERR_ARG
    assert b"null context" in lib.nemo_last_error()
    assert lib.nemo_order_sweep_dev(None, 1, a, a, 1, a, a, 1.0, 0.0, 0, a, a, a, a, a, a, a, None) == _lib.NEMO_ERR_ARG
    assert b"null context" in lib.nemo_last_error()
    assert not buf.any()


# ---- the host entry's two new argument checks, stand-alone under the sanitizers ---------------
def test_visit_and_uniform_checks_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler: the host checks cannot be built"
    exe = str(tmp_path / "order_sweep_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(REPO, "nem-mcmc-optimization_amd", "csrc"), "-I", os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "host", "order_sweep_check.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "order_sweep_check: ok" in out.stdout
