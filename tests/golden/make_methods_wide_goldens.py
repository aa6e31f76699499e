"""Capture the wide fixed-order optimizer fixtures from the reference.

Runs ONLY in the build container, where the reference is importable (see
``make_goldens.py``, whose flat import and ``wandb`` stub are reused), and
never from a test.  For each model of ``methods_wide_inputs.FIXTURES`` (S > 64:
the shapes that reach column_solve<2> / <4> of nemo_methods.hip) it runs one
``Method.opt_γ`` sweep (methods.py:397-405) and one ``InverseMethod.opt_b``
sweep (:117-129) of the reference from starting weights that make pairs move,
with a spy on the reference's ``minimize`` for every pair's (nit, nfev), and
writes ``methods_wide_<S>x<E>.npz``.  The fixtures are data: seeds, the order
and the reference's outputs.  The model is rebuilt from
``generator.synthetic_nem(S, E, model_seed)`` and the starts from their seeds
(``methods_wide_inputs``); the new weights are stored on the permissible pairs
only, in loop order (``pair_list``).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_methods_wide_goldens.py [name ...]

A fixture that misses a coverage condition (``check_coverage``) or holds a
failed minimisation is not written.
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import methods_wide_inputs as mw  # noqa: E402
from make_goldens import load_reference, ref_nem_without_diagnostics, repo_generator  # noqa: E402

MAX_BYTES = 128 * 1024  # the largest fixture committed before these


def capture(name, ref_nem, ref_utils, ref_methods, gen):
    f = mw.FIXTURES[name]
    s, e = f["S"], f["E"]
    net = gen.synthetic_network(s, e, f["model_seed"])
    m = ref_nem_without_diagnostics(ref_nem, ref_utils, net.adj.copy(), net.end_nodes, net.errors, s, e)
    mine = gen.synthetic_nem(s, e, f["model_seed"])  # what the tests rebuild
    assert np.array_equal(m.observed_knockdown_mat, mine.observed_knockdown_mat) and np.array_equal(m.U, mine.U)
    tables = m.get_score_tables(m.observed_knockdown_mat)
    order = mw.draw_order(s, f["order_seed"])
    ii, kk = mw.pair_list(order)
    g0, b0 = mw.fixture_starts(name, order)
    out = dict(S=s, E=e, order=order.astype(np.int32), model_seed=f["model_seed"], gamma_seed=f["gamma_seed"],
               inverse_seed=f["inverse_seed"], density=f["density"],
               # the starts are rebuilt from the seeds: their sums catch a generator whose stream changed
               gamma_start_sum=g0.sum(), inverse_start_sum=b0.sum())
    real = ref_methods.minimize
    new = {}
    for kind, cls, sweep, w0, bounds in (("gamma", ref_methods.Method, "opt_γ", g0, [(0, 1)]),
                                         ("inverse", ref_methods.InverseMethod, "opt_b", b0, [(-5000, 500)])):
        meth = cls(order, s, e, m.U, tables)
        spy = mw.MinimizeSpy(real)
        ref_methods.minimize = spy
        t0 = time.time()
        try:
            ll, w = getattr(meth, sweep)(w0.copy(), bounds)  # raises when a minimisation fails
        finally:
            ref_methods.minimize = real
        w = np.asarray(w, dtype=np.float64)
        assert all(spy.ok) and len(spy.nit) == len(ii)
        off = np.ones((s, s), dtype=bool)
        off[ii, kk] = False
        assert np.array_equal(w[off], w0[off])  # only the permissible pairs change
        assert max(spy.nit) < 256 and max(spy.nfev) < 256
        out.update({f"{kind}_ll": float(ll), f"{kind}_w": w[ii, kk],
                    f"{kind}_nit": np.array(spy.nit, dtype=np.uint8),
                    f"{kind}_nfev": np.array(spy.nfev, dtype=np.uint8)})
        new[kind] = w
        print(name, kind, "ll", ll, f"{time.time() - t0:.1f} s", flush=True)
    counts = mw.check_coverage(name, order, g0, new["gamma"], b0, new["inverse"])
    path = os.path.join(HERE, f"methods_wide_{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    if size > MAX_BYTES:
        os.remove(path)
        raise SystemExit(f"{path}: {size} bytes > {MAX_BYTES}")
    print(name, counts, size, "bytes", flush=True)


def main():
    ref_nem, _ref_mcmc, ref_utils = load_reference()
    import methods as ref_methods
    gen = repo_generator()
    for name in sys.argv[1:] or list(mw.FIXTURES):
        capture(name, ref_nem, ref_utils, ref_methods, gen)


if __name__ == "__main__":
    main()
