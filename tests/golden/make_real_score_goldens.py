"""Capture the true-graph score fixtures from the reference implementation.

Runs ONLY where the reference is importable (see ``make_goldens.py``, whose
flat import and ``wandb`` stub are reused), never from a test, and writes data
only.  For each model of ``real_score_inputs.FIXTURES`` it runs the
reference's ``NEM.compute_real_score`` (nem.py:88-144) twice, as its
constructor does -- on the real and on the observed knockdown matrix -- with a
spy on ``calculate_ll`` and on ``minimize``, and writes
``real_score_<name>.npz`` with, per call (prefix ``real_`` / ``obs_``):

    ll (n,)            every sweep's evaluation
    w (n, S, S)        the weights after every sweep (W[i][j]: child i, parent j)
    nit, status (n, pairs)   every solve's iterations / scipy status, pairs in
                       solve order (children 0..S-1, parents in parent_order)
    g0 (n, pairs)      every solve's initial forward-difference gradient
    order_ll, real_ll, parent_order   the three outputs

and the reference's own spread: the same two calls with ``local_ll_sum``'s sum
taken in long double, in reversed order, and with ``log1p``; ``d_ll``,
``d_w``, ``d_g`` are the largest per-sweep deviations of ll, the weights and
the initial gradients from the unmodified run.  A fixture whose variants
change a sweep count or a final output, or that misses one of the three
margin conditions (``check_conditions``), is not written.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_real_score_goldens.py [name ...]
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_real_score_goldens.py --time

``--time``: the reference's wall time for ONE sweep at 64 x 2000
(``generator.config_nem("C3")``, observed matrix) into
``real_score_time_ref.json``, with the machine's name.
"""
from __future__ import annotations

import copy
import json
import os
import platform
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import real_score_inputs as ri  # noqa: E402
from make_goldens import load_reference, ref_nem_without_diagnostics, repo_generator  # noqa: E402

MAX_BYTES = 512 * 1024
LL_FLOOR = W_FLOOR = 1e-6   # the tests' tolerances: max(10 d, floor)


def sum_plain(x, c):
    return -np.sum(np.log(c * x + 1.0))


def sum_longdouble(x, c):
    return float(-np.sum(np.log(c * x + 1.0).astype(np.longdouble)))


def sum_reversed(x, c):
    return -np.sum(np.ascontiguousarray(np.log(c * x + 1.0).ravel()[::-1]))


def sum_log1p(x, c):
    return -np.sum(np.log1p(c * x))


VARIANTS = {"longdouble": sum_longdouble, "reversed": sum_reversed, "log1p": sum_log1p}


class StopAfterSweep(Exception):
    pass


def run_call(ref_nem, m, knockdown, adj, objective=None, stop_after=None):
    """One compute_real_score call of the reference with the spies on."""
    s = m.num_s
    lls, times, solves = [], [], []
    real_min, real_obj = ref_nem.minimize, ref_nem.local_ll_sum
    orig_ll = m.calculate_ll

    def spy_ll(cell_ratios):
        times.append(time.perf_counter())
        if stop_after is not None and len(times) > stop_after:
            raise StopAfterSweep
        ow, ll = orig_ll(cell_ratios)
        lls.append(float(ll))
        return ow, ll

    def spy_min(fun, **kw):
        res = real_min(fun, **kw)
        c = kw["args"][0]
        x0, x1 = 0.5, 0.5 + 1e-8
        g0 = (fun(np.array([x1]), c) - fun(np.array([x0]), c)) / (x1 - x0)
        solves.append((float(res.x[0]), int(res.nit), float(g0), int(res.status), int(res.nfev)))
        return res

    m.calculate_ll = spy_ll
    ref_nem.minimize = spy_min
    if objective is not None:
        ref_nem.local_ll_sum = objective
    try:
        try:
            order_ll, real_ll, parent_order = m.compute_real_score(knockdown, copy.deepcopy(adj))
        except StopAfterSweep:
            return {"seconds": times[-1] - times[-2], "nfev": np.array([v[4] for v in solves])}
    finally:
        del m.calculate_ll
        ref_nem.minimize, ref_nem.local_ll_sum = real_min, real_obj
    parent_order = np.asarray(parent_order)
    pos = np.empty(s, dtype=np.int64)
    pos[parent_order] = np.arange(s)
    pairs = [(i, int(j)) for i in range(s) for j in parent_order[:pos[i]]]
    n = len(lls) - 2   # the last two evaluations are the final scores
    assert n >= 1 and len(solves) == n * len(pairs)
    w = np.zeros((n, s, s))
    sv = np.array(solves).reshape(n, len(pairs), 5)
    for p, (i, j) in enumerate(pairs):
        w[:, i, j] = sv[:, p, 0]
    assert sv[:, :, 1].max() < 65535
    return {"ll": np.array(lls[:n]), "w": w, "nit": sv[:, :, 1].astype(np.uint16), "g0": sv[:, :, 2],
            "status": sv[:, :, 3].astype(np.uint8), "order_ll": float(order_ll), "real_ll": float(real_ll),
            "parent_order": parent_order.astype(np.int32)}


def check_conditions(name, call, rec, d_ll, d_w, d_g):
    """The margins that keep the GPU's decisions the reference's (see the
    tests): the loop's test, the final rounding, the nit = 0 exits."""
    ll_tol, w_tol = max(10 * d_ll, LL_FLOOR), max(10 * d_w, W_FLOOR)
    diffs = np.diff(rec["ll"])
    m1 = np.abs(diffs - 1e-4).min() if diffs.size else np.inf
    moved = rec["nit"][-1] > 0
    s = rec["w"].shape[1]
    pos = np.empty(s, dtype=np.int64)
    pos[rec["parent_order"]] = np.arange(s)
    pairs = [(i, int(j)) for i in range(s) for j in rec["parent_order"][:pos[i]]]
    last = np.array([rec["w"][-1, i, j] for i, j in pairs])
    m2 = np.abs(last[moved] - 0.5).min() if moved.any() else np.inf
    m3 = np.abs(np.abs(rec["g0"]) - 0.1).min()
    ok = m1 > 100 * ll_tol and m2 > 10 * w_tol and m3 > 100 * d_g
    print(f"  {name}/{call}: sweeps {len(rec['ll'])}  |dll - 1e-4| >= {m1:.3g} (need {100 * ll_tol:.3g})  "
          f"|w - 0.5| >= {m2:.3g} (need {10 * w_tol:.3g})  ||g0| - 0.1| >= {m3:.3g} (need {100 * d_g:.3g})  "
          f"{'ok' if ok else 'MISSED'}", flush=True)
    return ok


def capture(name, ref_nem, ref_utils, gen):
    adj, end, err, s, e = ri.network_inputs(name, ref_utils, gen)
    m = ref_nem_without_diagnostics(ref_nem, ref_utils, copy.deepcopy(adj), end, err, s, e)
    mine = ri.build_nem(name)   # what the tests rebuild
    assert np.array_equal(m.observed_knockdown_mat, mine.observed_knockdown_mat) and np.array_equal(m.U, mine.U)
    assert np.array_equal(m.real_knockdown_mat, mine.real_knockdown_mat)
    calls = {"real": m.real_knockdown_mat, "obs": m.observed_knockdown_mat}
    out = {"S": s, "E": e}
    d_ll = d_w = d_g = 0.0
    base = {}
    t0 = time.time()
    for call, k in calls.items():
        base[call] = run_call(ref_nem, m, k, adj)
        for vname, obj in VARIANTS.items():
            v = run_call(ref_nem, m, k, adj, obj)
            b = base[call]
            if len(v["ll"]) != len(b["ll"]):
                raise SystemExit(f"{name}/{call}: variant {vname} runs {len(v['ll'])} sweeps, not {len(b['ll'])}")
            if (v["order_ll"], v["real_ll"]) != (b["order_ll"], b["real_ll"]) or \
                    not np.array_equal(v["parent_order"], b["parent_order"]):
                raise SystemExit(f"{name}/{call}: variant {vname} changes a final output")
            d_ll = max(d_ll, np.abs(v["ll"] - b["ll"]).max())
            d_w = max(d_w, np.abs(v["w"] - b["w"]).max())
            d_g = max(d_g, np.abs(v["g0"] - b["g0"]).max())
    print(f"{name}: {s} x {e}  d_ll {d_ll:.3g}  d_w {d_w:.3g}  d_g {d_g:.3g}  ({time.time() - t0:.1f} s)", flush=True)
    ok = all([check_conditions(name, call, base[call], d_ll, d_w, d_g) for call in calls])
    if not ok:
        raise SystemExit(f"{name}: a margin condition is missed; choose another model")
    for call, rec in base.items():
        out.update({f"{call}_{key}": val for key, val in rec.items()})
    out.update(d_ll=d_ll, d_w=d_w, d_g=d_g)
    path = os.path.join(HERE, f"real_score_{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    if size > MAX_BYTES:
        os.remove(path)
        raise SystemExit(f"{path}: {size} bytes > {MAX_BYTES}")
    print(f"{name}: wrote {size} bytes", flush=True)


def cpu_name():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def time_one_sweep(ref_nem, ref_utils, gen):
    s, e, seed = gen.CONFIGS["C3"][:3]
    net = gen.synthetic_network(s, e, seed)
    m = ref_nem_without_diagnostics(ref_nem, ref_utils, net.adj.copy(), net.end_nodes, net.errors, s, e)
    r = run_call(ref_nem, m, m.observed_knockdown_mat, net.adj.copy(), stop_after=1)
    rec = {"S": s, "E": e, "config": "C3", "call": "observed", "seconds_one_sweep": r["seconds"],
           "solves": int(r["nfev"].size), "nfev_mean": float(r["nfev"].mean()), "cpu": cpu_name(),
           "threads": os.cpu_count(), "numpy": np.__version__}
    with open(os.path.join(HERE, "real_score_time_ref.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(rec, flush=True)


def main():
    ref_nem, _ref_mcmc, ref_utils = load_reference()
    gen = repo_generator()
    if "--time" in sys.argv[1:]:
        return time_one_sweep(ref_nem, ref_utils, gen)
    for name in sys.argv[1:] or list(ri.FIXTURES):
        capture(name, ref_nem, ref_utils, gen)


if __name__ == "__main__":
    main()
