"""The fused step on real-valued (generic) tables, option exact_generic, next to
the fast generic step and the factored exact step of the same build.

    python tools/generic_step_probe.py --mode generic_exact|generic_fast|factored_exact
                                       [--chains 16] [--steps 20] [--warmup 3] [--s 64] [--e 2000]
                                       [--form F] [--cform 0|1]
    python tools/generic_step_probe.py --summarize KERNEL_STATS.csv --steps N

generic_*: ``TableModel.from_log_ratios(R)``, R ~ N(0, 1) (seed 0), with option
exact 1 / 0; factored_exact: the synthetic NEM of the same shape.  Every mode
runs warmup + steps synchronous ``nemo_optimal_weights`` calls of ``chains``
chains (random orders, W ~ U(-3, 3)) and prints the wall milliseconds per
step.  Under ``rocprofv3 --kernel-trace --stats`` the run's kernel_stats.csv
holds the kernels of all warmup + steps calls; ``--summarize`` prints the
kernel milliseconds per step and each kernel's share from it.

``--form`` / ``--cform`` set the exact local optima's ``exact_form`` and
``exact_cform`` (a row-shared generic table follows them like a factored one:
``--cform 0`` stored rows, ``1`` per-parent recompute rows; ``--form 2``
throughput, ``7`` slot, ...).  The result line also names the form that ran
(``exact_form_used``), ``exact_rc`` / ``exact_shared``, and the device memory
taken between staging and the end of the first step (``step_mem_mb``: the
buffers ``exact_reserve`` and ``nemo_reserve`` allocate), from
``torch.cuda.mem_get_info`` when torch is importable.
"""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nem-mcmc-optimization_amd"))


def summarize(path, steps):
    rows = []
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            rows.append((r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])))
    total = sum(r[2] for r in rows)
    out = {"kernel_ms_per_step": total / steps / 1e6, "steps": steps, "kernels": []}
    for name, calls, ns in sorted(rows, key=lambda r: -r[2]):
        # "void nemo::(anonymous namespace)::kernel<args>(params)" -> "kernel<args>"
        short = name.replace("(anonymous namespace)::", "").split("(")[0].split("::")[-1]
        out["kernels"].append({"name": short, "calls": calls, "ms_per_step": ns / steps / 1e6,
                               "share": ns / total})
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["generic_exact", "generic_fast", "factored_exact"])
    ap.add_argument("--chains", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--s", type=int, default=64)
    ap.add_argument("--e", type=int, default=2000)
    ap.add_argument("--form", type=int, default=None)
    ap.add_argument("--cform", type=int, default=None)
    ap.add_argument("--summarize")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.steps)
    if not a.mode:
        ap.error("--mode or --summarize")
    import numpy as np
    from scipy.special import expit

    from nemo import generator
    from nemo.engine import Engine
    from nemo.nem import TableModel
    from nemo.nem_order_mcmc import SIG0, SIG1
    s, e, n = a.s, a.e, a.chains
    if a.mode == "factored_exact":
        eng = Engine.for_nem(generator.synthetic_nem(s, e, 0))
    else:
        eng = Engine.for_model(TableModel.from_log_ratios(np.random.default_rng(0).normal(0, 1, (s, e))))
        eng.set_option("exact", 1 if a.mode == "generic_exact" else 0)
    exact = bool(eng.get_option("exact")) and bool(eng.get_option("exact_ok"))
    if exact != (a.mode != "generic_fast"):
        raise SystemExit(f"{a.mode}: exact={eng.get_option('exact')} exact_ok={eng.get_option('exact_ok')}")
    if a.form is not None:
        eng.set_option("exact_form", a.form)
    if a.cform is not None:
        eng.set_option("exact_cform", a.cform)

    def used_mb():
        try:
            import torch
            free, total = torch.cuda.mem_get_info(eng.device)
            return (total - free) / 2**20
        except Exception:
            return None

    def opt(name):   # (None on a build without the option: the probe also times older builds)
        try:
            return eng.get_option(name)
        except Exception:
            return None

    mem0 = used_mb()
    rng = np.random.default_rng(3)
    pos = np.array([rng.permutation(s) for _ in range(n)], dtype=np.int32)
    w = rng.uniform(-3, 3, (n, s, s))
    w01 = expit(w)
    anc = np.clip(rng.random((n, s, s)) - 0.5, 0, 1)

    def step():
        return eng.optimal_weights(pos, w01, anc, w, SIG0, SIG1, raise_on_fail=False)

    mem1 = None
    for _ in range(a.warmup):
        step()
        mem1 = used_mb() if mem1 is None else mem1
    ts = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        out = step()
        ts.append(time.perf_counter() - t0)
    print(json.dumps({"mode": a.mode, "S": s, "E": e, "chains": n, "steps": a.steps, "warmup": a.warmup,
                      "factored": eng.factored, "exact_form": eng.get_option("exact_form"),
                      "exact_cform": eng.get_option("exact_cform"),
                      "exact_form_used": opt("exact_form_used"), "exact_rc": opt("exact_rc"),
                      "exact_shared": opt("exact_shared"),
                      "step_mem_mb": None if mem0 is None or mem1 is None else mem1 - mem0,
                      "wall_ms_per_step_median": 1e3 * float(np.median(ts)),
                      "wall_ms_per_step_mean": 1e3 * float(np.mean(ts)),
                      "ll1_0": float(out[1][0]), "ll_dag_0": float(out[2][0])}))


if __name__ == "__main__":
    main()
