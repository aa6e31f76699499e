#!/usr/bin/env python
"""Rate and latency of the order score at per-gene error rates (nemo_score_rates_dev).

At S x E (default 64 x 2000) and a batch (default 2048) it times, with device
events after a warm-up and alternating in one run,

* ``rates``        nemo_score_rates_dev with d ll / d w01 (every evaluation at
                   its own per-gene rates),
* ``rates-nogw``   the same without d ll / d w01 (ll, dA, dB alone),
* ``grad``         nemo_score_grad_dev on the same engine, grad_path 0 (the
                   fused kernel this one is a variant of, at the staged rates),

and the same three for one evaluation (latency).  One JSON line per run.

    python tools/rates_bench.py [--s 64] [--e 2000] [--batch 2048] [--rounds 5] [--iters 10]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nem-mcmc-optimization_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s", type=int, default=64)
    ap.add_argument("--e", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    import torch
    from scipy.special import expit

    from nemo import _lib, generator
    from nemo.engine import Engine

    m = generator.synthetic_nem(a.s, a.e, a.seed)
    eng = Engine.from_knockdown(m.observed_knockdown_mat, m.A, m.B)
    eng.set_option("exact", 0)
    eng.set_option("grad_path", 0)
    eng.reserve(a.batch)
    lib = _lib.load()
    rng = np.random.default_rng(a.seed)
    pos = np.stack([np.argsort(rng.permutation(a.s)) for _ in range(a.batch)]).astype(np.int32)
    w01 = expit(rng.uniform(-3.0, 3.0, (a.batch, a.s, a.s)))
    al, be = rng.uniform(0.01, 0.3, (2, a.batch, a.s))
    rates = np.ascontiguousarray(np.stack([np.log(al / (1 - be)), np.log(be / (1 - al))], axis=1))
    dpos, dw, dr = torch.from_numpy(pos).cuda(), torch.from_numpy(w01).cuda(), torch.from_numpy(rates).cuda()
    dll = torch.empty(a.batch, dtype=torch.float64, device="cuda")
    dg = torch.empty((a.batch, a.s, a.s), dtype=torch.float64, device="cuda")
    ddr = torch.empty_like(dr)
    st = torch.cuda.current_stream().cuda_stream

    def rates_fn(want_gw):
        def run(b):
            _lib.check(lib.nemo_score_rates_dev(eng.handle, b, dpos.data_ptr(), dw.data_ptr(), dr.data_ptr(), 0,
                                                dll.data_ptr(), ddr.data_ptr(), dg.data_ptr() if want_gw else None, st))
        return run

    def grad(b):
        _lib.check(lib.nemo_score_grad_dev(eng.handle, b, dpos.data_ptr(), dw.data_ptr(), 0, dll.data_ptr(),
                                           dg.data_ptr(), st))

    variants = {"rates": rates_fn(True), "rates-nogw": rates_fn(False), "grad": grad}

    def timed(fn, b):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn(b)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters   # ms per call

    out = {"S": a.s, "E": a.e, "batch": a.batch, "rounds": a.rounds, "iters": a.iters, "build_id": _lib.build_id()}
    for b, key in ((a.batch, "batch"), (1, "one")):
        for fn in variants.values():   # warm-up
            fn(b)
            fn(b)
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(a.rounds):      # alternating: every round times each variant once
            for k, fn in variants.items():
                ms[k].append(timed(fn, b))
        for k, v in ms.items():
            med = float(np.median(v))
            out[f"{key}_{k}_ms"] = round(med, 4)
            out[f"{key}_{k}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
            if key == "batch":
                out[f"{key}_{k}_evals_per_s"] = round(b / med * 1e3, 1)
    out["batch_rates_over_grad"] = round(out["batch_rates_ms"] / out["batch_grad_ms"], 3)
    # at the staged scalar rates the two calls agree to rounding
    ll_r, _, _, g_r = eng.score_rates(pos[:4], w01[:4], float(m.A), float(m.B))
    ll_g, g_g = eng.score_grad(pos[:4], w01[:4])
    out["max_abs_ll_diff_rates_grad"] = float(np.abs(ll_r - ll_g).max())
    out["max_abs_grad_diff_rates_grad"] = float(np.abs(g_r - g_g).max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
