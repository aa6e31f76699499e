#!/usr/bin/env python
"""Rate and latency of the order-score gradient (nemo_score_grad_dev).

At S x E (default 64 x 2000) and a batch (default 2048) it times, with device
events after a warm-up and alternating in one run,

* ``fused``     nemo_score_grad_dev, option grad_path 0 (the fused kernel),
* ``two-pass``  nemo_score_grad_dev, option grad_path 1,
* ``score+ow``  nemo_score_dev with the order weights requested, fact_kernel 1:
                the only way to a gradient's ingredients without the kernels
                above (it stops at the order weights: no gradient is formed),

and the same three for one evaluation (latency).  One JSON line per run.

    python tools/grad_bench.py [--s 64] [--e 2000] [--batch 2048] [--rounds 5] [--iters 10]
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
    eng.reserve(a.batch)
    lib = _lib.load()
    rng = np.random.default_rng(a.seed)
    pos = np.stack([np.argsort(rng.permutation(a.s)) for _ in range(a.batch)]).astype(np.int32)
    w01 = expit(rng.uniform(-3.0, 3.0, (a.batch, a.s, a.s)))
    dpos, dw = torch.from_numpy(pos).cuda(), torch.from_numpy(w01).cuda()
    dll = torch.empty(a.batch, dtype=torch.float64, device="cuda")
    dg = torch.empty((a.batch, a.s, a.s), dtype=torch.float64, device="cuda")
    dow = torch.empty((a.batch, a.s + 1, a.e), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def grad(path):
        def run(b):
            eng.set_option("grad_path", path)
            _lib.check(lib.nemo_score_grad_dev(eng.handle, b, dpos.data_ptr(), dw.data_ptr(), 0, dll.data_ptr(),
                                               dg.data_ptr(), st))
        return run

    def score_ow(b):
        eng.set_option("fact_kernel", 1)
        _lib.check(lib.nemo_score_dev(eng.handle, b, dpos.data_ptr(), dw.data_ptr(), 0, dll.data_ptr(), None, None,
                                      dow.data_ptr(), st))
        eng.set_option("fact_kernel", 0)

    variants = {"fused": grad(0), "two-pass": grad(1), "score+ow": score_ow}

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
    eng.set_option("grad_path", 0)
    ll_f, g_f = eng.score_grad(pos[:4], w01[:4])
    out["grad_path_used_auto"] = eng.get_option("grad_path_used")
    eng.set_option("grad_path", 1)
    ll_t, g_t = eng.score_grad(pos[:4], w01[:4])
    out["max_abs_grad_diff_fused_two_pass"] = float(np.abs(g_f - g_t).max())
    out["max_abs_grad"] = float(np.abs(g_f).max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
