#!/usr/bin/env python
"""Rate of one order sweep in one launch (nemo_order_sweep_dev) against the loop of
relocation-score calls it replaces.

At S x E (default 64 x 2000, the C3 model) and each batch (default 16, 256 and
2048), with nvisit = S in label order and beta = 1, it times, with device events
after a warm-up and alternating in one run,

* ``gibbs``     nemo_order_sweep_dev with seeded uniforms,
* ``u0``        the same with u = 0: every node goes to position 0 (the upper bound
                of the re-walks and fresh log-sum-exps: a move at every visit),
* ``stay``      greedy against a huge min_gain: every row is scored, nothing moves
                (the lower bound: the walks alone),
* ``loop``      S successive nemo_score_relocations_dev calls: what
                ``gibbs_orders`` does per sweep today, without its host work,
* ``reloc``     one such call,

and the sweep kernel alone through the engine's own events (option timing_kernel
5).  One JSON line per run: medians over the rounds, min and max beside them.

    python tools/order_sweep_bench.py [--s 64] [--e 2000] [--batches 16,256,2048] [--rounds 5] [--iters 3]
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
    ap.add_argument("--batches", default="16,256,2048")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(",")]

    import torch

    from nemo import _lib, generator
    from nemo.engine import Engine

    m = generator.synthetic_nem(a.s, a.e, a.seed)
    eng = Engine.from_knockdown(m.observed_knockdown_mat, m.A, m.B)
    eng.set_option("exact", 0)
    nb = max(batches)
    eng.reserve(nb)
    lib = _lib.load()
    rng = np.random.default_rng(a.seed)
    s = a.s
    pos = np.stack([np.argsort(rng.permutation(s)) for _ in range(nb)]).astype(np.int32)
    w01 = rng.uniform(0.02, 0.98, (nb, s, s))                           # a soft full matrix per chain
    visit = np.ascontiguousarray(np.broadcast_to(np.arange(s, dtype=np.int32), (nb, s)))
    dpos0, dw, dvisit = torch.from_numpy(pos).cuda(), torch.from_numpy(w01).cuda(), torch.from_numpy(visit).cuda()
    du = torch.from_numpy(rng.random((nb, s))).cuda()
    dzero = torch.zeros((nb, s), dtype=torch.float64, device="cuda")
    dpout = torch.empty((nb, s), dtype=torch.int32, device="cuda")
    dll = torch.empty(nb, dtype=torch.float64, device="cuda")
    dq = torch.empty((nb, s), dtype=torch.int32, device="cuda")
    drow = torch.empty((nb, s, s), dtype=torch.float64, device="cuda")
    dvis = torch.empty((nb, s), dtype=torch.float64, device="cuda")
    dnm = torch.empty(nb, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def sweep(b, u, beta, min_gain):
        _lib.check(lib.nemo_order_sweep_dev(eng.handle, b, dpos0.data_ptr(), dw.data_ptr(), s, dvisit.data_ptr(),
                                            u.data_ptr(), beta, min_gain, 0, dpout.data_ptr(), None, dll.data_ptr(),
                                            dq.data_ptr(), drow.data_ptr(), dvis.data_ptr(), dnm.data_ptr(), st))

    def reloc(b):
        _lib.check(lib.nemo_score_relocations_dev(eng.handle, b, dpos0.data_ptr(), dw.data_ptr(), 0, dll.data_ptr(),
                                                  drow.data_ptr(), st))

    def loop(b):
        for _ in range(s):
            reloc(b)

    variants = {"gibbs": lambda b: sweep(b, du, 1.0, 0.0), "u0": lambda b: sweep(b, dzero, 1.0, 0.0),
                "stay": lambda b: sweep(b, dzero, float("inf"), 1e300), "loop": loop, "reloc": reloc}

    def timed(fn, b):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn(b)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters   # ms per call

    def kernel_ms(fn, b):
        eng.set_option("timing_kernel", 5)
        eng.timing(True)
        for _ in range(a.iters):
            fn(b)
        torch.cuda.synchronize()
        ms, n = eng.timing_read()
        eng.timing(False)
        eng.set_option("timing_kernel", 0)
        return ms / max(n, 1)

    out = {"S": s, "E": a.e, "nvisit": s, "rounds": a.rounds, "iters": a.iters, "build_id": _lib.build_id()}
    for b in batches:
        for fn in variants.values():   # warm-up
            fn(b)
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        kms = []
        for _ in range(a.rounds):      # alternating: every round times each variant once
            for k, fn in variants.items():
                ms[k].append(timed(fn, b))
            kms.append(kernel_ms(variants["gibbs"], b))
        key = f"b{b}"
        for k, v in ms.items():
            out[f"{key}_{k}_ms"] = round(float(np.median(v)), 4)
            out[f"{key}_{k}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
        out[f"{key}_gibbs_kernel_ms"] = round(float(np.median(kms)), 4)
        out[f"{key}_loop_over_gibbs"] = round(out[f"{key}_loop_ms"] / out[f"{key}_gibbs_ms"], 2)
        out[f"{key}_gibbs_over_reloc"] = round(out[f"{key}_gibbs_ms"] / out[f"{key}_reloc_ms"], 2)
        variants["gibbs"](b)
        torch.cuda.synchronize()
        out[f"{key}_gibbs_moves_per_sweep"] = round(float(dnm[:b].double().mean()), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
