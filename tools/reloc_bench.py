#!/usr/bin/env python
"""Rate of the exact relocation scores (nemo_score_relocations_dev) against the
loop they replace and against the move-score call.

At S x E (default 64 x 2000, the C3 model) and each batch (default 16, 256 and
2048) it times, with device events after a warm-up and alternating in one run,

* ``reloc``     nemo_score_relocations_dev (the two-pass forward, then
                reloc_reduce_kernel),
* ``moves``     nemo_score_moves_dev, fused: half the logs, no exp, no wave sum,
* ``brute``     nemo_score_dev with fact_kernel 2 (the fp64 MFMA score kernel):
                what scoring every relocation costs without this call, one full
                evaluation per relocated order, (S - 1)^2 distinct ones per
                order.  Its rate is measured on full batches of evaluations and
                divided by that count,

and reloc_reduce_kernel alone through the engine's own events (option
timing_kernel 4).  A sweep = the score change of every relocation of one order.
One JSON line per run: medians over the rounds, min and max beside them.

    python tools/reloc_bench.py [--s 64] [--e 2000] [--batches 16,256,2048] [--rounds 7] [--iters 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nem-mcmc-optimization_amd"))

# VALU instructions per step of a wave in reloc_reduce_kernel's walk, counted in
# the gfx950 code of the factored instance: 53 fp64 (two table exponentials, the
# FMA into the running sum, the add into the exponent, log1p_fast with log_fast,
# the wave sum's adds) and 32 others (the selects by the two bits and by the sign
# of the exponent, the integer halves of exp and log, addresses); the wave sum's
# twelve ds_bpermute are LDS instructions.  A wave64 VALU instruction holds its
# SIMD's port for 4 cycles.  A wave step serves 64 effects of one target; a node
# takes S - 1 steps per 64 effects
VALU_F64_PER_STEP = 53
VALU_OTHER_PER_STEP = 32
SIMDS, CLOCK_HZ, CYCLES = 1024, 2.4e9, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s", type=int, default=64)
    ap.add_argument("--e", type=int, default=2000)
    ap.add_argument("--batches", default="16,256,2048")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
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
    pos = np.stack([np.argsort(rng.permutation(a.s)) for _ in range(nb)]).astype(np.int32)
    w01 = (rng.random((nb, a.s, a.s)) < 0.3).astype(np.float64)     # a full 0/1 matrix per chain
    dpos, dw, dwa = torch.from_numpy(pos).cuda(), torch.from_numpy(w01).cuda(), torch.from_numpy(1.0 - w01).cuda()
    dll = torch.empty(nb, dtype=torch.float64, device="cuda")
    dd = torch.empty((nb, a.s, a.s), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    targets = (a.s - 1) ** 2        # distinct neighbouring orders (S (S - 1) entries, the adjacent ones twice)

    def reloc(b):
        _lib.check(lib.nemo_score_relocations_dev(eng.handle, b, dpos.data_ptr(), dw.data_ptr(), 0,
                                                  dll.data_ptr(), dd.data_ptr(), st))

    def moves(b):
        eng.set_option("moves_path", 0)
        _lib.check(lib.nemo_score_moves_dev(eng.handle, b, dpos.data_ptr(), dw.data_ptr(), dwa.data_ptr(), 0,
                                            dll.data_ptr(), dd.data_ptr(), st))

    def brute(b):
        eng.set_option("fact_kernel", 2)
        _lib.check(lib.nemo_score_dev(eng.handle, b, dpos.data_ptr(), dw.data_ptr(), 0, dll.data_ptr(), None, None,
                                      None, st))
        eng.set_option("fact_kernel", 0)

    variants = {"reloc": reloc, "moves": moves, "brute": brute}

    def timed(fn, b):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn(b)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters   # ms per call

    def kernel_ms(fn, b):
        eng.set_option("timing_kernel", 4)
        eng.timing(True)
        for _ in range(a.iters):
            fn(b)
        torch.cuda.synchronize()
        ms, n = eng.timing_read()
        eng.timing(False)
        eng.set_option("timing_kernel", 0)
        return ms / max(n, 1)

    out = {"S": a.s, "E": a.e, "targets": targets, "rounds": a.rounds, "iters": a.iters, "build_id": _lib.build_id()}
    steps_per_eval = a.s * (a.s - 1) * ((a.e + 63) // 64)   # wave steps
    for b in batches:
        for fn in variants.values():   # warm-up
            fn(b)
            fn(b)
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        kms = {"reloc": []}
        for _ in range(a.rounds):      # alternating: every round times each variant once
            for k, fn in variants.items():
                ms[k].append(timed(fn, b))
            for k in kms:
                kms[k].append(kernel_ms(variants[k], b))
        key = f"b{b}"
        for k, v in ms.items():
            med = float(np.median(v))
            out[f"{key}_{k}_ms"] = round(med, 4)
            out[f"{key}_{k}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
        out[f"{key}_brute_evals_per_s"] = round(b / out[f"{key}_brute_ms"] * 1e3, 1)
        out[f"{key}_brute_sweeps_per_s"] = round(b / out[f"{key}_brute_ms"] * 1e3 / targets, 3)
        for k in ("reloc",):
            out[f"{key}_{k}_sweeps_per_s"] = round(b / out[f"{key}_{k}_ms"] * 1e3, 1)
            out[f"{key}_{k}_over_brute"] = round(out[f"{key}_{k}_sweeps_per_s"] / out[f"{key}_brute_sweeps_per_s"], 1)
            out[f"{key}_{k}_over_moves"] = round(out[f"{key}_{k}_ms"] / out[f"{key}_moves_ms"], 2)
            med = float(np.median(kms[k]))
            out[f"{key}_{k}_kernel_ms"] = round(med, 4)
            out[f"{key}_{k}_kernel_ms_min_max"] = [round(min(kms[k]), 4), round(max(kms[k]), 4)]
        budget = SIMDS * CLOCK_HZ * out[f"{key}_reloc_kernel_ms"] * 1e-3
        steps = b * steps_per_eval
        out[f"{key}_reloc_valu_bound_fraction"] = round(
            steps * (VALU_F64_PER_STEP + VALU_OTHER_PER_STEP) * CYCLES / budget, 3)
        out[f"{key}_reloc_f64_valu_fraction"] = round(steps * VALU_F64_PER_STEP * CYCLES / budget, 3)
    ll, d = eng.score_relocations(pos[:4], w01[:4])
    out["reloc_path_used"] = eng.get_option("reloc_path_used")
    out["max_abs_dll"] = float(np.abs(d).max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
