#!/usr/bin/env python
"""Time of one ``nemo_real_sweep`` (the true-graph fit's sweep).

At S x E (default: BASELINE config C3, 64 x 2000, the observed call) it runs
the fit's first sweeps, then times each sweep's call again from its recorded
input weights: after a warm-up, ``--iters`` calls per round, ``--rounds``
rounds, alternating the sweeps.  Per sweep it reports

* ``pairs_ms``   the pair-solve kernel alone (device events of the context's
                 timing interface, option ``timing_kernel`` 2),
* ``call_ms``    the host-pointer call (copies in, evaluation, solves, copies
                 out, synchronise) by the host clock,
* ``nfev``       objective evaluations per solve from ``info`` (each is one
                 pass over the order weights at two points),
* ``logs``       logs the kernel takes: pairs (S+1) E (nfev + 1), the + 1 being
                 the x-independent sum taken once per pair,
* ``valu_floor_ms``  logs x VALU_PER_LOG fp64-rate wave instructions over the
                 device's vector issue rate -- the estimate the measured time
                 is to be read against, not a measurement.

With ``--ref-json`` (the file tests/golden/make_real_score_goldens.py --time
writes on the CPU machine) the ratio to the reference's one sweep is added.
One JSON line.

    python tools/real_score_time.py [--s 64 --e 2000 --seed 2] [--sweeps 2] [--rounds 5] [--iters 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "nem-mcmc-optimization_amd"))

# per element and point: one multiply by alpha shared by the two points (0.5),
# the fma, log_fast's 11 fp64 + 5 integer operations, the add into the sum
VALU_PER_LOG = 0.5 + 1 + 16 + 1
SIMDS, CLOCK_HZ, CYCLES_PER_F64_WAVE_OP = 256 * 4, 2.4e9, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s", type=int, default=0)
    ap.add_argument("--e", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sweeps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--ref-json", default=os.path.join(REPO, "tests", "golden", "real_score_time_ref.json"))
    a = ap.parse_args()

    from nemo import _lib, generator
    from nemo.engine import Engine

    m = generator.synthetic_nem(a.s, a.e, a.seed) if a.s else generator.config_nem("C3")
    s, e = m.num_s, m.num_e
    eng = Engine.for_nem(m)
    adj = np.asarray(m.adj_matrix)
    order = np.argsort(np.sum(adj, axis=1))[::-1]
    pos = np.empty(s, dtype=np.int32)
    pos[order] = np.arange(s, dtype=np.int32)
    mask = pos[None, :] < pos[:, None]
    npairs = int(mask.sum())

    inputs, w = [], np.where(mask, 0.5, 0.0)
    lls = []
    for _ in range(a.sweeps):          # the fit's first sweeps (also the warm-up of every shape)
        inputs.append(w)
        w_out, ll, info = eng.real_sweep(pos, w)
        w = np.where(mask, w_out[0], 0.0)
        lls.append(float(ll[0]))
    for w_in in inputs:
        eng.real_sweep(pos, w_in)

    eng.set_option("timing_kernel", 2)
    pairs_ms = [[] for _ in inputs]
    call_ms = [[] for _ in inputs]
    nfev = []
    for _ in range(a.rounds):
        for k, w_in in enumerate(inputs):
            eng.timing(True)           # (resets the event pool)
            t0 = time.perf_counter()
            for _ in range(a.iters):
                _, _, info = eng.real_sweep(pos, w_in)
            call_ms[k].append((time.perf_counter() - t0) * 1e3 / a.iters)
            ms, n = eng.timing_read()
            assert n == a.iters
            pairs_ms[k].append(ms / n)
            eng.timing(False)
            if len(nfev) <= k:
                ev = info[0][mask] >> 16
                nfev.append((float(ev.mean()) / 2, int(ev.max()) // 2,
                             int(((info[0][mask] & 15) >= _lib.LBFGSB_ABNORMAL).sum())))
    eng.set_option("timing_kernel", 0)

    out = {"S": s, "E": e, "pairs": npairs, "rounds": a.rounds, "iters": a.iters, "build_id": _lib.build_id(),
           "factored": eng.factored, "sweep_ll": lls, "sweeps": []}
    for k in range(len(inputs)):
        mean_ev, max_ev, abnormal = nfev[k]
        logs = npairs * (s + 1) * e * (2 * mean_ev + 1)
        floor = logs / 64 * VALU_PER_LOG * CYCLES_PER_F64_WAVE_OP / SIMDS / CLOCK_HZ * 1e3
        med = float(np.median(pairs_ms[k]))
        out["sweeps"].append({
            "sweep": k, "pairs_ms": round(med, 4),
            "pairs_ms_min_max": [round(min(pairs_ms[k]), 4), round(max(pairs_ms[k]), 4)],
            "call_ms": round(float(np.median(call_ms[k])), 4),
            "evaluations_per_solve": round(mean_ev, 3), "evaluations_max": max_ev, "abnormal": abnormal,
            "logs": int(logs), "valu_floor_ms": round(floor, 4), "floor_over_measured": round(floor / med, 3)})
    if os.path.exists(a.ref_json) and not a.s:
        with open(a.ref_json) as fh:
            ref = json.load(fh)
        if (ref["S"], ref["E"]) == (s, e):
            out["reference_cpu"] = ref["cpu"]
            out["reference_one_sweep_s"] = round(ref["seconds_one_sweep"], 3)
            out["reference_over_call"] = round(ref["seconds_one_sweep"] * 1e3 / out["sweeps"][0]["call_ms"], 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
