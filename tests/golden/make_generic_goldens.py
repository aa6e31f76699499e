"""Capture the exact_generic fixtures from the reference implementation.

Runs ONLY in the build container, where the reference is importable (see
``make_goldens.py``, whose flat import, ``wandb`` stub and ``opt_weights``
pass-through are reused).  The reference's ``NEMOrderMCMC`` is driven with a
duck-typed model object that holds real-valued tables (``generic_tables.py``)
in place of a ``NEM``; the fixtures are data (seeds, table hashes, inputs and
the reference's outputs) and store no reference source.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_generic_goldens.py

Writes ``generic_step_{6x130,9x300,12x1000}.npz`` (one
get_optimal_weights(init=True) per table kind), ``generic_step_9x300_cap3.npz``
(parents_list cut to the last 3 predecessors, as ``capture_capped_step``),
``generic_traj_9x300_{shared,own}.npz`` (20 steps of method(), seed 3) and
``generic_meta.json`` (the versions at capture).
"""
from __future__ import annotations

import json
import os
import platform
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from generic_tables import KINDS, generic_tables, step_inputs, table_sha256  # noqa: E402
from make_goldens import capture_replica_exchange, load_reference, quiet  # noqa: E402

TABLE_SEED = {"shared": 11, "own": 12}


class Model:
    """What NEMOrderMCMC.__init__ reads of a NEM (nem_order_mcmc.py:37-44)."""
    observed_knockdown_mat = None

    def __init__(self, u, t):
        self.num_s, self.num_e = t.shape[0], t.shape[2]
        self.U, self._t = u, t

    def get_score_tables(self, _):
        return self._t


def capture_step(ref_mcmc, s, e, cap=0):
    """One get_optimal_weights(init=True) (nem_order_mcmc.py:172-208) per table
    kind from (perm, raw W) of ``step_inputs``: eval #1's ll and order weights,
    the new weights and the dag's score.  With a cap, parents_list is cut to
    the last <= cap predecessors and W to those entries."""
    out = dict(S=s, E=e, cap=cap)
    for kind in KINDS:
        seed = TABLE_SEED[kind]
        u, t = generic_tables(kind, s, e, seed)
        perm, w = step_inputs(s, seed)
        mc = ref_mcmc.NEMOrderMCMC(Model(u, t), perm)
        if cap:
            capped = np.empty(s, dtype=object)
            for i, pl in enumerate(mc.parents_list):
                capped[i] = pl[max(0, len(pl) - cap):]
            mc.parents_list = capped
            keep = np.zeros((s, s), dtype=bool)
            for i, pl in enumerate(capped):
                keep[i, pl] = True
            w = np.where(keep, w, 0.0)
        mc.parent_weights = w.copy()
        dag_ll = quiet(mc.get_optimal_weights, init=True)
        out.update({f"{kind}_seed": seed, f"{kind}_sha256": table_sha256(u, t), f"{kind}_perm": perm,
                    f"{kind}_W": w, f"{kind}_ll1": mc.ll, f"{kind}_ow": mc.order_weights,
                    f"{kind}_W_new": mc.parent_weights, f"{kind}_dag_ll": dag_ll})
        print(f"generic step {s}x{e} cap={cap} {kind}: ll1={mc.ll} dag_ll={dag_ll}")
    name = f"generic_step_{s}x{e}" + (f"_cap{cap}" if cap else "")
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)


def capture_traj(ref_mcmc, kind, s=9, e=300, n_iter=20, seed=3):
    """method() (nem_order_mcmc.py:257-310) for n_iter steps from the identity
    order, random.seed(seed), gamma = 2S/E, the default swap_prob: every
    proposal and accept, every score, the best score and order, the final
    weights and the final ``random`` state."""
    u, t = generic_tables(kind, s, e, TABLE_SEED[kind])
    rec = {"perm": [], "i1": [], "i2": [], "acc": []}
    cls = ref_mcmc.NEMOrderMCMC
    orig_new, orig_acc = cls.get_new_order, cls.accepting

    def new_order(self, curr, swap_prob=0.95):
        p, i1, i2 = orig_new(self, curr, swap_prob=swap_prob)
        rec["perm"].append(p.copy())
        rec["i1"].append(i1)
        rec["i2"].append(i2)
        return p, i1, i2

    def accepting(self, *a):
        r = orig_acc(self, *a)
        rec["acc"].append(bool(r[0]))
        return r

    order0 = np.arange(s)
    gamma, swap_prob = 2.0 * s / e, 0.95
    cls.get_new_order, cls.accepting = new_order, accepting
    try:
        random.seed(seed)
        mc = cls(Model(u, t), order0)
        best, best_dag = quiet(mc.method, n_iterations=n_iter, gamma=gamma, swap_prob=swap_prob)
    finally:
        cls.get_new_order, cls.accepting = orig_new, orig_acc
    np.savez_compressed(
        os.path.join(HERE, f"generic_traj_{s}x{e}_{kind}.npz"), S=s, E=e, kind=kind, table_seed=TABLE_SEED[kind],
        sha256=table_sha256(u, t), seed=seed, order0=order0, gamma=gamma, swap_prob=swap_prob, n_iter=n_iter,
        perm=np.array(rec["perm"]), i1=np.array(rec["i1"]), i2=np.array(rec["i2"]), acc=np.array(rec["acc"]),
        all_scores=np.array(mc.all_score_list), best_score=best, best_order=np.asarray(mc.best_order),
        best_dag=np.asarray(best_dag), final_W=mc.parent_weights,
        rng_state_after=np.array(random.getstate()[1], dtype=np.int64))
    print(f"generic traj {s}x{e} {kind}: best={best} accepts={int(np.sum(rec['acc']))}")


def main():
    import scipy
    _ref_nem, ref_mcmc, _ref_utils = load_reference()
    for s, e in ((6, 130), (9, 300), (12, 1000)):
        capture_step(ref_mcmc, s, e)
    capture_step(ref_mcmc, 9, 300, cap=3)
    for kind in KINDS:
        capture_traj(ref_mcmc, kind)
    # replica_exchange_method (nem_order_mcmc.py:344-363) on the row-shared
    # tables: 10 replicas, 2 rounds of 3 steps (make_goldens.py's capture)
    u, t = generic_tables("shared", 9, 300, TABLE_SEED["shared"])
    capture_replica_exchange(_ref_nem, ref_mcmc, _ref_utils, n_exchange=2, n_iter=3, seed=5,
                             model=(Model(u, t), np.arange(9)), name="generic_9x300_shared")
    meta = dict(python=platform.python_version(), numpy=np.__version__, scipy=scipy.__version__,
                machine=platform.machine())
    with open(os.path.join(HERE, "generic_meta.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
    print(meta)


if __name__ == "__main__":
    main()
