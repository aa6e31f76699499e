"""Capture the row-shared exact_generic fixtures past one numpy buffer from
the reference implementation.

Runs ONLY in the build container, where the reference is importable, never
from a test (see ``make_generic_goldens.py``, whose duck-typed ``Model`` and
table seeds are reused; ``make_goldens.py`` loads the reference).  The tables
are ``generic_tables.py``'s "shared" kind -- per-effect log ratios R, T[i][j] =
R[j] -- at sizes whose np.sum runs over more than one buffer of 8192 terms.
The fixtures are data (seeds, table hashes, inputs and the reference's
outputs) and store no reference source.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_shared_goldens.py

Writes ``shared_step_4x9000.npz`` (buffers [8192, 808]) and
``shared_step_3x16500.npz`` ([8192, 8192, 116]): one
get_optimal_weights(init=True) from ``step_inputs`` -- eval #1's ll and column
sums cs, the new weights, the dag's score; the (S+1) x E order weights are left
out (the oracle gives them).  ``shared_traj_5x9000.npz``: 20 steps of method(),
seed 3, as ``generic_traj_9x300_shared.npz``.
"""
from __future__ import annotations

import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from generic_tables import generic_tables, step_inputs, table_sha256  # noqa: E402
from make_generic_goldens import TABLE_SEED, Model  # noqa: E402
from make_goldens import load_reference, quiet  # noqa: E402

SEED = TABLE_SEED["shared"]


def capture_step(ref_mcmc, s, e):
    u, t = generic_tables("shared", s, e, SEED)
    perm, w = step_inputs(s, SEED)
    mc = ref_mcmc.NEMOrderMCMC(Model(u, t), perm)
    mc.parent_weights = w.copy()
    dag_ll = quiet(mc.get_optimal_weights, init=True)
    # (cell_ratios: eval #1's cells, nem_order_mcmc.py:181; calculate_ll's cell_sums, :90)
    cs = np.logaddexp.reduce(mc.cell_ratios, axis=0)
    assert sum(cs) == mc.ll
    np.savez_compressed(os.path.join(HERE, f"shared_step_{s}x{e}.npz"), S=s, E=e, cap=0, seed=SEED,
                        sha256=table_sha256(u, t), perm=perm, W=w, ll1=mc.ll, cs=cs, W_new=mc.parent_weights,
                        dag_ll=dag_ll)
    print(f"shared step {s}x{e}: ll1={mc.ll} dag_ll={dag_ll}")


def capture_traj(ref_mcmc, s=5, e=9000, n_iter=20, seed=3):
    u, t = generic_tables("shared", s, e, SEED)
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
        os.path.join(HERE, f"shared_traj_{s}x{e}.npz"), S=s, E=e, kind="shared", table_seed=SEED,
        sha256=table_sha256(u, t), seed=seed, order0=order0, gamma=gamma, swap_prob=swap_prob, n_iter=n_iter,
        perm=np.array(rec["perm"]), i1=np.array(rec["i1"]), i2=np.array(rec["i2"]), acc=np.array(rec["acc"]),
        all_scores=np.array(mc.all_score_list), best_score=best, best_order=np.asarray(mc.best_order),
        best_dag=np.asarray(best_dag), final_W=mc.parent_weights,
        rng_state_after=np.array(random.getstate()[1], dtype=np.int64))
    print(f"shared traj {s}x{e}: best={best} accepts={int(np.sum(rec['acc']))}")


def main():
    _ref_nem, ref_mcmc, _ref_utils = load_reference()
    capture_step(ref_mcmc, 4, 9000)
    capture_step(ref_mcmc, 3, 16500)
    capture_traj(ref_mcmc)


if __name__ == "__main__":
    main()
