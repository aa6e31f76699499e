"""The seeded inputs of tests/test_gpu_walk_sched.py, shared with
tools/make_walk_golden.py (which records fact_kernel 10's ll on them from the
build that preceded the walk's software pipeline): the shapes and the seven
weight sets of tests/test_gpu_cinit16.py, and S = 64 with E = 1040 (9 sets of
8 tiles: wave 0 of the 8 walks two sets, so an iteration follows a set finish).
"""
import numpy as np
from scipy.special import expit

CASES = [(s, e) for s in (9, 20, 64) for e in (16, 40, 130)] + [(64, 1040)]
CAPS = (0, 7)
CROWD = (64, 130, 1200)   # S, E, batch: two blocks per CU on 256 CUs
GOLDEN = "i8l_walk_parent.npz"


def key(s, e, cap):
    return f"ll_s{s}_e{e}_cap{cap}"


def _pos(perm):
    pos = np.empty(len(perm), dtype=np.int32)
    pos[np.asarray(perm)] = np.arange(len(perm))
    return pos


def weights(rng, s):
    sat = np.where(rng.random((s, s)) < 0.5, 1e-12, 1.0 - 1e-12)
    return np.stack([expit(rng.uniform(-3, 3, (s, s))), expit(rng.uniform(-30, 30, (s, s))), np.ones((s, s)),
                     sat, np.full((s, s), 1e-12), np.full((s, s), 1.0 - 1e-12), sat.T.copy()])


def inputs(s, e):
    """(model, perms, pos, w01) of one case: seven evaluations."""
    from nemo import generator
    m = generator.synthetic_nem(s, e, 2)
    rng = np.random.default_rng(1000 * s + e)
    w01 = weights(rng, s)
    perms = [rng.permutation(s) for _ in range(len(w01))]
    pos = np.array([_pos(p) for p in perms])
    return m, perms, pos, w01
