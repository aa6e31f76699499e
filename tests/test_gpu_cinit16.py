"""Slice 4's C-init by one 16-bit shift in the two-tile walks of the log2 int8
kernels (fact_kernel 10, 17 and 20, and 18 for 64 < S <= 128; i8l_cinit16 in
nemo_factored_i8.hip), on
the smallest shapes that reach every path: one, two and four row blocks
(S = 9, 20, 64), one tile, three tiles (the odd tail repeats a tile) and
nine (E = 16, 40, 130).  fact_kernel 16 walks one tile per iteration with no
C-init in slice 4, so it is the reference for the walk's arithmetic; the
oracle is the reference for the score.  A shift that kept the destination's
high half would break every cell, the saturated weights put large |Delta|
and both ends of T_0's low field into play."""
import numpy as np
import pytest
from scipy.special import expit

import nemo_oracle as no
from nemo import generator
from nemo.engine import Engine

pytestmark = pytest.mark.gpu

PAIR_TOL = 1e-9     # 10 against 16 (test_int8_kernel_bits_independent_of_split)
ORACLE_TOL = 1e-6


def _pos(perm):
    pos = np.empty(len(perm), dtype=np.int32)
    pos[np.asarray(perm)] = np.arange(len(perm))
    return pos


def _weights(rng, s):
    sat = np.where(rng.random((s, s)) < 0.5, 1e-12, 1.0 - 1e-12)
    return np.stack([expit(rng.uniform(-3, 3, (s, s))), expit(rng.uniform(-30, 30, (s, s))), np.ones((s, s)),
                     sat, np.full((s, s), 1e-12), np.full((s, s), 1.0 - 1e-12), sat.T.copy()])


def _check(s, e, two_tile, one_tile):
    m = generator.synthetic_nem(s, e, 2)
    t = m.get_score_tensor()
    eng = Engine.for_nem(m)
    try:
        rng = np.random.default_rng(1000 * s + e)
        w01 = _weights(rng, s)
        n = len(w01)
        perms = [rng.permutation(s) for _ in range(n)]
        pos = np.array([_pos(p) for p in perms])
        eng.set_option("exact", 0)
        for cap in (0, 7):
            ref = np.array([no.order_score(m.U, t, perms[c], w01[c], cap=cap) for c in range(n)])
            eng.set_option("fact_kernel", one_tile)
            assert eng.score_kernel(cap)[0] == one_tile
            one = eng.score(pos, w01, cap=cap)
            print(f"S={s} E={e} cap={cap} fk={one_tile} max|ll-oracle|={np.max(np.abs(one - ref)):.3e}")
            assert np.max(np.abs(one - ref)) <= ORACLE_TOL, (one_tile, cap)
            for fk in two_tile:
                eng.set_option("fact_kernel", fk)
                assert eng.score_kernel(cap)[0] == fk
                ll = eng.score(pos, w01, cap=cap)
                print(f"S={s} E={e} cap={cap} fk={fk} max|ll-fk{one_tile}|={np.max(np.abs(ll - one)):.3e} "
                      f"max|ll-oracle|={np.max(np.abs(ll - ref)):.3e}")
                assert np.max(np.abs(ll - one)) <= PAIR_TOL, (fk, cap)
                assert np.max(np.abs(ll - ref)) <= ORACLE_TOL, (fk, cap)
                # one evaluation alone (another block split): the same bits
                assert eng.score(pos[3:4], w01[3:4], cap=cap)[0] == ll[3], (fk, cap)
    finally:
        eng.close()


@pytest.mark.parametrize("e", [16, 40, 130])
@pytest.mark.parametrize("s", [9, 20, 64])
def test_two_tile_walk_cinit16(s, e):
    _check(s, e, two_tile=(10, 17, 20), one_tile=16)


@pytest.mark.parametrize("s", [65, 128])
def test_wide_two_tile_walk_cinit16(s):
    """score_i8w_kernel's two-tile walk (18) takes the same C-init over its two
    K halves; 19 walks one tile per iteration with none."""
    _check(s, 40, two_tile=(18,), one_tile=19)
