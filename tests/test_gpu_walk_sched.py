"""The issue order of the two-tile walk (i8l_walk2 in nemo_factored_i8.hip;
fact_kernel 10, 17 and 20) must not move a bit of ll.  A wait that is missing
or too short shows as wrong cells, and may show only when the LDS latency
varies, so the shapes are the smallest that reach every path of the walk --
one, two and four row blocks (S = 9, 20, 64); one tile, an odd tail, and a
wave that runs more than one iteration (E = 16, 40, 130); a wave that walks
two sets, so that an iteration follows a set finish (S = 64, E = 1040) -- and
one batch that fills every CU with two blocks.

tests/golden/i8l_walk_parent.npz holds fact_kernel 10's ll on these inputs as
the build before the walk was reordered computed it
(tools/make_walk_golden.py); fact_kernel 16 walks one tile per iteration and
is the reference for the arithmetic, the oracle for the score."""
import numpy as np
import pytest

import nemo_oracle as no
import walk_sched_inputs as wi
from conftest import golden
from nemo.engine import Engine

pytestmark = pytest.mark.gpu

PAIR_TOL = 1e-9     # 10 against 16 (tests/test_gpu_cinit16.py)
ORACLE_TOL = 1e-6
TWO_TILE = (10, 17, 20)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def parent():
    return golden(wi.GOLDEN)


@pytest.mark.parametrize("s,e", wi.CASES)
def test_walk_bits_and_values(s, e, parent):
    m, perms, pos, w01 = wi.inputs(s, e)
    t = m.get_score_tensor()
    n = len(w01)
    eng = Engine.for_nem(m)
    try:
        eng.set_option("exact", 0)
        for cap in wi.CAPS:
            ref = np.array([no.order_score(m.U, t, perms[c], w01[c], cap=cap) for c in range(n)])
            gold = parent[wi.key(s, e, cap)]
            eng.set_option("fact_kernel", 16)
            assert eng.score_kernel(cap)[0] == 16
            one = eng.score(pos, w01, cap=cap)
            for fk in TWO_TILE:
                eng.set_option("fact_kernel", fk)
                assert eng.score_kernel(cap)[0] == fk
                ll = eng.score(pos, w01, cap=cap)
                print(f"S={s} E={e} cap={cap} fk={fk} bits differ from the parent's in "
                      f"{int(np.sum(_bits(ll) != _bits(gold)))} of {n}, max|ll-fk16|={np.max(np.abs(ll - one)):.3e} "
                      f"max|ll-oracle|={np.max(np.abs(ll - ref)):.3e}")
                assert np.array_equal(_bits(ll), _bits(gold)), (fk, cap)
                assert np.max(np.abs(ll - one)) <= PAIR_TOL, (fk, cap)
                assert np.max(np.abs(ll - ref)) <= ORACLE_TOL, (fk, cap)
                # one evaluation alone (the block-split path): the same bits
                alone = eng.score(pos[3:4], w01[3:4], cap=cap)
                assert _bits(alone)[0] == _bits(ll)[3], (fk, cap)
    finally:
        eng.close()


def test_walk_bits_on_a_crowded_cu(parent):
    """1200 evaluations, the seven inputs repeated cyclically: two blocks per
    CU and every wave in contention for the LDS; each ll is its small-batch
    value (and so the parent's), bit for bit."""
    s, e, batch = wi.CROWD
    m, _, pos, w01 = wi.inputs(s, e)
    idx = np.arange(batch) % len(w01)
    eng = Engine.for_nem(m)
    try:
        eng.set_option("exact", 0)
        for cap in wi.CAPS:
            gold = parent[wi.key(s, e, cap)]
            for fk in TWO_TILE:
                eng.set_option("fact_kernel", fk)
                assert eng.score_kernel(cap)[0] == fk
                small = eng.score(pos, w01, cap=cap)
                big = eng.score(pos[idx], w01[idx], cap=cap)
                bad = np.flatnonzero(_bits(big) != _bits(small)[idx])
                print(f"S={s} E={e} cap={cap} fk={fk} batch={batch}: {len(bad)} ll differ from the small batch's")
                assert len(bad) == 0, (fk, cap, bad[:8])
                assert np.array_equal(_bits(small), _bits(gold)), (fk, cap)
    finally:
        eng.close()
