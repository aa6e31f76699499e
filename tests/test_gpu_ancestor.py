"""GPU: the step's W~ and ancestor_x made on the device (csrc/nemo_ancestor.hip:
getrf + getri of scipy's OpenBLAS restated) against scipy's expit and
scipy.linalg.inv -- the reference's own calls (nem_order_mcmc.py:98-103,
:185) -- to the bit.

* Smooth inputs (W uniform(-4, 4), stale entries uniform(0, 1)) at ten sizes,
  with and without a cap (test_ancestor_equals_scipy_bit_for_bit).
* Every S from 2 to 64, each its own case, on the families of
  tests/ancestor_inputs.py (saturated, few-valued, subnormal and 1 - 2^-53,
  +-40 logits, stale entries of either sign, the identity and the reversed
  order under the caps 0, 1, 3, S - 2, S - 1, S + 5, chains with a non-zero
  pivot below DBL_MIN, planted zero columns, an overflowing chain): a chain
  whose inverse is
  finite equals the host's W~ and ancestor_x to the bit, signed zeros
  included, with flag 0; a chain on which scipy raises LinAlgError (from
  getrf's info or from getri's) has flag bit 1; a chain whose inverse is
  non-finite without an error has flag 4 alone; and neither disturbs the
  chains beside it in the batch.
* One chain alone and 300 chains (more blocks than CUs) at S = 47 and 64.
* scipy's own errors through the engine: a singular I - W~ at S = 7, 16, 40
  and 64, a non-finite one at S = 16; the engine steps afterwards.
* Flag 4 through the engine and through a chain batch at S = 33 and 64: the
  step is recomputed from the host's W~ / ancestor_x and equals the step the
  host's inputs give (NaN for NaN).
* The fused step from W against the fused step from the host's W~ /
  ancestor_x; chain batches with the device's ancestor_x against the host's
  (InvPool) step for step.

No tolerance anywhere: bit equality, equal-NaN equality on the recompute
path, or a flag value."""
import numpy as np
import pytest
from scipy.linalg import LinAlgError, inv
from scipy.special import expit

import ancestor_inputs as ai
from nemo import _lib, generator
from nemo.chains import ChainBatch
from nemo.engine import Engine
from nemo.invpool import InvPool
from nemo.nem_order_mcmc import SIG0, SIG1, permissible_batch

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _host(pos, w, cap=0):
    """chains._prepare's host computation: scipy's expit and inv."""
    mask = permissible_batch(pos, cap)
    sig = w.copy()
    sig[mask] = expit(w[mask])
    eye = np.identity(w.shape[-1])
    return sig, np.stack([np.clip(inv(eye - s) - eye, 0, 1) for s in sig])


def _weights(rng, pos, stale, diag=False):
    n, s = pos.shape
    mask = permissible_batch(pos)
    w = np.where(mask, rng.uniform(-4, 4, (n, s, s)), 0.0)
    if stale:   # left by earlier orders: expit(x*) values outside today's parents
        w = np.where(~mask & (rng.random((n, s, s)) < 0.15), rng.uniform(0, 1, (n, s, s)), w)
    for k in range(n):
        np.fill_diagonal(w[k], rng.uniform(-0.5, 0.5, s) if diag else 0.0)
    return w


def _device(eng, pos, w, cap=0):
    import torch
    n = w.shape[0]
    dpos = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.int32)).cuda()
    dw = torch.from_numpy(np.ascontiguousarray(w)).cuda()
    d01, danc = torch.empty_like(dw), torch.empty_like(dw)
    dfl = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.load().nemo_ancestor_dev(eng._ctx, n, dpos.data_ptr(), dw.data_ptr(), int(cap), d01.data_ptr(),
                                             danc.data_ptr(), dfl.data_ptr(), st))
    torch.cuda.synchronize()
    return d01.cpu().numpy(), danc.cpu().numpy(), dfl.cpu().numpy()


@pytest.mark.parametrize("s", [2, 3, 5, 11, 16, 17, 33, 48, 63, 64])
def test_ancestor_equals_scipy_bit_for_bit(s):
    eng = Engine.for_nem(generator.synthetic_nem(s, 40, 0))
    rng = np.random.default_rng(100 + s)
    n = 24
    pos = np.array([rng.permutation(s) for _ in range(n)], dtype=np.int32)
    for stale, diag in ((False, False), (True, False), (True, True)):
        w = _weights(rng, pos, stale, diag)
        for cap in ((0, 3) if s >= 5 else (0,)):
            sig, anc = _host(pos, w, cap)
            d01, danc, fl = _device(eng, pos, w, cap)
            assert np.array_equal(fl, np.zeros(n)), fl
            assert _bits_equal(d01, sig), (stale, diag, cap)
            assert _bits_equal(danc, anc), (stale, diag, cap)
    eng.close()


def test_ancestor_flags_and_scipys_errors():
    m = generator.synthetic_nem(16, 40, 0)
    eng = Engine.for_nem(m)
    rng = np.random.default_rng(4)
    pos = np.array([rng.permutation(16) for _ in range(3)], dtype=np.int32)
    w = _weights(rng, pos, True)
    i = int(np.argmin(pos[1]))        # first in chain 1's order: no permissible parents
    w[1, i, :] = 0.0
    w[1, i, i] = 1.0                  # row i of I - W~ all zero: singular
    w[2, 5, 5] = np.inf               # I - W~ not finite
    _, _, fl = _device(eng, pos, w)
    assert fl[0] == 0 and fl[1] == 1 and fl[2] & 2
    with pytest.raises(LinAlgError):
        eng.optimal_weights_w(pos[:2], w[:2], SIG0, SIG1)
    with pytest.raises(ValueError):
        eng.optimal_weights_w(pos[2:], w[2:], SIG0, SIG1)
    # the host's own calls raise the same
    with pytest.raises(LinAlgError):
        _host(pos[1:2], w[1:2])
    with pytest.raises(ValueError):
        _host(pos[2:], w[2:])
    # the engine still steps afterwards
    out = eng.optimal_weights_w(pos[:1], w[:1], SIG0, SIG1, raise_on_fail=False)
    assert np.isfinite(out[3]).all()
    eng.close()


@pytest.mark.parametrize("cap,overlap", [(0, 1), (3, 1), (0, 0)])
def test_step_from_w_equals_step_from_host_ancestor(cap, overlap):
    """nemo_optimal_weights_w (W in) against nemo_optimal_weights with the
    host's W~ / ancestor_x: every output to the bit, direct and queued, with
    ancestor_x beside eval #1 on a second stream (option anc_overlap 1, the
    default) or in line."""
    m = generator.config_nem("C3")
    eng = Engine.for_nem(m)
    eng.set_option("anc_overlap", overlap)
    rng = np.random.default_rng(21 + cap)
    n = 16
    pos = np.array([rng.permutation(64) for _ in range(n)], dtype=np.int32)
    w = _weights(rng, pos, True)
    sig, anc = _host(pos, w, cap)
    ref = eng.optimal_weights(pos, sig, anc, w, SIG0, SIG1, cap=cap, raise_on_fail=False)
    got = eng.optimal_weights_w(pos, w, SIG0, SIG1, cap=cap, raise_on_fail=False)
    assert _bits_equal(got[0], sig) and _bits_equal(got[1], anc)
    for a, b in zip(got[2:5], ref[:3]):
        assert _bits_equal(a, b)
    assert np.array_equal(got[5], ref[3])
    # queued: two calls in flight, ended in order
    calls = [eng.bind_optimal_weights_w(pos[h::2], w[h::2], SIG0, SIG1, cap=cap) for h in (0, 1)]
    for c in calls:
        c.begin()
    for h, c in enumerate(calls):
        c.end()
        wn, ll1, lld, info = c.result(raise_on_fail=False)
        assert _bits_equal(c.anc, anc[h::2]) and _bits_equal(wn, ref[0][h::2])
        assert _bits_equal(ll1, ref[1][h::2]) and _bits_equal(lld, ref[2][h::2])
    eng.close()


def test_chain_batch_device_ancestor_equals_host_pool():
    """ChainBatch with the device's ancestor_x (the default at S <= 64) and
    with the host's (InvPool workers), pipelined in two groups: the same
    proposals, scores, accepts, weights and ancestor_x, step for step."""
    m = generator.config_nem("C3")
    eng = Engine.for_nem(m)
    from nemo import utils
    order = utils.initial_order_guess(m.observed_knockdown_mat)
    res = []
    pool = InvPool(64, 8, n_workers=1)
    try:
        for pl in (None, pool):
            cb = ChainBatch(m, [order] * 8, seeds=list(range(40, 48)), engine=eng, on_fail="continue",
                            inv_pool=pl, groups=2)
            best, orders = cb.run(6)
            res.append((best, orders, cb.accepted, [c.parent_weights.copy() for c in cb.chains],
                        [c.ancestor_x.copy() for c in cb.chains],
                        [np.array(c.all_score_list) for c in cb.chains]))
    finally:
        pool.close()
    (b1, o1, a1, w1, x1, s1), (b2, o2, a2, w2, x2, s2) = res
    assert _bits_equal(b1, b2) and np.array_equal(o1, o2) and np.array_equal(a1, a2)
    for u, v in zip(w1 + x1 + s1, w2 + x2 + s2):
        assert _bits_equal(u, v)
    eng.close()


# --------------------------------------------------------------------------
# every S, across the weight space (tests/ancestor_inputs.py)
# --------------------------------------------------------------------------
def _diff(got, ref):
    """How two arrays differ: (values, of which only the sign of a zero)."""
    g, r = np.asarray(got).view(np.uint64), np.asarray(ref).view(np.uint64)
    bad = g != r
    zero = bad & (np.asarray(got) == 0) & (np.asarray(ref) == 0)
    return int(bad.sum()), int(zero.sum())


def _check_batch(s, cap, labels, classes, d01, danc, fl, failures):
    for k, ((fam, j), (cls, sig, anc)) in enumerate(zip(labels, classes)):
        where = (s, fam, cap, j)
        if cls == "a":
            if not fl[k] & 1:
                failures.append(where + (f"scipy raises LinAlgError, flag {fl[k]}",))
        elif cls == "c":
            if not (fl[k] & 4 and fl[k] & 3 == 0):
                failures.append(where + (f"non-finite inverse, flag {fl[k]}",))
        else:
            if fl[k] != 0:
                failures.append(where + (f"finite inverse, flag {fl[k]}",))
            if not _bits_equal(d01[k], sig):
                failures.append(where + ("W~: %d values differ (%d only in the sign of zero)" % _diff(d01[k], sig),))
            if not _bits_equal(danc[k], anc):
                failures.append(where + ("ancestor_x: %d values differ (%d only in the sign of zero)"
                                         % _diff(danc[k], anc),))


@pytest.mark.parametrize("s", ai.SIZES)
def test_ancestor_every_size_every_family(s):
    """One device call per (S, cap) on every chain of ancestor_inputs.batch:
    the classes share the batch, so a failing chain's neighbours are checked
    for the host's bits beside it.  Every failing (S, family, cap, chain) is
    collected before the assertion."""
    eng = Engine.for_nem(generator.synthetic_nem(s, 40, 0))
    failures = []
    for cap in ai.all_caps(s):
        pos, w, labels = ai.batch(s, cap)
        d01, danc, fl = _device(eng, pos.copy(), w.copy(), cap)
        _check_batch(s, cap, labels, ai.classified(_host, s, cap), d01, danc, fl, failures)
    eng.close()
    assert not failures, "\n".join(map(str, failures))


@pytest.mark.parametrize("s", [47, 64])
def test_ancestor_one_chain_and_more_blocks_than_cus(s):
    """The sat family's chains one at a time (a one-block grid) and 300 at once:
    each equals the same chain in its batch of eight, and the host's."""
    eng = Engine.for_nem(generator.synthetic_nem(s, 40, 0))
    pos, w = ai.family("sat", s, 0)
    sig, anc = _host(pos, w.copy(), 0)
    r01, ranc, rfl = _device(eng, pos, w, 0)
    assert np.array_equal(rfl, np.zeros(ai.CHAINS)) and _bits_equal(r01, sig) and _bits_equal(ranc, anc)
    for k in range(ai.CHAINS):
        d01, danc, fl = _device(eng, pos[k:k + 1], w[k:k + 1], 0)
        assert fl[0] == 0 and _bits_equal(d01[0], r01[k]) and _bits_equal(danc[0], ranc[k]), k
    idx = np.arange(300) % ai.CHAINS
    d01, danc, fl = _device(eng, pos[idx], w[idx], 0)
    assert np.array_equal(fl, np.zeros(300))
    bad = [k for k in range(300) if not (_bits_equal(d01[k], r01[idx[k]]) and _bits_equal(danc[k], ranc[idx[k]]))]
    assert not bad, bad
    eng.close()


@pytest.mark.parametrize("s,j", [(7, 0), (40, 1), (64, 2)])
def test_singular_chain_raises_scipys_error_through_the_engine(s, j):
    """A zero pivot in the first (S = 7), a middle (S = 40) and the last
    (S = 64) panel: LinAlgError, as scipy raises; the engine steps afterwards."""
    eng = Engine.for_nem(generator.synthetic_nem(s, 40, 0))
    pos, w = ai.singular(s)
    with pytest.raises(LinAlgError):
        _host(pos[j:j + 1], w[j:j + 1].copy())
    with pytest.raises(LinAlgError):
        eng.optimal_weights_w(pos[j:j + 1], w[j:j + 1], SIG0, SIG1)
    gpos, gw = ai.family("wide", s, 0)
    out = eng.optimal_weights_w(gpos[:1], gw[:1], SIG0, SIG1, raise_on_fail=False)
    sig, anc = _host(gpos[:1], gw[:1].copy())
    assert _bits_equal(out[0], sig) and _bits_equal(out[1], anc) and np.isfinite(out[3]).all()
    eng.close()


def _eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("s", [33, 64])
def test_non_finite_inverse_is_recomputed_from_the_hosts(s):
    """Flag 4 -> AncestorRecompute -> recompute(): one overflowing chain and
    three finite ones through optimal_weights_w and through
    chains.optimal_weights_batch give what the step from the host's W~ /
    ancestor_x gives, NaN for NaN.  (The overflowing chain's ancestor_x holds
    NaN: every local objective adds |expit(x) - ancestor_x|, so f and g are NaN
    at the first point and L-BFGS-B ends there -- DESIGN.md 3.8.)"""
    from nemo import chains
    m = generator.synthetic_nem(s, 40, 0)
    eng = Engine.for_nem(m)
    opos, ow = ai.overflow(s)
    gpos, gw = ai.family("wide", s, 0)
    pos = np.ascontiguousarray(np.concatenate([gpos[:1], opos, gpos[1:3]]))
    w = np.ascontiguousarray(np.concatenate([gw[:1], ow, gw[1:3]]))
    cls = ai.classify(_host, pos, w, 0)
    assert [c for c, _, _ in cls] == ["b", "c", "b", "b"]
    sig, anc = np.stack([c[1] for c in cls]), np.stack([c[2] for c in cls])
    assert np.isnan(anc[1]).any()
    _, _, fl = _device(eng, pos, w)
    assert fl.tolist() == [0, 4, 0, 0]
    ref = eng.optimal_weights(pos, sig, anc, w, SIG0, SIG1, raise_on_fail=False)
    got = eng.optimal_weights_w(pos, w, SIG0, SIG1, raise_on_fail=False)
    assert _eq(got[0], sig) and _eq(got[1], anc)
    for a, b in zip(got[2:], ref):
        assert _eq(a, b)
    # the finite chains: the host's bits
    for k in (0, 2, 3):
        assert _bits_equal(got[1][k], anc[k]) and _bits_equal(got[2][k], ref[0][k])
    cb = ChainBatch(m, [np.argsort(p) for p in pos], seeds=list(range(4)), engine=eng, on_fail="continue")
    for k, c in enumerate(cb.chains):
        assert np.array_equal(c._pos, pos[k])
        c.parent_weights = w[k].copy()
    lld = chains.optimal_weights_batch(cb.chains, eng, raise_on_fail=False)
    assert _eq(lld, ref[2])
    for k, c in enumerate(cb.chains):
        assert _eq(c.parent_weights, ref[0][k]) and _eq(c.ll, ref[1][k]) and _eq(c.ancestor_x, anc[k]), k
    # the engine still steps afterwards
    out = eng.optimal_weights_w(pos[:1], w[:1], SIG0, SIG1, raise_on_fail=False)
    assert _bits_equal(out[2], ref[0][:1])
    eng.close()
