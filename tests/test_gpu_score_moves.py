"""nemo_score_moves / nemo_score_moves_dev (csrc/nemo_moves.hip) against the
long-double reference of tests/moves_ref.py (GPU).

Inputs: score_grad_ref's own lists -- seeded two-valued tables at S = 2, 15, 17
x E = 1, 15, 16, 17, 63, 64, 65 (row-block, tile and word edges) and at E =
1040 (two parts of the fused kernel's cut of E), the error-rate ladder at S =
16, 33, 60, 64 x E = 40, 130 and three table-built models (every pair slot of
SPAD = 64 is met) under the fused kernel and, with option moves_path 1, the
two-pass path; nem04 at S = 128 on the two-pass path by itself; stream_models'
real-valued tables, generic and row-shared, one of them wide.  w_alt per
evaluation: moves_ref.alt_weights (uniform, 0, 1, the flip of the rounded w01,
and w01 itself, which must score exactly 0).

Per case and cap: |dll - ref| <= tol_ij (moves_ref's tolerance, derived there;
tests/test_moves_cpu.py holds numpy fp64 to a half of it), ll within
stream_models.tol_ll, exactly +0.0 off the permissible set and where w_alt ==
w01, the same bits with NaN at every entry of w01 and w_alt that is not
permissible, for a batch of one, for slots of a batch of 37, for a second run
and for the device entry on a side stream, and fused against two-pass within
2 tol_ij.  Each case prints its worst error over tolerance (pytest -s)."""
import numpy as np
import pytest

import moves_ref as mr
import score_grad_ref as gr
import stream_models as sm
from nemo import _lib
from nemo.engine import Engine

pytestmark = pytest.mark.gpu

LD = np.longdouble


def _factored_engine(m):
    if m.nem is not None:
        eng = Engine.from_knockdown(m.nem.observed_knockdown_mat, m.nem.A, m.nem.B)
    else:
        eng = Engine(m.U, m.T)
    assert eng.factored
    return eng


def _generic_engine(c):
    u, t = sm.tables(c.name)
    eng = Engine(u, t, dtype=c.dtype, exact_generic=c.generic)
    assert not eng.factored
    return eng


def _poisoned(w, perms, cap):
    """w with NaN at every entry that is not a permissible pair."""
    w = w.copy()
    for k, perm in enumerate(perms):
        w[k][~mr.permissible(perm, cap)] = np.nan
    return w


def _dev(eng, pos, w, wa, cap):
    """nemo_score_moves_dev on a side torch stream, outputs preset to NaN."""
    import torch
    b = pos.shape[0]
    eng.reserve(b)
    side = torch.cuda.Stream()
    dpos, dw, dwa = torch.from_numpy(pos).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(wa).cuda()
    dll = torch.full((b,), float("nan"), dtype=torch.float64, device="cuda")
    dd = torch.full((b, eng.S, eng.S), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        eng.score_moves_dev(b, dpos.data_ptr(), dw.data_ptr(), dwa.data_ptr(), dll.data_ptr(), dd.data_ptr(), cap=cap,
                            stream=side.cuda_stream)
    side.synchronize()
    return dll.cpu().numpy(), dd.cpu().numpy()


def _against_ref(tag, ll, d, refs, perms, w01, wa, cap, factor=1.0):
    """-> worst err / tol; asserts the tolerance, finiteness and the exact zeros."""
    worst = 0.0
    for k, ref in enumerate(refs):
        ok = mr.permissible(perms[k], cap)
        assert np.isfinite(d[k]).all() and np.isfinite(ll[k]), (tag, cap, k)
        zero = ~ok | (wa[k] == w01[k])
        assert (d[k][zero] == 0.0).all() and not np.signbit(d[k][zero]).any(), (tag, cap, k, "exact +0.0")
        err = np.abs(d[k].astype(LD) - ref.dll).astype(np.float64)
        ok &= ref.tol > 0.0
        if ok.any():
            ratio = err[ok] / ref.tol[ok]
            worst = max(worst, float(ratio.max()))
            assert (err[ok] <= factor * ref.tol[ok]).all(), (tag, cap, k, float(ratio.max()))
        assert abs(float(LD(ll[k]) - ref.cs.sum())) <= ref.tol_ll, (tag, cap, k, "ll")
    return worst


def _bits(eng, path, tag, pos, w01, wa, perms, cap, ll, d):
    """NaN off the permissible set, batch of one, slots of a batch of 37, a second run, the device entry."""
    n = len(perms)
    l2, d2 = eng.score_moves(pos, _poisoned(w01, perms, cap), _poisoned(wa, perms, cap), cap=cap)
    assert np.array_equal(l2, ll) and np.array_equal(d2, d), (tag, cap, "NaN off the permissible set")
    for one in (0, n - 1):
        l1, d1 = eng.score_moves(pos[one:one + 1], w01[one:one + 1], wa[one:one + 1], cap=cap)
        assert l1[0] == ll[one] and np.array_equal(d1[0], d[one]), (tag, cap, "batch of one", one)
    idx = (sm.tile_batch(n, 37) + 5) % n
    p37, w37, a37 = (np.ascontiguousarray(x[idx]) for x in (pos, w01, wa))
    l37, d37 = eng.score_moves(p37, w37, a37, cap=cap)
    assert np.array_equal(l37, ll[idx]) and np.array_equal(d37, d[idx]), (tag, cap, "batch of 37")
    l3, d3 = eng.score_moves(p37, w37, a37, cap=cap)
    assert np.array_equal(l3, l37) and np.array_equal(d3, d37), (tag, cap, "second run")
    ld, dd = _dev(eng, p37, w37, a37, cap)
    assert np.array_equal(ld, l37) and np.array_equal(dd, d37), (tag, cap, "device entry on a side stream")
    assert eng.get_option("moves_path_used") == path, (tag, cap)


@pytest.mark.parametrize("name", mr.factored_ids())
def test_factored_fused_and_two_pass(name):
    m, perms, pos, w01 = mr.factored_inputs(name)
    wa = mr.factored_alt(name)
    eng = _factored_engine(m)
    worst = {1: 0.0, 2: 0.0}
    try:
        assert eng.get_option("moves_path_used") == 0
        for cap in mr.factored_caps(m.S):
            refs = mr.factored_refs(name, cap)
            got = {}
            for path, option in ((2, 0), (1, 1)):
                eng.set_option("moves_path", option)
                ll, d = eng.score_moves(pos, w01, wa, cap=cap)
                assert eng.get_option("moves_path_used") == path, (name, cap)
                worst[path] = max(worst[path], _against_ref(f"{name} path {path}", ll, d, refs, perms, w01, wa, cap))
                _bits(eng, path, f"{name} path {path}", pos, w01, wa, perms, cap, ll, d)
                got[path] = d
            for k, ref in enumerate(refs):
                assert (np.abs(got[2][k] - got[1][k]) <= 2.0 * ref.tol).all(), (name, cap, k, "fused against two-pass")
    finally:
        eng.close()
    print(f"MOVES {name} worst err/tol: fused {worst[2]:.3f} two-pass {worst[1]:.3f}")


def test_factored_past_64_takes_the_two_pass_path():
    name = mr.WIDE_MODEL
    m, perms, pos, w01 = mr.factored_inputs(name)
    wa = mr.factored_alt(name)
    eng = _factored_engine(m)
    worst = 0.0
    try:
        for cap in mr.factored_caps(m.S):
            ll, d = eng.score_moves(pos, w01, wa, cap=cap)
            assert eng.get_option("moves_path_used") == 1
            worst = max(worst, _against_ref(name, ll, d, mr.factored_refs(name, cap), perms, w01, wa, cap))
            _bits(eng, 1, name, pos, w01, wa, perms, cap, ll, d)
    finally:
        eng.close()
    print(f"MOVES {name} worst err/tol: two-pass {worst:.3f}")


@pytest.mark.parametrize("name", mr.GENERIC)
def test_generic_tables(name):
    c, _, _, perms, pos, w01 = mr.generic_inputs(name)
    wa = mr.generic_alt(name)
    eng = _generic_engine(c)
    worst = 0.0
    try:
        for cap in mr.generic_caps(c.s):
            ll, d = eng.score_moves(pos, w01, wa, cap=cap)
            assert eng.get_option("moves_path_used") == 1
            worst = max(worst, _against_ref(name, ll, d, mr.generic_refs(name, cap), perms, w01, wa, cap))
            _bits(eng, 1, name, pos, w01, wa, perms, cap, ll, d)
    finally:
        eng.close()
    print(f"MOVES {name} worst err/tol: two-pass {worst:.3f}")


@pytest.mark.parametrize("name", ["nem04-S33-E130", "small-S17-E1040"])
def test_consistent_with_the_gradient(name):
    """A short step along one weight, w_alt = w01 + h (0.5 - w01) with h = 2^-20: dll / (w_alt - w01) is
    nemo_score_grad's entry within twice score_grad_ref's tolerance plus the second-order term, taken in
    long double as the difference between the reference's dll / step and the reference's gradient."""
    m, perms, pos, w01 = mr.factored_inputs(name)
    h = 2.0 ** -20
    wa = w01 + h * (0.5 - w01)
    et = np.exp(m.T.astype(LD))
    eng = _factored_engine(m)
    try:
        for option in (0, 1):
            eng.set_option("moves_path", option)
            ll, d = eng.score_moves(pos, w01, wa)
            lg, g = eng.score_grad(pos, w01)
            for k, perm in enumerate(perms):
                step = wa[k] - w01[k]
                ok = mr.permissible(perm) & (step != 0.0)
                mref = mr.moves_reference(m.U, m.T, perm, w01[k], wa[k], et=et)
                gref = gr.factored_refs(name, 0)[k]
                second = np.abs(mref.dll[ok] / step[ok].astype(LD) - gref.g[ok]).astype(np.float64)
                bound = 2.0 * gref.tol[ok] + second
                assert (np.abs(d[k][ok] / step[ok] - g[k][ok]) <= bound).all(), (name, option, k)
                assert abs(ll[k] - lg[k]) <= 2.0 * mref.tol_ll
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["nem08-S16-E40", "small-S17-E65"])
def test_consistent_across_a_move(name):
    """After one move is applied, the next call's ll is the previous ll + dll."""
    m, perms, pos, w01 = mr.factored_inputs(name)
    wa = mr.factored_alt(name)
    eng = _factored_engine(m)
    try:
        for option in (0, 1):
            eng.set_option("moves_path", option)
            ll, d = eng.score_moves(pos, w01, wa)
            refs = mr.factored_refs(name, 0)
            w2 = w01.copy()
            picks = []
            for k, perm in enumerate(perms):
                ij = np.argwhere(mr.permissible(perm))
                i, j = ij[(7 * k + 3) % len(ij)]
                w2[k, i, j] = wa[k, i, j]
                picks.append((i, j))
            ll2, _ = eng.score_moves(pos, w2, wa)
            for k, (i, j) in enumerate(picks):
                assert abs(ll2[k] - (ll[k] + d[k, i, j])) <= refs[k].tol_ll + refs[k].tol[i, j], (name, option, k)
    finally:
        eng.close()


def test_entry_checks():
    import torch
    m, perms, pos, w01 = mr.factored_inputs("small-S15-E17")
    wa = mr.factored_alt("small-S15-E17")
    lib = _lib.load()
    f32 = Engine(m.U, m.T, dtype="f32")
    try:
        with pytest.raises(RuntimeError, match="f32") as ei:
            f32.score_moves(pos, w01, wa)
        assert ei.value.code == _lib.NEMO_ERR_ARG
    finally:
        f32.close()
    eng = _factored_engine(m)
    try:
        b = pos.shape[0]
        # the host entry: w_alt outside [0, 1] or not finite at a permissible pair, a bad permutation, a negative cap
        ll = np.full(b, 7.0)
        d = np.full((b, m.S, m.S), 7.0)
        a = _lib.addr
        i, j = np.argwhere(mr.permissible(perms[1]))[4]
        for bad in (np.nan, np.inf, -np.inf, -1e-9, 1.0 + 1e-9):
            w = wa.copy()
            w[1, i, j] = bad
            assert lib.nemo_score_moves(eng.handle, b, a(pos), a(w01), a(w), 0, a(ll), a(d)) == _lib.NEMO_ERR_ARG, bad
            assert b"w_alt[1]" in lib.nemo_last_error()
        w = wa.copy()
        w[1, j, i] = np.nan      # not permissible: not looked at
        p1, w1, a1 = (np.ascontiguousarray(x[1:2]) for x in (pos, w01, w))
        l1, d1 = np.empty(1), np.empty((1, m.S, m.S))
        assert lib.nemo_score_moves(eng.handle, 1, a(p1), a(w1), a(a1), 0, a(l1), a(d1)) == _lib.NEMO_OK
        assert np.isfinite(l1).all() and np.isfinite(d1).all()
        p = pos.copy()
        p[2, 0] = p[2, 1]
        assert lib.nemo_score_moves(eng.handle, b, a(p), a(w01), a(wa), 0, a(ll), a(d)) == _lib.NEMO_ERR_ARG
        assert lib.nemo_score_moves(eng.handle, b, a(pos), a(w01), a(wa), -1, a(ll), a(d)) == _lib.NEMO_ERR_ARG
        assert lib.nemo_score_moves(eng.handle, 0, None, None, None, 0, None, None) == _lib.NEMO_OK
        assert lib.nemo_score_moves(eng.handle, 1, None, None, None, 0, None, None) == _lib.NEMO_ERR_ARG
        for k in range(5):
            args = [a(pos), a(w01), a(wa), 0, a(ll), a(d)]
            args[k if k < 3 else k + 1] = None
            assert lib.nemo_score_moves(eng.handle, b, *args) == _lib.NEMO_ERR_ARG, k
        assert (ll == 7.0).all() and (d == 7.0).all()        # no refused call wrote anything
        # the device entry
        eng.reserve(b)
        dpos = torch.from_numpy(np.tile(pos, (2, 1))).cuda()
        dw, dwa = torch.from_numpy(np.tile(w01, (2, 1, 1))).cuda(), torch.from_numpy(np.tile(wa, (2, 1, 1))).cuda()
        dll = torch.zeros(2 * b, dtype=torch.float64, device="cuda")
        dd = torch.zeros((2 * b, m.S, m.S), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        args = (dpos.data_ptr(), dw.data_ptr(), dwa.data_ptr(), 0, dll.data_ptr(), dd.data_ptr(), None)
        assert lib.nemo_score_moves_dev(eng.handle, 2 * b, *args) == _lib.NEMO_ERR_STATE
        assert b"reserved" in lib.nemo_last_error()
        for k in (0, 1, 2, 4, 5):
            aa = list(args)
            aa[k] = None
            assert lib.nemo_score_moves_dev(eng.handle, b, *aa) == _lib.NEMO_ERR_ARG, k
        aa = list(args)
        aa[3] = -1
        assert lib.nemo_score_moves_dev(eng.handle, b, *aa) == _lib.NEMO_ERR_ARG
        assert lib.nemo_score_moves_dev(eng.handle, 0, *args) == _lib.NEMO_OK
        with pytest.raises(_lib.NemoError):
            eng.set_option("moves_path", 2)
        eng.set_option("timing_kernel", 3)
        eng.set_option("timing_kernel", 0)
        torch.cuda.synchronize()
        assert float(dd.abs().sum()) == 0.0 and float(dll.abs().sum()) == 0.0   # no refused call wrote anything
    finally:
        eng.close()


class _Recording:
    """An engine's score_moves with the w01 of every call kept."""

    def __init__(self, eng):
        self.eng, self.calls = eng, []

    def score_moves(self, pos, w01, w_alt, cap=0):
        self.calls.append(np.array(w01))
        return self.eng.score_moves(pos, w01, w_alt, cap=cap)


@pytest.mark.parametrize("start", ["zero", "rounded"])
def test_greedy_flips(start):
    from nemo.methods import greedy_flips
    m, pos, w0 = mr.greedy_inputs(start)
    min_gain = 1e-9
    _, want_flips, _ = mr.numpy_greedy(mr.NumpyEngine(m.U, m.T), pos, w0, min_gain=min_gain)
    eng = _factored_engine(m)
    try:
        rec = _Recording(eng)
        trace = []
        w, ll, n = greedy_flips(rec, pos, w0, min_gain=min_gain, ll_trace=trace)
        assert eng.get_option("moves_path_used") == 2
    finally:
        eng.close()
    assert mr.flips_of(rec.calls) == want_flips          # the CPU greedy's steps (its margins: tests/test_moves_cpu.py)
    assert list(n) == [len(f) for f in want_flips]
    et = np.exp(m.T.astype(LD))
    lls = np.stack(trace)
    for k in range(len(pos)):
        perm = np.argsort(pos[k])
        ref = mr.moves_reference(m.U, m.T, perm, w[k], 1.0 - w[k], et=et)
        ok = mr.permissible(perm)
        assert (ref.dll[ok] <= min_gain + ref.tol[ok]).all(), (start, k, "a single flip still gains")
        assert abs(float(LD(ll[k]) - ref.cs.sum())) <= ref.tol_ll, (start, k)
        assert (np.diff(lls[:, k]) >= -2.0 * ref.tol_ll).all(), (start, k, "ll fell")


def test_greedy_method():
    from nemo.methods import GreedyMethod
    m, pos, w0 = mr.greedy_inputs("rounded")
    order = np.argsort(pos[0])
    _, want_flips, _ = mr.numpy_greedy(mr.NumpyEngine(m.U, m.T), pos[:1], np.zeros((1, m.S, m.S)))
    gm = GreedyMethod(order, m.S, m.E, m.U, m.T)
    try:
        dag_t, ll = gm.optimize()
        assert gm.n_flips == len(want_flips[0]) and len(gm.ll_list) == gm.n_flips + 1
        assert (np.diff(gm.ll_list) >= 0.0).all() and gm.ll_list[-1] == ll
        want = np.zeros((m.S, m.S))
        for i, j in want_flips[0]:
            want[i, j] = 1.0 - want[i, j]
        assert np.array_equal(dag_t.T, want)
        assert abs(ll - gm._ll_of(dag_t.T)) <= 1e-8          # the engine's own (int8) score of the same DAG
        dag2, ll2 = gm.optimize(start=w0[0], max_iter=3)
        assert gm.n_flips == 3 and len(gm.ll_list) == 4 and ll2 == gm.ll_list[-1]
    finally:
        gm.engine.close()
