"""nemo_score_relocations / nemo_score_relocations_dev (csrc/nemo_reloc.hip)
against the long-double reference of tests/reloc_ref.py (GPU).

Inputs: reloc_ref's lists -- S = 2 (one relocation per node), S = 15, 16, 17, 33,
60, 64, S = 17 at E = 1, 15, 16, 17, 63, 64, 65 (wave and word edges) and at E =
1040, four rungs of the error-rate ladder at S = 64, E = 40 (nem12: a log range
of 1 740), three table-built models and the mirrored deep table whose exponent
passes +709, each on auto and with option reloc_path 1 (one path today: the same
bits, reloc_path_used 1); nem04 at S = 128; every generic case of
score_grad_ref.GENERIC.  Full weight matrices: reloc_ref.full_weights.

Per case: |dll - ref| <= tol_aq (reloc_ref's tolerance, derived there;
tests/test_reloc_cpu.py holds numpy fp64 to a half of it), ll within
stream_models.tol_ll, exactly +0.0 at q = pos[a], adjacent transpositions agreeing
from both sides, the same bits with NaN on the diagonal of w01, for a batch of
one, for slots of a batch of 37, for a second run and for the device entry on a
side stream.  Each case prints its worst error over tolerance (pytest -s).

Observed worst error over tolerance on an MI355X: 0.032 (nem08-S64-E40), 0.008 on
the real-valued tables; gibbs_orders' worst z-score 0.89 (DESIGN.md 3.14,
MEASUREMENTS.md)."""
import numpy as np
import pytest

import fixed_point_models as fm
import reloc_ref as rr
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


def _dev(eng, pos, w):
    """nemo_score_relocations_dev on a side torch stream, outputs preset to NaN."""
    import torch
    b = pos.shape[0]
    eng.reserve(b)
    side = torch.cuda.Stream()
    dpos, dw = torch.from_numpy(pos).cuda(), torch.from_numpy(w).cuda()
    dll = torch.full((b,), float("nan"), dtype=torch.float64, device="cuda")
    dd = torch.full((b, eng.S, eng.S), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        eng.score_relocations_dev(b, dpos.data_ptr(), dw.data_ptr(), dll.data_ptr(), dd.data_ptr(),
                                  stream=side.cuda_stream)
    side.synchronize()
    return dll.cpu().numpy(), dd.cpu().numpy()


def _against_ref(tag, ll, d, refs, perms, factor=1.0):
    """-> worst err / tol; asserts the tolerance, finiteness, the exact zeros and the adjacent symmetry."""
    worst = 0.0
    for k, ref in enumerate(refs):
        s = len(perms[k])
        assert np.isfinite(d[k]).all() and np.isfinite(ll[k]), (tag, k)
        pos = np.argsort(perms[k])
        stay = d[k][np.arange(s), pos]
        assert (stay == 0.0).all() and not np.signbit(stay).any(), (tag, k, "exact +0.0")
        err = np.abs(d[k].astype(LD) - ref.dll).astype(np.float64)
        ok = ref.tol > 0.0
        assert ok.sum() == s * (s - 1)
        ratio = err[ok] / ref.tol[ok]
        worst = max(worst, float(ratio.max()))
        assert (err[ok] <= factor * ref.tol[ok]).all(), (tag, k, float(ratio.max()))
        assert abs(float(LD(ll[k]) - ref.cs.sum())) <= ref.tol_ll, (tag, k, "ll")
        a, n = perms[k][:-1], perms[k][1:]
        p = np.arange(s - 1)
        assert (np.abs(d[k][a, p + 1] - d[k][n, p]) <= ref.tol[a, p + 1] + ref.tol[n, p]).all(), (tag, k, "adjacent")
    return worst


def _bits(eng, path, tag, pos, w, ll, d):
    """NaN on the diagonal, batch of one, slots of a batch of 37, a second run, the device entry."""
    n = len(pos)
    wn = w.copy()
    wn[:, np.arange(eng.S), np.arange(eng.S)] = np.nan
    l2, d2 = eng.score_relocations(pos, wn)
    assert np.array_equal(l2, ll) and np.array_equal(d2, d), (tag, "NaN on the diagonal")
    for one in (0, n - 1):
        l1, d1 = eng.score_relocations(pos[one:one + 1], w[one:one + 1])
        assert l1[0] == ll[one] and np.array_equal(d1[0], d[one]), (tag, "batch of one", one)
    idx = (sm.tile_batch(n, 37) + 5) % n
    p37, w37 = (np.ascontiguousarray(x[idx]) for x in (pos, w))
    l37, d37 = eng.score_relocations(p37, w37)
    assert np.array_equal(l37, ll[idx]) and np.array_equal(d37, d[idx]), (tag, "batch of 37")
    l3, d3 = eng.score_relocations(p37, w37)
    assert np.array_equal(l3, l37) and np.array_equal(d3, d37), (tag, "second run")
    ld, dd = _dev(eng, p37, w37)
    assert np.array_equal(ld, l37) and np.array_equal(dd, d37), (tag, "device entry on a side stream")
    assert eng.get_option("reloc_path_used") == path, tag


@pytest.mark.parametrize("name", rr.factored_ids())
def test_factored_models(name):
    """Auto and option reloc_path 1: the two-pass path either way (reloc_path_used 1) and the same bits."""
    m, perms, pos, w = rr.factored_case(name)
    refs = rr.factored_refs(name)
    eng = _factored_engine(m)
    got = {}
    try:
        assert eng.get_option("reloc_path_used") == 0
        for option in (0, 1):
            eng.set_option("reloc_path", option)
            for cap in (0, m.S - 1, m.S + 5):             # a cap that cuts nothing: the same bits
                ll, d = eng.score_relocations(pos, w, cap=cap)
                assert eng.get_option("reloc_path_used") == 1, name
                if cap:
                    assert np.array_equal(ll, got[option][0]) and np.array_equal(d, got[option][1]), (name, cap)
                else:
                    got[option] = (ll, d)
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), (name, "option 0 and 1")
        ll, d = got[0]
        worst = _against_ref(name, ll, d, refs, perms)
        _bits(eng, 1, name, pos, w, ll, d)
    finally:
        eng.close()
    print(f"RELOC {name} worst err/tol: {worst:.4f}")


def test_factored_past_64():
    name = rr.WIDE_MODEL
    m, perms, pos, w = rr.factored_case(name)
    eng = _factored_engine(m)
    try:
        ll, d = eng.score_relocations(pos, w)
        assert eng.get_option("reloc_path_used") == 1
        worst = _against_ref(name, ll, d, rr.factored_refs(name), perms)
        _bits(eng, 1, name, pos, w, ll, d)
    finally:
        eng.close()
    print(f"RELOC {name} worst err/tol: two-pass {worst:.4f}")


@pytest.mark.parametrize("name", rr.GENERIC)
def test_generic_tables(name):
    c, _, _, perms, pos, w = rr.generic_case(name)
    eng = _generic_engine(c)
    try:
        ll, d = eng.score_relocations(pos, w)
        assert eng.get_option("reloc_path_used") == 1
        worst = _against_ref(name, ll, d, rr.generic_refs(name), perms)
        _bits(eng, 1, name, pos, w, ll, d)
    finally:
        eng.close()
    print(f"RELOC {name} worst err/tol: two-pass {worst:.4f}")


@pytest.mark.parametrize("name", rr.RESCORE)
def test_rescoring(name):
    """ll + dll[a][q] is nemo_score_grad's ll of the relocated order: every (a, q) of the model's
    evaluations 0, 1 and 5 (soft, saturated and coin-flip weights on random orders), within the two
    tol_ll plus the entry's tolerance; the relocated order's tol_ll comes from its own long-double
    reference."""
    m, perms, pos, w = rr.factored_case(name)
    refs = rr.factored_refs(name)
    et = np.exp(m.T.astype(LD))
    s = m.S
    eng = _factored_engine(m)
    try:
        ll, d = eng.score_relocations(pos, w)
        for k in (0, 1, 5):
            aq = [(a, q) for a in range(s) for q in range(s) if q != pos[k, a]]
            new = [rr.apply_relocation(perms[k], a, q) for a, q in aq]
            npos = np.stack([np.argsort(p) for p in new]).astype(np.int32)
            l2, _ = eng.score_grad(npos, np.ascontiguousarray(np.broadcast_to(w[k], (len(aq), s, s))))
            for t, (a, q) in enumerate(aq):
                _, cs2, cells2, _ = fm.reference(m.U, m.T, new[t], w[k], 0, full=True, et=et)
                tll2 = sm.tol_ll(cs2, sm.tol_cell(s - 1, float(np.abs(cells2).max())))
                bound = refs[k].tol_ll + tll2 + refs[k].tol[a, q]
                assert abs(l2[t] - (ll[k] + d[k, a, q])) <= bound, (name, k, a, q)
    finally:
        eng.close()


def test_entry_checks():
    import ctypes
    import torch
    m, perms, pos, w = rr.factored_case("small-S15-E16")
    lib = _lib.load()
    f32 = Engine(m.U, m.T, dtype="f32")
    try:
        with pytest.raises(RuntimeError, match="f32") as ei:
            f32.score_relocations(pos, w)
        assert ei.value.code == _lib.NEMO_ERR_ARG
    finally:
        f32.close()
    a = _lib.addr
    b = pos.shape[0]
    ll = np.full(b, 7.0)
    d = np.full((b, m.S, m.S), 7.0)
    ctx = ctypes.c_void_p()
    assert lib.nemo_ctx_create(0, m.S, m.E, _lib.NEMO_F64, ctypes.byref(ctx)) == _lib.NEMO_OK
    try:
        assert lib.nemo_score_relocations(ctx, b, a(pos), a(w), 0, a(ll), a(d)) == _lib.NEMO_ERR_STATE   # unstaged
        assert lib.nemo_score_relocations_dev(ctx, b, a(pos), a(w), 0, a(ll), a(d), None) == _lib.NEMO_ERR_STATE
    finally:
        lib.nemo_ctx_destroy(ctx)
    eng = _factored_engine(m)
    try:
        # the host entry: a cap that cuts, an off-diagonal weight outside [0, 1] or not finite, a bad permutation
        for cap in (1, 3, m.S - 2):
            assert lib.nemo_score_relocations(eng.handle, b, a(pos), a(w), cap, a(ll), a(d)) == _lib.NEMO_ERR_ARG, cap
            assert b"cap" in lib.nemo_last_error()
        assert lib.nemo_score_relocations(eng.handle, b, a(pos), a(w), -1, a(ll), a(d)) == _lib.NEMO_ERR_ARG
        i, j = perms[1][3], perms[1][9]          # j after i in the order: not a permissible pair, read all the same
        for bad in (np.nan, np.inf, -np.inf, -1e-9, 1.0 + 1e-9):
            for ii, jj in ((i, j), (j, i)):
                wb = w.copy()
                wb[1, ii, jj] = bad
                assert lib.nemo_score_relocations(eng.handle, b, a(pos), a(wb), 0, a(ll), a(d)) == _lib.NEMO_ERR_ARG
                assert b"w01[1]" in lib.nemo_last_error()
        p = pos.copy()
        p[2, 0] = p[2, 1]
        assert lib.nemo_score_relocations(eng.handle, b, a(p), a(w), 0, a(ll), a(d)) == _lib.NEMO_ERR_ARG
        assert lib.nemo_score_relocations(eng.handle, 0, None, None, 0, None, None) == _lib.NEMO_OK
        for k in range(4):
            args = [a(pos), a(w), 0, a(ll), a(d)]
            args[k if k < 2 else k + 1] = None
            assert lib.nemo_score_relocations(eng.handle, b, *args) == _lib.NEMO_ERR_ARG, k
        assert (ll == 7.0).all() and (d == 7.0).all()        # no refused call wrote anything
        # the device entry
        eng.reserve(b)
        dpos = torch.from_numpy(np.tile(pos, (2, 1))).cuda()
        dw = torch.from_numpy(np.tile(w, (2, 1, 1))).cuda()
        dll = torch.zeros(2 * b, dtype=torch.float64, device="cuda")
        dd = torch.zeros((2 * b, m.S, m.S), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        args = (dpos.data_ptr(), dw.data_ptr(), 0, dll.data_ptr(), dd.data_ptr(), None)
        assert lib.nemo_score_relocations_dev(eng.handle, 2 * b, *args) == _lib.NEMO_ERR_STATE
        assert b"reserved" in lib.nemo_last_error()
        for k in (0, 1, 3, 4):
            aa = list(args)
            aa[k] = None
            assert lib.nemo_score_relocations_dev(eng.handle, b, *aa) == _lib.NEMO_ERR_ARG, k
        for cap in (-1, 2, m.S - 2):
            aa = list(args)
            aa[2] = cap
            assert lib.nemo_score_relocations_dev(eng.handle, b, *aa) == _lib.NEMO_ERR_ARG
        assert lib.nemo_score_relocations_dev(eng.handle, 0, *args) == _lib.NEMO_OK
        with pytest.raises(_lib.NemoError):
            eng.set_option("reloc_path", 2)
        eng.set_option("timing_kernel", 4)
        eng.set_option("timing_kernel", 0)
        torch.cuda.synchronize()
        assert float(dd.abs().sum()) == 0.0 and float(dll.abs().sum()) == 0.0   # no refused call wrote anything
    finally:
        eng.close()


class _Recording:
    """An engine's score_relocations with the pos of every call kept."""

    def __init__(self, eng):
        self.eng, self.calls = eng, []

    def score_relocations(self, pos, w01, cap=0):
        self.calls.append(np.array(pos))
        return self.eng.score_relocations(pos, w01, cap=cap)


def test_greedy_relocations():
    from nemo.methods import greedy_relocations
    m, pos, w = rr.greedy_inputs()
    cpu = rr.NumpyEngine(m.U, m.T)
    want_trace = []
    want_pos, _, want_n = greedy_relocations(cpu, pos, w, ll_trace=want_trace)
    eng = _factored_engine(m)
    try:
        rec = _Recording(eng)
        trace = []
        got_pos, ll, n = greedy_relocations(rec, pos, w, ll_trace=trace)
        assert eng.get_option("reloc_path_used") == 1
    finally:
        eng.close()
    # the CPU hill-climb's steps, order by order (its margins: tests/test_reloc_cpu.py)
    assert rr.moves_of(rec.calls) == rr.moves_of(cpu.calls)
    assert np.array_equal(got_pos, want_pos) and np.array_equal(n, want_n)
    et = np.exp(m.T.astype(LD))
    lls, want = np.stack(trace), np.stack(want_trace)
    assert lls.shape == want.shape
    for k in range(len(pos)):
        ref = rr.reloc_reference(m.U, m.T, np.argsort(got_pos[k]), w[k], et=et)
        stay = ref.tol == 0.0
        assert (ref.dll[~stay] <= 1e-9 + ref.tol[~stay]).all(), (k, "a single relocation still gains")
        assert abs(float(LD(ll[k]) - ref.cs.sum())) <= ref.tol_ll, k
        assert (np.abs(lls[:, k] - want[:, k]) <= 2.0 * ref.tol_ll + 1e-9 * np.abs(want[:, k])).all(), (k, "ll trace")
        assert (np.diff(lls[:, k]) >= -2.0 * ref.tol_ll).all(), (k, "ll fell")


def test_gibbs_orders():
    """The S = 4 model of tests/test_reloc_cpu.py on the device: the same seed gives the numpy engine's
    chains (the draws depend on dll through a CDF, so the orders agree unless a uniform falls within
    rounding of a CDF step), and the marginals are within 3 standard errors of the enumeration."""
    from nemo.methods import gibbs_orders
    u, t, w = rr.gibbs_model()
    exact = rr.gibbs_enumeration()
    b = rr.GIBBS_CHAINS
    rng = np.random.default_rng(rr.GIBBS_SEED)
    pos = np.stack([np.argsort(rng.permutation(4)) for _ in range(b)]).astype(np.int32)
    wb = np.ascontiguousarray(np.broadcast_to(w, (b, 4, 4)))
    eng = Engine(u, t)
    try:
        out_pos, lls, before = gibbs_orders(eng, pos, wb, rr.GIBBS_SWEEPS, burn_in=rr.GIBBS_BURN, rng=rr.GIBBS_SEED)
        ll_end, _ = eng.score_relocations(out_pos, wb)
    finally:
        eng.close()
    assert np.isfinite(lls).all() and lls.shape == (rr.GIBBS_SWEEPS * 4, b)
    assert np.abs(lls[-1] - ll_end).max() <= 1e-9              # the recorded score is the held order's
    z = rr.gibbs_z(before, exact)
    print(f"RELOC gibbs_orders (device): worst z-score {z:.2f}")
    assert z <= 3.0, z
