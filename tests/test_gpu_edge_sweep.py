"""nemo_edge_sweep / nemo_edge_sweep_dev (csrc/nemo_sweep.hip) against the
long-double reference of tests/sweep_ref.py (GPU).

Cases (sweep_ref's lists): seeded two-valued tables at S = 2, 15, 17 x E = 1,
15, 16, 17, 63, 64, 65 (a single pair; fewer effects than threads; wave and
word edges, one wave at 1 and 2 effects per thread), E = 129 (4 per thread),
257, 513, 1025, 1040, 2049 (every block-size switch), 4097 and 8193 (8 and 16
effects per thread: the instances that keep no t_e), the error-rate ladder at S = 16, 33, 60, 64, two table-built models,
nem04 at S = 128, and stream_models' real-valued tables, generic and
row-shared; every cap of factored_caps / generic_caps.  Thresholds logit(u) per
evaluation.  tests/test_sweep_cpu.py asserts that every visit of these clears
its threshold by more than twice its tolerance, so a device within tolerance
takes the reference's decisions: w_out, alt_out and nacc are compared exactly,
gains and scores within sweep_ref's derived tolerances.  Models with no such
margin (saturated children against a wide table) run under forced decisions,
thr = +-inf, and in the same-bits checks.  Each case prints its worst error over
tolerance (pytest -s)."""
import numpy as np
import pytest

import moves_ref as mr
import stream_models as sm
import sweep_ref as sr
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


def _bits_equal(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
               for x, y in zip(a, b))


def _poisoned(w, perms, cap):
    w = w.copy()
    for k, perm in enumerate(perms):
        w[k][~mr.permissible(perm, cap)] = np.nan
    return w


def _dev(eng, pos, w, wa, thr, cap, inplace=False, optional=True):
    """nemo_edge_sweep_dev on a side torch stream, outputs preset to NaN -> the host entry's tuple."""
    import torch
    b = pos.shape[0]
    eng.reserve(b)
    side = torch.cuda.Stream()
    dpos, dw, dwa, dthr = (torch.from_numpy(x).cuda() for x in (pos, w, wa, thr))
    nan = float("nan")
    dwo = dw if inplace else torch.full_like(dw, nan)
    dao = dwa if inplace else torch.full_like(dwa, nan)
    dll0 = torch.full((b,), nan, dtype=torch.float64, device="cuda")
    dll = torch.full((b,), nan, dtype=torch.float64, device="cuda")
    dg = torch.full((b, eng.S, eng.S), nan, dtype=torch.float64, device="cuda")
    dn = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        eng.edge_sweep_dev(b, dpos.data_ptr(), dw.data_ptr(), dwa.data_ptr(), dthr.data_ptr(), dwo.data_ptr(),
                           dao.data_ptr(), dll.data_ptr(), d_ll0=dll0.data_ptr() if optional else None,
                           d_gain=dg.data_ptr() if optional else None, d_nacc=dn.data_ptr() if optional else None,
                           cap=cap, stream=side.cuda_stream)
    side.synchronize()
    return tuple(x.cpu().numpy() for x in (dwo, dao, dll0, dll, dg, dn))


def _against_ref(tag, got, refs, perms, w01, wa, cap):
    """-> worst err / tol; the decisions exactly, gains and scores within tolerance, the exact zeros."""
    w_out, alt_out, ll0, ll, gain, nacc = got
    worst = 0.0
    for k, ref in enumerate(refs):
        ok = mr.permissible(perms[k], cap)
        assert np.array_equal(w_out[k], ref.w_out) and np.array_equal(alt_out[k], ref.alt_out), (tag, cap, k)
        assert nacc[k] == ref.nacc, (tag, cap, k)
        zero = ~ok | (wa[k] == w01[k])
        assert (gain[k][zero] == 0.0).all() and not np.signbit(gain[k][zero]).any(), (tag, cap, k, "exact +0.0")
        err = np.abs(gain[k].astype(LD) - ref.gain).astype(np.float64)
        ok &= ref.tol > 0.0
        if ok.any():
            ratio = err[ok] / ref.tol[ok]
            worst = max(worst, float(ratio.max()))
            assert (err[ok] <= ref.tol[ok]).all(), (tag, cap, k, float(ratio.max()))
        e0, e1 = abs(float(LD(ll0[k]) - ref.cs0.sum())), abs(float(LD(ll[k]) - ref.cs.sum()))
        worst = max(worst, e0 / ref.tol_ll0, e1 / ref.tol_ll)
        assert e0 <= ref.tol_ll0 and e1 <= ref.tol_ll, (tag, cap, k, "ll", e0, e1)
    return worst


def _bits(eng, tag, pos, w01, wa, thr, perms, cap, got):
    """NaN off the permissible set, a batch of one, slots of a batch of 37, a second run, in place, the device entry."""
    n = len(perms)
    p2 = eng.edge_sweep(pos, _poisoned(w01, perms, cap), _poisoned(wa, perms, cap), _poisoned(thr, perms, cap), cap=cap)
    assert _bits_equal(p2[2:], got[2:]), (tag, cap, "NaN off the permissible set")
    for k, perm in enumerate(perms):
        ok = mr.permissible(perm, cap)
        assert np.array_equal(p2[0][k][ok], got[0][k][ok]) and np.array_equal(p2[1][k][ok], got[1][k][ok])
        assert np.isnan(p2[0][k][~ok]).all() and np.isnan(p2[1][k][~ok]).all()      # carried through
    for one in (0, n - 1):
        g1 = eng.edge_sweep(pos[one:one + 1], w01[one:one + 1], wa[one:one + 1], thr[one:one + 1], cap=cap)
        assert _bits_equal(g1, [x[one:one + 1] for x in got]), (tag, cap, "batch of one", one)
    idx = (sm.tile_batch(n, 37) + 5) % n
    a37 = [np.ascontiguousarray(x[idx]) for x in (pos, w01, wa, thr)]
    g37 = eng.edge_sweep(*a37, cap=cap)
    assert _bits_equal(g37, [x[idx] for x in got]), (tag, cap, "batch of 37")
    assert _bits_equal(eng.edge_sweep(*a37, cap=cap), g37), (tag, cap, "second run")
    assert _bits_equal(_dev(eng, *a37, cap), g37), (tag, cap, "device entry on a side stream")
    assert _bits_equal(_dev(eng, *a37, cap, inplace=True), g37), (tag, cap, "in place")
    bare = _dev(eng, *a37, cap, optional=False)
    assert _bits_equal((bare[0], bare[1], bare[3]), (g37[0], g37[1], g37[3])), (tag, cap, "optional outputs null")


def _forced(eng, tag, pos, w01, wa, perms, cap, refs_inf=None):
    """thr = +inf: nothing moves, ll == ll0 bit for bit.  thr = -inf: every move is taken."""
    n, s = len(perms), eng.S
    okb = np.stack([mr.permissible(p, cap) for p in perms])
    got = eng.edge_sweep(pos, w01, wa, np.full((n, s, s), np.inf), cap=cap)
    assert _bits_equal(got[:2], (w01, wa)) and (got[5] == 0).all(), (tag, cap, "+inf")
    assert _bits_equal([got[2]], [got[3]]), (tag, cap, "+inf: ll is ll0")
    got = eng.edge_sweep(pos, w01, wa, np.full((n, s, s), -np.inf), cap=cap)
    assert np.array_equal(got[0][okb], wa[okb]) and np.array_equal(got[1][okb], w01[okb]), (tag, cap, "-inf")
    assert _bits_equal((got[0][~okb], got[1][~okb]), (w01[~okb], wa[~okb]))
    assert np.array_equal(got[5], okb.sum(axis=(1, 2))) and np.isfinite(got[3]).all() and np.isfinite(got[4]).all()
    swept = np.where(okb, wa, w01)
    fresh, _ = eng.score_moves(pos, swept, swept, cap=cap)
    if refs_inf is not None:
        for k, ref in enumerate(refs_inf):
            assert abs(got[3][k] - fresh[k]) <= 2.0 * ref.tol_ll, (tag, cap, k, "-inf against a fresh score")
    return got


# ---- against the reference -----------------------------------------------------------------
@pytest.mark.parametrize("name", sr.DECISION_FACTORED)
def test_factored_against_reference(name):
    m, perms, pos, w01, wa, thr = sr.factored_case(name)
    eng = _factored_engine(m)
    worst = 0.0
    try:
        for cap in sr.factored_caps(m.S):
            got = eng.edge_sweep(pos, w01, wa, thr, cap=cap)
            worst = max(worst, _against_ref(name, got, sr.factored_refs(name, cap), perms, w01, wa, cap))
            _bits(eng, name, pos, w01, wa, thr, perms, cap, got)
    finally:
        eng.close()
    print(f"SWEEP {name} worst err/tol: {worst:.3f}")


@pytest.mark.parametrize("name", sr.GENERIC)
def test_generic_against_reference(name):
    c, _, _, perms, pos, w01, wa, thr = sr.generic_case(name)
    eng = _generic_engine(c)
    worst = 0.0
    try:
        for cap in sr.generic_caps(c.s):
            got = eng.edge_sweep(pos, w01, wa, thr, cap=cap)
            worst = max(worst, _against_ref(name, got, sr.generic_refs(name, cap), perms, w01, wa, cap))
            _bits(eng, name, pos, w01, wa, thr, perms, cap, got)
    finally:
        eng.close()
    print(f"SWEEP {name} worst err/tol: {worst:.3f}")


# ---- forced decisions ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sr.FORCED_FACTORED + ("small-S2-E1", "small-S17-E65", "small-S5-E1025",
                                                       "small-S2-E8193", "nem04-S33-E40"))
def test_forced_decisions_factored(name):
    m, perms, pos, w01, wa, thr = sr.factored_case(name)
    et = np.exp(m.T.astype(LD))
    eng = _factored_engine(m)
    try:
        for cap in sr.factored_caps(m.S):
            refs = None
            if name not in sr.FORCED_FACTORED:      # (there the summed tolerance is astronomically wide)
                refs = [sr.sweep_reference(m.U, m.T, p, w, a, np.full((m.S, m.S), -np.inf), cap, et=et)
                        for p, w, a in zip(perms, w01, wa)]
            _forced(eng, name, pos, w01, wa, perms, cap, refs)
            if name in sr.FORCED_FACTORED:
                _bits(eng, name, pos, w01, wa, thr, perms, cap, eng.edge_sweep(pos, w01, wa, thr, cap=cap))
    finally:
        eng.close()


@pytest.mark.parametrize("name", sr.FORCED_GENERIC + ("f64-own-S18-E130-a3",))
def test_forced_decisions_generic(name):
    c, u, t, perms, pos, w01, wa, thr = sr.generic_case(name)
    eng = _generic_engine(c)
    try:
        for cap in sr.generic_caps(c.s):
            refs = None
            if name not in sr.FORCED_GENERIC:
                et = sm._exp_table(name)
                refs = [sr.sweep_reference(u, t, p, w, a, np.full((c.s, c.s), -np.inf), cap, et=et)
                        for p, w, a in zip(perms, w01, wa)]
            _forced(eng, name, pos, w01, wa, perms, cap, refs)
            if name in sr.FORCED_GENERIC:
                _bits(eng, name, pos, w01, wa, thr, perms, cap, eng.edge_sweep(pos, w01, wa, thr, cap=cap))
    finally:
        eng.close()


# ---- round trip and consistency with nemo_score_moves ----------------------------------------------
@pytest.mark.parametrize("name", ["nem08-S16-E40", "small-S17-E65"])
def test_round_trip(name):
    """A sweep, then the reverse of every taken move with thr = -inf (+inf elsewhere):
    the starting weights return exactly and ll returns to ll0 within tolerance."""
    m, perms, pos, w01, wa, thr = sr.factored_case(name)
    et = np.exp(m.T.astype(LD))
    eng = _factored_engine(m)
    try:
        w1, a1, ll0, ll1, _, nacc = eng.edge_sweep(pos, w01, wa, thr)
        refs = sr.factored_refs(name, 0)
        back = np.where(np.stack([r.acc for r in refs]), -np.inf, np.inf)
        w2, a2, ll1b, ll2, _, nacc2 = eng.edge_sweep(pos, w1, a1, back)
        assert _bits_equal((w2, a2), (w01, wa)) and np.array_equal(nacc2, nacc)
        for k, ref in enumerate(refs):
            ref2 = sr.sweep_reference(m.U, m.T, perms[k], w1[k], a1[k], back[k], et=et)
            assert abs(ll1b[k] - ll1[k]) <= ref.tol_ll + ref2.tol_ll0, (name, k)
            assert abs(ll2[k] - ll0[k]) <= ref2.tol_ll + ref.tol_ll0, (name, k)
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["nem04-S16-E40", "small-S17-E1040", "small-S15-E17"])
def test_first_visit_is_the_move_score(name):
    """The first visited pair is scored at the starting state: nemo_score_moves' dll there."""
    m, perms, pos, w01, wa, thr = sr.factored_case(name)
    eng = _factored_engine(m)
    try:
        gain = eng.edge_sweep(pos, w01, wa, thr)[4]
        ll, dll = eng.score_moves(pos, w01, wa)
        refs = mr.factored_refs(name, 0)       # (S <= 17: sweep_ref keeps every evaluation)
        for k, perm in enumerate(perms):
            i, j = perm[1], perm[0]
            assert abs(gain[k, i, j] - dll[k, i, j]) <= 2.0 * refs[k].tol[i, j], (name, k)
    finally:
        eng.close()


# ---- entry checks -----------------------------------------------------------------------------------
def test_entry_checks():
    import torch
    name = "small-S15-E17"
    m, perms, pos, w01, wa, thr = sr.factored_case(name)
    lib = _lib.load()
    f32 = Engine(m.U, m.T, dtype="f32")
    try:
        with pytest.raises(RuntimeError, match="f32") as ei:
            f32.edge_sweep(pos, w01, wa, thr)
        assert ei.value.code == _lib.NEMO_ERR_ARG
    finally:
        f32.close()
    eng = _factored_engine(m)
    try:
        b, s = pos.shape[0], m.S
        a = _lib.addr
        wo, ao, g = (np.full((b, s, s), 7.0) for _ in range(3))
        l0, l1 = np.full(b, 7.0), np.full(b, 7.0)
        na = np.full(b, 7, dtype=np.int32)
        outs = (a(wo), a(ao), a(l0), a(l1), a(g), a(na))

        def call(p=pos, w=w01, al=wa, th=thr, cap=0, n=b, o=outs):
            return lib.nemo_edge_sweep(eng.handle, n, a(p), a(w), a(al), a(th), cap, *o)

        i, j = np.argwhere(mr.permissible(perms[1]))[4]
        for bad in (np.nan, np.inf, -np.inf, -1e-9, 1.0 + 1e-9):
            w = wa.copy()
            w[1, i, j] = bad
            assert call(al=w) == _lib.NEMO_ERR_ARG, bad
            assert b"w_alt[1]" in lib.nemo_last_error()
        t = thr.copy()
        t[1, i, j] = np.nan
        assert call(th=t) == _lib.NEMO_ERR_ARG
        assert b"thr[1]" in lib.nemo_last_error()
        p = pos.copy()
        p[2, 0] = p[2, 1]
        assert call(p=p) == _lib.NEMO_ERR_ARG
        assert call(cap=-1) == _lib.NEMO_ERR_ARG
        for k in (0, 1, 3):     # the required outputs: w_out, alt_out, ll_out
            o = list(outs)
            o[k] = None
            assert call(o=o) == _lib.NEMO_ERR_ARG, k
        assert lib.nemo_edge_sweep(eng.handle, b, a(pos), a(w01), a(wa), None, 0, *outs) == _lib.NEMO_ERR_ARG
        assert lib.nemo_edge_sweep(eng.handle, b, None, a(w01), a(wa), a(thr), 0, *outs) == _lib.NEMO_ERR_ARG
        assert lib.nemo_edge_sweep(eng.handle, b, a(pos), None, a(wa), a(thr), 0, *outs) == _lib.NEMO_ERR_ARG
        assert lib.nemo_edge_sweep(eng.handle, b, a(pos), a(w01), None, a(thr), 0, *outs) == _lib.NEMO_ERR_ARG
        for x in (wo, ao, g, l0, l1, na):
            assert (x == 7).all()                             # no refused call wrote anything
        assert lib.nemo_edge_sweep(eng.handle, 0, *([None] * 4), 0, *([None] * 6)) == _lib.NEMO_OK
        # the same values at a pair that is not permissible are not looked at; the optional outputs may be null
        w, t = wa.copy(), thr.copy()
        w[1, j, i] = np.nan
        t[1, j, i] = np.nan
        assert call(al=w, th=t, o=(a(wo), a(ao), None, a(l1), None, None)) == _lib.NEMO_OK
        want = eng.edge_sweep(pos, w01, wa, thr)
        ok = np.stack([mr.permissible(q) for q in perms])
        assert np.array_equal(wo[ok], want[0][ok]) and np.array_equal(ao[ok], want[1][ok]) and np.array_equal(l1, want[3])
        assert np.isnan(ao[1, j, i]) and (l0 == 7.0).all() and (g == 7.0).all() and (na == 7).all()
        # the device entry
        eng.reserve(b)
        tile = lambda x: torch.from_numpy(np.tile(x, (2,) + (1,) * (x.ndim - 1))).cuda()      # noqa: E731
        dpos, dw, dwa, dthr = tile(pos), tile(w01), tile(wa), tile(thr)
        dwo, dao = torch.zeros_like(dw), torch.zeros_like(dwa)
        dll = torch.zeros(2 * b, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        args = [dpos.data_ptr(), dw.data_ptr(), dwa.data_ptr(), dthr.data_ptr(), 0, dwo.data_ptr(), dao.data_ptr(),
                None, dll.data_ptr(), None, None, None]
        assert lib.nemo_edge_sweep_dev(eng.handle, 2 * b, *args) == _lib.NEMO_ERR_STATE
        assert b"reserved" in lib.nemo_last_error()
        for k in (0, 1, 2, 3, 5, 6, 8):
            aa = list(args)
            aa[k] = None
            assert lib.nemo_edge_sweep_dev(eng.handle, b, *aa) == _lib.NEMO_ERR_ARG, k
        aa = list(args)
        aa[4] = -1
        assert lib.nemo_edge_sweep_dev(eng.handle, b, *aa) == _lib.NEMO_ERR_ARG
        assert lib.nemo_edge_sweep_dev(eng.handle, 0, *args) == _lib.NEMO_OK
        torch.cuda.synchronize()
        assert float(dwo.abs().sum()) == 0.0 and float(dll.abs().sum()) == 0.0      # no refused call wrote anything
        # a NaN threshold on the device entry never takes its move
        t = thr.copy()
        t[1, i, j] = np.nan
        t2 = thr.copy()
        t2[1, i, j] = np.inf
        assert _bits_equal(_dev(eng, pos, w01, wa, t, 0), eng.edge_sweep(pos, w01, wa, t2))
    finally:
        eng.close()


def test_e_past_the_bound_is_refused():
    from nemo import limits
    s, e = 2, limits.MAX_E_EDGE_SWEEP + 1
    m = sr.get_model(f"small-S{s}-E{e}")
    eng = _factored_engine(m)
    try:
        pos = np.array([[0, 1]], dtype=np.int32)
        z = np.zeros((1, s, s))
        with pytest.raises(RuntimeError, match=str(limits.MAX_E_EDGE_SWEEP)) as ei:
            eng.edge_sweep(pos, z, 1.0 - z, z)
        assert ei.value.code == _lib.NEMO_ERR_ARG
    finally:
        eng.close()


# ---- the Python layer ---------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["zero", "rounded"])
def test_sweep_flips(start):
    from nemo.methods import sweep_flips
    m, pos, w0 = mr.greedy_inputs(start)
    cpu = sr.Recording(sr.NumpySweepEngine(m.U, m.T))
    want_w, want_ll, want_n, want_sweeps = sweep_flips(cpu, pos, w0)
    eng = _factored_engine(m)
    try:
        rec = sr.Recording(eng)
        trace = []
        w, ll, n, sweeps = sweep_flips(rec, pos, w0, ll_trace=trace)
    finally:
        eng.close()
    assert sweeps == want_sweeps and np.array_equal(n, want_n) and np.array_equal(w, want_w)
    for got, want in zip(rec.calls, cpu.calls):      # the CPU run's flips, sweep by sweep (its margins: test_sweep_cpu.py)
        assert np.array_equal(got[1], want[1])
    et = np.exp(m.T.astype(LD))
    lls = np.stack(trace)
    for k in range(len(pos)):
        ref = mr.moves_reference(m.U, m.T, np.argsort(pos[k]), w[k], 1.0 - w[k], et=et)
        assert abs(float(LD(ll[k]) - ref.cs.sum())) <= ref.tol_ll, (start, k)
        assert (np.diff(lls[:, k]) >= -2.0 * ref.tol_ll).all(), (start, k, "ll fell")


def test_sweep_method():
    from nemo.methods import SweepMethod, sweep_flips
    m, pos, _ = mr.greedy_inputs("zero")
    order = np.argsort(pos[0])
    want_w, _, want_n, want_sweeps = sweep_flips(sr.NumpySweepEngine(m.U, m.T), pos[:1], np.zeros((1, m.S, m.S)))
    sm_ = SweepMethod(order, m.S, m.E, m.U, m.T)
    try:
        dag_t, ll = sm_.optimize()
        assert sm_.n_flips == int(want_n[0]) and sm_.n_sweeps == want_sweeps and len(sm_.ll_list) == want_sweeps + 1
        assert np.array_equal(dag_t.T, want_w[0]) and sm_.ll_list[-1] == ll
        assert abs(ll - sm_._ll_of(dag_t.T)) <= 1e-8          # the engine's own (int8) score of the same DAG
        _, ll1 = sm_.optimize(max_sweeps=1)
        assert sm_.n_sweeps == 1 and len(sm_.ll_list) == 2 and ll1 == sm_.ll_list[-1]
    finally:
        sm_.engine.close()


def test_gibbs_edges():
    from nemo.methods import gibbs_edges
    m, pos, w0 = sr.gibbs_inputs()
    kw = dict(beta=sr.GIBBS_BETA, log_prior_odds=sr.GIBBS_RHO, burn_in=sr.GIBBS_BURN, rng=sr.GIBBS_SEED)
    cpu = sr.Recording(sr.NumpySweepEngine(m.U, m.T))
    want_w, want_ll, want_p = gibbs_edges(cpu, pos, w0, sr.GIBBS_SWEEPS, **kw)
    eng = _factored_engine(m)
    try:
        w, lls, prob = gibbs_edges(eng, pos, w0, sr.GIBBS_SWEEPS, **kw)
    finally:
        eng.close()
    assert np.array_equal(w, want_w)
    # |d sigmoid| <= |beta d gain| / 4; the device is within tol of the reference and numpy within a half
    refs = sr.call_refs(m, cpu.calls)
    bound = np.zeros_like(prob)
    for row in refs[sr.GIBBS_BURN:]:
        bound += np.stack([r.tol for r in row]) * (1.5 * sr.GIBBS_BETA / 4.0)
    bound /= sr.GIBBS_SWEEPS - sr.GIBBS_BURN
    assert (np.abs(prob - want_p) <= bound + 2.0 ** -52).all(), float(np.abs(prob - want_p).max())
    for k in range(len(pos)):
        assert abs(lls[-1, k] - want_ll[-1, k]) <= 1.5 * refs[-1][k].tol_ll
