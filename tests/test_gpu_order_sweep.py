"""nemo_order_sweep / nemo_order_sweep_dev (csrc/nemo_order_sweep.hip) against the
long-double sweep of tests/order_sweep_ref.py (GPU).

Inputs: order_sweep_ref's lists -- S = 2 (one relocation per node), S = 3, S = 15,
16, 17, 33, 60, 64, S = 128 with 16 visits, S = 17 at E = 1, 15, 16, 17, 63, 64, 65
(wave and word edges), at E on each side of every switch of the block size (64 | 65,
128 | 129, 256 | 257, 512 | 513) and of the effects per thread (1024 | 1025) and at E
= 1040, three table-built models, and every generic case of score_grad_ref.GENERIC.
Two sweeps in label order (nvisit = 2 S), so the second runs on an updated, drifted
state.  Each case runs with seeded uniforms where tests/test_order_sweep_cpu.py
asserts a positive decision margin at every visit (then q, pos_out and nmoved must
EQUAL the reference's) and with forced uniforms, u alternating 0 and 2.0 (then they
equal what u dictates: position 0, position S - 1 -- the longest walks); nem12 at S
= 64, the mirrored deep table and the amplitude-70 and -171 tables, whose tolerance
is too wide for a margin, run forced alone.

Per case: |dll - ref| <= the visit's tolerance (reloc_ref's, widened by the drift
bound derived in order_sweep_ref), exactly +0.0 at the visited node's position,
ll_vis and ll within tol_ll plus drift, ll within twice that of nemo_score_grad's ll
of (pos_out, w01); the same bits, decisions included, with NaN on the diagonal of
w01, for a batch of one, for slots of a batch of 37, for a second run, in place and
for the device entry on a side stream with outputs preset to NaN.  Each case prints
its worst error over tolerance (pytest -s).

Observed worst error over tolerance on an MI355X: 0.016 (small-S17-E1), 0.007 on the
other factored models, 0.005 on the real-valued tables; the fused gibbs_orders' worst
z-score 0.89 (MEASUREMENTS.md)."""
import ctypes

import numpy as np
import pytest

import order_sweep_ref as osr
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


def _dev(eng, pos, w, visit, u, beta=1.0, min_gain=0.0, in_place=False):
    """nemo_order_sweep_dev on a side torch stream, outputs preset to NaN (-1 for the integers)."""
    import torch
    b, nv = visit.shape
    eng.reserve(b)
    side = torch.cuda.Stream()
    dpos, dw = torch.from_numpy(pos).cuda(), torch.from_numpy(w).cuda()
    dvisit = torch.from_numpy(visit).cuda()
    du = None if u is None else torch.from_numpy(u).cuda()
    dout = dpos if in_place else torch.full((b, eng.S), -1, dtype=torch.int32, device="cuda")
    f = dict(dtype=torch.float64, device="cuda")
    ll0, ll = torch.full((b,), float("nan"), **f), torch.full((b,), float("nan"), **f)
    dll, vis = torch.full((b, nv, eng.S), float("nan"), **f), torch.full((b, nv), float("nan"), **f)
    q = torch.full((b, nv), -1, dtype=torch.int32, device="cuda")
    nm = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        eng.order_sweep_dev(b, dpos.data_ptr(), dw.data_ptr(), nv, dvisit.data_ptr(),
                            None if du is None else du.data_ptr(), dout.data_ptr(), ll.data_ptr(),
                            d_ll0=ll0.data_ptr(), d_q=q.data_ptr(), d_dll=dll.data_ptr(), d_ll_vis=vis.data_ptr(),
                            d_nmoved=nm.data_ptr(), beta=beta, min_gain=min_gain, stream=side.cuda_stream)
    side.synchronize()
    return tuple(x.cpu().numpy() for x in (dout, ll0, ll, q, dll, vis, nm))


def _same(got, want, tag):
    for x, y, what in zip(got, want, ("pos_out", "ll0", "ll", "q", "dll", "ll_vis", "nmoved")):
        assert np.array_equal(x, y), (tag, what)


def _against_ref(tag, got, refs, want_q=None):
    """-> worst err / tol over the batch; asserts decisions, tolerances and the exact zeros."""
    pos_out, ll0, ll, q, dll, vis, nmoved = got
    worst = 0.0
    for k, ref in enumerate(refs):
        wq = ref.q if want_q is None else want_q
        assert np.array_equal(q[k], wq), (tag, k, "q")
        assert np.array_equal(np.argsort(pos_out[k]), ref.perms[-1]), (tag, k, "pos_out")
        assert nmoved[k] == ref.nmoved, (tag, k, "nmoved")
        assert np.isfinite(dll[k]).all() and np.isfinite(vis[k]).all(), (tag, k)
        s = dll.shape[2]
        for v in range(len(wq)):
            p = ref.p[v]
            assert dll[k, v, p] == 0.0 and not np.signbit(dll[k, v, p]), (tag, k, v, "exact +0.0")
            ok = np.arange(s) != p
            err = np.abs(dll[k, v].astype(LD) - ref.rows[v]).astype(np.float64)
            ratio = err[ok] / ref.tols[v][ok]
            worst = max(worst, float(ratio.max()))
            assert (ratio <= 1.0).all(), (tag, k, v, float(ratio.max()))
            assert abs(float(LD(vis[k, v]) - ref.ll[v + 1])) <= ref.tol_ll[v + 1], (tag, k, v, "ll_vis")
            if wq[v] == p:          # nothing moved: the previous value's bits
                assert vis[k, v] == (vis[k, v - 1] if v else ll0[k]), (tag, k, v, "ll_vis carried")
        assert abs(float(LD(ll0[k]) - ref.ll[0])) <= ref.tol_ll[0], (tag, k, "ll0")
        assert abs(float(LD(ll[k]) - ref.ll[-1])) <= ref.tol_ll[-1], (tag, k, "ll")
        assert ll[k] == (vis[k, -1] if len(wq) else ll0[k]), (tag, k, "ll is the last visit's")
    return worst


def _rescored(eng, tag, got, w, refs):
    """ll_out against nemo_score_grad's ll of (pos_out, w01): within 2 tol_ll + drift (tol_ll carries the drift)."""
    l2, _ = eng.score_grad(got[0], w)
    for k, ref in enumerate(refs):
        assert abs(l2[k] - got[2][k]) <= 2.0 * ref.tol_ll[-1], (tag, k, "against nemo_score_grad")


def _bits(eng, tag, pos, w, visit, u, got):
    """NaN on the diagonal, batch of one, slots of a batch of 37, a second run, in place, the device entry."""
    n = len(pos)
    wn = w.copy()
    wn[:, np.arange(eng.S), np.arange(eng.S)] = np.nan
    _same(eng.order_sweep(pos, wn, visit, u), got, (tag, "NaN on the diagonal"))
    for one in (0, n - 1):
        g1 = eng.order_sweep(pos[one:one + 1], w[one:one + 1], visit[one:one + 1], u[one:one + 1])
        _same(g1, tuple(x[one:one + 1] for x in got), (tag, "batch of one", one))
    idx = (sm.tile_batch(n, 37) + 5) % n
    p37, w37, v37, u37 = (np.ascontiguousarray(x[idx]) for x in (pos, w, visit, u))
    want = tuple(x[idx] for x in got)
    _same(eng.order_sweep(p37, w37, v37, u37), want, (tag, "batch of 37"))
    _same(eng.order_sweep(p37, w37, v37, u37), want, (tag, "second run"))
    _same(_dev(eng, p37, w37, v37, u37), want, (tag, "device entry on a side stream"))
    _same(_dev(eng, p37, w37, v37, u37, in_place=True), want, (tag, "in place"))


def _stack(cases):
    """pos, w, visit, u of a list of (…, pos, w, visit, us) cases as a batch."""
    return tuple(np.ascontiguousarray(np.stack([c[i] for c in cases])) for i in (-4, -3, -2, -1))


def _run_factored(name, forced, bits):
    ks = osr.evals_of(name, forced)
    cases = [osr.factored_sweep_case(name, k, forced) for k in ks]
    refs = [osr.factored_sweep_ref(name, k, forced) for k in ks]
    m = cases[0][0]
    pos, w, visit, u = _stack(cases)
    want_q = osr.forced_q(visit.shape[1], m.S) if forced else None
    eng = _factored_engine(m)
    try:
        got = eng.order_sweep(pos, w, visit, u)
        worst = _against_ref(name, got, refs, want_q)
        _rescored(eng, name, got, w, refs)
        if bits:
            _bits(eng, name, pos, w, visit, u, got)
    finally:
        eng.close()
    print(f"ORDER-SWEEP {name} {'forced' if forced else 'seeded'} worst err/tol: {worst:.4f}")


@pytest.mark.parametrize("name", osr.MARGINED + osr.SHAPES + (rr.WIDE_MODEL,))
def test_factored_seeded(name):
    """Seeded uniforms: the reference's decisions exactly (margins: tests/test_order_sweep_cpu.py)."""
    _run_factored(name, False, True)


@pytest.mark.parametrize("name", osr.MARGINED + osr.SHAPES + osr.FORCED + ("table-edge-S8-E40",))
def test_factored_forced(name):
    """u alternating 0 and 2.0: the visited node to position 0, then to S - 1."""
    _run_factored(name, True, name in osr.FORCED)


@pytest.mark.parametrize("name", rr.GENERIC)
def test_generic_tables(name):
    c = rr.generic_case(name)[0]
    eng = _generic_engine(c)
    try:
        for forced in (True, False):
            if not forced and name not in osr.GENERIC_MARGINED:
                continue
            ks = (0, 1, 5) if forced and c.s <= 18 else (0,)
            cases = [osr.generic_sweep_case(name, k, forced) for k in ks]
            refs = [osr.generic_sweep_ref(name, k, forced) for k in ks]
            pos, w, visit, u = _stack(cases)
            got = eng.order_sweep(pos, w, visit, u)
            worst = _against_ref(name, got, refs, osr.forced_q(visit.shape[1], c.s) if forced else None)
            _rescored(eng, name, got, w, refs)
            if forced:
                _bits(eng, name, pos, w, visit, u, got)
            print(f"ORDER-SWEEP {name} {'forced' if forced else 'seeded'} worst err/tol: {worst:.4f}")
    finally:
        eng.close()


def test_visit_lists():
    """A node repeated back to back (the second visit sees the first one's move), a list that is no
    permutation, no visits at all, and the nullable outputs left out."""
    name = "nem04-S16-E40"
    m, perms, pos, w = rr.factored_case(name)
    et = np.exp(m.T.astype(LD))
    lists = (np.array([3, 3, 3, 7, 7, 0, 3], dtype=np.int32), np.array([5, 1, 5, 1, 9, 9, 2], dtype=np.int32))
    eng = _factored_engine(m)
    try:
        for visit in lists:
            ks = (0, 1, 5)
            us = [osr.seeded_u(len(visit), 100 + k) for k in ks]
            refs = [osr.sweep_reference(m.U, m.T, perms[k], w[k], visit, us[i], et=et) for i, k in enumerate(ks)]
            assert all((r.margin > 0.0).all() for r in refs)
            p, ww = np.ascontiguousarray(pos[list(ks)]), np.ascontiguousarray(w[list(ks)])
            vv, uu = np.ascontiguousarray(np.tile(visit, (3, 1))), np.ascontiguousarray(np.stack(us))
            got = eng.order_sweep(p, ww, vv, uu)
            _against_ref((name, tuple(visit)), got, refs)
            # the nullable outputs one by one: the others keep their bits
            lib, a = _lib.load(), _lib.addr
            for drop in range(5):
                out = [np.empty_like(x) for x in got]
                args = [a(out[1]), a(out[2]), a(out[3]), a(out[4]), a(out[5]), a(out[6])]
                args[(0, 2, 3, 4, 5)[drop]] = None
                rc = lib.nemo_order_sweep(eng.handle, 3, a(p), a(ww), len(visit), a(vv), a(uu), 1.0, 0.0, 0,
                                          a(out[0]), *args)
                assert rc == _lib.NEMO_OK
                for i in range(7):
                    if i != (1, 3, 4, 5, 6)[drop]:
                        assert np.array_equal(out[i], got[i]), (drop, i)
        # nvisit = 0: the state is scored and pos copied through
        got0 = eng.order_sweep(pos, w, np.zeros((len(pos), 0), dtype=np.int32))
        ll, _ = eng.score_relocations(pos, w)
        refs = rr.factored_refs(name)
        assert np.array_equal(got0[0], pos) and np.array_equal(got0[1], got0[2]) and not got0[6].any()
        for k, ref in enumerate(refs):
            assert abs(float(LD(got0[2][k]) - ref.cs.sum())) <= ref.tol_ll and abs(got0[2][k] - ll[k]) <= 2 * ref.tol_ll
    finally:
        eng.close()


def test_greedy_mode():
    """beta = inf on reloc_ref.greedy_inputs(): the reference's decisions (its margins:
    tests/test_order_sweep_cpu.py), which are the numpy engine's; u is not read (null)."""
    m, pos, w = rr.greedy_inputs()
    refs = osr.greedy_sweep_refs()
    visit = np.ascontiguousarray(np.tile(osr.label_sweeps(m.S), (len(pos), 1)))
    cpu = osr.NumpyEngine(m.U, m.T).order_sweep(pos, w, visit, beta=np.inf, min_gain=1e-9)
    eng = _factored_engine(m)
    try:
        got = eng.order_sweep(pos, w, visit, beta=np.inf, min_gain=1e-9)
        worst = _against_ref("greedy", got, refs)
        assert np.array_equal(got[3], cpu[3]) and np.array_equal(got[0], cpu[0]) and np.array_equal(got[6], cpu[6])
        _same(_dev(eng, pos, w, visit, None, beta=np.inf, min_gain=1e-9), got, "greedy, device entry, null u")
        # a huge min_gain takes nothing: the order and the score's bits stay
        none = eng.order_sweep(pos, w, visit, beta=np.inf, min_gain=1e300)
        assert np.array_equal(none[0], pos) and not none[6].any() and np.array_equal(none[2], none[1])
        assert np.array_equal(none[3], pos[:, :m.S]) and (none[5] == none[1][:, None]).all()
    finally:
        eng.close()
    print(f"ORDER-SWEEP greedy worst err/tol: {worst:.4f}")


def test_entry_checks():
    import torch
    m, perms, pos, w = rr.factored_case("small-S15-E16")
    lib = _lib.load()
    a = _lib.addr
    b, s = pos.shape
    nv = s
    visit = np.ascontiguousarray(np.tile(osr.label_sweeps(s), (b, 1)))
    u = np.ascontiguousarray(np.stack([osr.seeded_u(nv, k) for k in range(b)]))
    f32 = Engine(m.U, m.T, dtype="f32")
    try:
        with pytest.raises(RuntimeError, match="f32") as ei:
            f32.order_sweep(pos, w, visit, u)
        assert ei.value.code == _lib.NEMO_ERR_ARG
    finally:
        f32.close()
    po = np.full((b, s), 7, dtype=np.int32)
    ll0, ll = np.full(b, 7.0), np.full(b, 7.0)
    q = np.full((b, nv), 7, dtype=np.int32)
    d = np.full((b, nv, s), 7.0)
    vis = np.full((b, nv), 7.0)
    nm = np.full(b, 7, dtype=np.int32)
    outs = (a(po), a(ll0), a(ll), a(q), a(d), a(vis), a(nm))

    def call(h, pos_=pos, w_=w, nv_=nv, visit_=visit, u_=u, beta=1.0, mg=0.0, cap=0, bb=b):
        return lib.nemo_order_sweep(h, bb, a(pos_), a(w_), nv_, a(visit_), None if u_ is None else a(u_), beta, mg,
                                    cap, *outs)

    ctx = ctypes.c_void_p()
    assert lib.nemo_ctx_create(0, m.S, m.E, _lib.NEMO_F64, ctypes.byref(ctx)) == _lib.NEMO_OK
    try:
        assert call(ctx) == _lib.NEMO_ERR_STATE               # unstaged
        assert lib.nemo_order_sweep_dev(ctx, b, a(pos), a(w), nv, a(visit), a(u), 1.0, 0.0, 0, *outs,
                                        None) == _lib.NEMO_ERR_STATE
    finally:
        lib.nemo_ctx_destroy(ctx)
    eng = _factored_engine(m)
    h = eng.handle
    try:
        for cap in (1, 3, s - 2):
            assert call(h, cap=cap) == _lib.NEMO_ERR_ARG, cap
            assert b"cap" in lib.nemo_last_error()
        assert call(h, cap=-1) == _lib.NEMO_ERR_ARG
        assert call(h, nv_=-1) == _lib.NEMO_ERR_ARG
        for beta in (0.0, -1.0, np.nan, -np.inf):
            assert call(h, beta=beta) == _lib.NEMO_ERR_ARG, beta
            assert b"beta" in lib.nemo_last_error()
        for mg in (-1e-300, np.nan, -np.inf):
            assert call(h, mg=mg) == _lib.NEMO_ERR_ARG, mg
            assert b"min_gain" in lib.nemo_last_error()
        i, j = perms[1][3], perms[1][9]
        for bad in (np.nan, np.inf, -np.inf, -1e-9, 1.0 + 1e-9):
            for ii, jj in ((i, j), (j, i)):
                wb = w.copy()
                wb[1, ii, jj] = bad
                assert call(h, w_=wb) == _lib.NEMO_ERR_ARG
                assert b"w01[1]" in lib.nemo_last_error()
        p = pos.copy()
        p[2, 0] = p[2, 1]
        assert call(h, pos_=p) == _lib.NEMO_ERR_ARG
        for bad in (-1, s, 1 << 30):
            vb = visit.copy()
            vb[2, 4] = bad
            assert call(h, visit_=vb) == _lib.NEMO_ERR_ARG
            assert b"visit[2][4]" in lib.nemo_last_error()
        for bad in (np.nan, np.inf, -1e-9):
            ub = u.copy()
            ub[1, 6] = bad
            assert call(h, u_=ub) == _lib.NEMO_ERR_ARG
            assert b"u[1][6]" in lib.nemo_last_error()
            assert call(h, u_=ub, beta=np.inf) == _lib.NEMO_OK        # greedy: u is not read
            for x in (po, q, nm):
                x[:] = 7
            for x in (ll0, ll, d, vis):
                x[:] = 7.0
        assert call(h, u_=None) == _lib.NEMO_ERR_ARG                   # Gibbs needs u
        assert lib.nemo_order_sweep(h, 0, None, None, 0, None, None, 1.0, 0.0, 0, *([None] * 7)) == _lib.NEMO_OK
        # null pointers one by one: pos, w01, visit, pos_out, ll_out are required
        base = [a(pos), a(w), nv, a(visit), a(u), 1.0, 0.0, 0, *outs]
        for k in (0, 1, 3, 8, 10):
            args = list(base)
            args[k] = None
            assert lib.nemo_order_sweep(h, b, *args) == _lib.NEMO_ERR_ARG, k
        assert (po == 7).all() and (ll0 == 7.0).all() and (ll == 7.0).all() and (q == 7).all()
        assert (d == 7.0).all() and (vis == 7.0).all() and (nm == 7).all()        # no refused call wrote anything
        # the device entry
        eng.reserve(b)
        t2 = lambda x: torch.from_numpy(np.tile(x, (2,) + (1,) * (x.ndim - 1))).cuda()     # noqa: E731
        dpos, dw, dv, du = t2(pos), t2(w), t2(visit), t2(u)
        dpo = torch.zeros((2 * b, s), dtype=torch.int32, device="cuda")
        dl0 = torch.zeros(2 * b, dtype=torch.float64, device="cuda")
        dl = torch.zeros(2 * b, dtype=torch.float64, device="cuda")
        dq = torch.zeros((2 * b, nv), dtype=torch.int32, device="cuda")
        dd = torch.zeros((2 * b, nv, s), dtype=torch.float64, device="cuda")
        dvis = torch.zeros((2 * b, nv), dtype=torch.float64, device="cuda")
        dnm = torch.zeros(2 * b, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        args = [dpos.data_ptr(), dw.data_ptr(), nv, dv.data_ptr(), du.data_ptr(), 1.0, 0.0, 0, dpo.data_ptr(),
                dl0.data_ptr(), dl.data_ptr(), dq.data_ptr(), dd.data_ptr(), dvis.data_ptr(), dnm.data_ptr(), None]
        assert lib.nemo_order_sweep_dev(h, 2 * b, *args) == _lib.NEMO_ERR_STATE
        assert b"reserved" in lib.nemo_last_error()
        for k in (0, 1, 3, 4, 8, 10):
            aa = list(args)
            aa[k] = None
            assert lib.nemo_order_sweep_dev(h, b, *aa) == _lib.NEMO_ERR_ARG, k
        for k, bad in ((7, -1), (7, 2), (7, s - 2), (2, -1), (5, 0.0), (5, float("nan")), (6, -1.0), (6, float("nan"))):
            aa = list(args)
            aa[k] = bad
            assert lib.nemo_order_sweep_dev(h, b, *aa) == _lib.NEMO_ERR_ARG, (k, bad)
        assert lib.nemo_order_sweep_dev(h, 0, *args) == _lib.NEMO_OK
        eng.set_option("timing_kernel", 5)
        eng.set_option("timing_kernel", 0)
        with pytest.raises(_lib.NemoError, match="5 order sweeps"):
            eng.set_option("timing_kernel", 6)
        torch.cuda.synchronize()
        for x in (dpo, dl0, dl, dq, dd, dvis, dnm):
            assert float(x.double().abs().sum()) == 0.0                  # no refused call wrote anything
    finally:
        eng.close()


def test_nan_inputs_on_the_device_entry():
    """The device entry cannot refuse a NaN weight or uniform: every q is within [0, S - 1], the order returned
    is a permutation and the one replayed from q, a visit whose row holds a NaN moves nothing (the walk's
    log1p floors a NaN sum, so such rows are rare), and the clean slot of the batch keeps its bits."""
    m, perms, pos, w = rr.factored_case("small-S15-E16")
    s = m.S
    visit = np.ascontiguousarray(np.tile(osr.label_sweeps(s), (2, 1)))
    u = np.ascontiguousarray(np.stack([osr.seeded_u(s, k) for k in range(2)]))
    wn = np.ascontiguousarray(w[:2]).copy()
    wn[1, 4, :] = np.nan                  # node 4's weights as a child: every row that passes 4 or visits 4
    un = u.copy()
    un[1, 3::4] = np.nan
    eng = _factored_engine(m)
    try:
        clean = _dev(eng, np.ascontiguousarray(pos[:2]), np.ascontiguousarray(w[:2]), visit, u)
        got = _dev(eng, np.ascontiguousarray(pos[:2]), wn, visit, un)
    finally:
        eng.close()
    for x, y in zip(got, clean):
        assert np.array_equal(x[0], y[0])                               # the clean slot: the same bits
    pos_out, _, _, q, dll, _, nmoved = got
    assert sorted(pos_out[1]) == list(range(s)) and (q[1] >= 0).all() and (q[1] < s).all()
    held = pos[1].copy()
    from nemo.methods import apply_relocation
    for v in range(s):
        if np.isnan(dll[1, v]).any():
            assert q[1, v] == held[v], v
        held = apply_relocation(held, v, int(q[1, v]))
    assert np.array_equal(held, pos_out[1])


def test_gibbs_orders_fused():
    """The S = 4 model on the device, one order_sweep call per sweep: the numpy engine's chains (the margin of
    every draw: tests/test_order_sweep_cpu.py) and the marginals within 3 standard errors of the enumeration."""
    from nemo.methods import gibbs_orders
    u, t, w = rr.gibbs_model()
    exact = rr.gibbs_enumeration()
    b = rr.GIBBS_CHAINS
    pos = osr.gibbs_start()
    wb = np.ascontiguousarray(np.broadcast_to(w, (b, 4, 4)))
    least, want_pos = osr.gibbs_margins()
    assert least > 0.0
    cpu = gibbs_orders(osr.NumpyEngine(u, t), pos, wb, rr.GIBBS_SWEEPS, burn_in=rr.GIBBS_BURN, rng=rr.GIBBS_SEED,
                       fused=True)
    eng = Engine(u, t)
    try:
        out_pos, lls, before = gibbs_orders(eng, pos, wb, rr.GIBBS_SWEEPS, burn_in=rr.GIBBS_BURN, rng=rr.GIBBS_SEED,
                                            fused=True)
        ll_end, _ = eng.score_relocations(out_pos, wb)
    finally:
        eng.close()
    assert np.array_equal(out_pos, want_pos) and np.array_equal(out_pos, cpu[0])
    assert lls.shape == (rr.GIBBS_SWEEPS * 4, b) and np.abs(lls - cpu[1]).max() <= 1e-9
    assert np.abs(lls[-1] - ll_end).max() <= 1e-9
    assert np.abs(before - cpu[2]).max() <= 1e-9
    z = rr.gibbs_z(before, exact)
    print(f"ORDER-SWEEP gibbs_orders fused (device): worst z-score {z:.2f}")
    assert z <= 3.0, z


def test_sweep_relocations():
    """Ends where no single relocation gains more than min_gain plus tolerance."""
    from nemo.methods import sweep_relocations
    m, pos, w = rr.greedy_inputs()
    et = np.exp(m.T.astype(LD))
    eng = _factored_engine(m)
    try:
        trace = []
        out, ll, n, sweeps = sweep_relocations(eng, pos, w, ll_trace=trace)
    finally:
        eng.close()
    assert sweeps >= 2 and len(trace) == sweeps + 1 and np.array_equal(trace[-1], trace[-2])
    assert (n >= [r.nmoved for r in osr.greedy_sweep_refs()]).all()
    for k in range(len(pos)):
        ref = rr.reloc_reference(m.U, m.T, np.argsort(out[k]), w[k], et=et)
        stay = ref.tol == 0.0
        assert (ref.dll[~stay] <= 1e-9 + ref.tol[~stay]).all(), (k, "a single relocation still gains")
        assert abs(float(LD(ll[k]) - ref.cs.sum())) <= ref.tol_ll, k       # the last sweep moved nothing: a forward's ll
        assert (np.diff(np.stack(trace)[:, k]) >= -2.0 * ref.tol_ll).all(), (k, "ll fell")
