"""nemo_score_rates / nemo_score_rates_dev (csrc/nemo_grad.hip) against the
long-double reference of tests/rates_ref.py (GPU).

Models: the error-rate ladder's rungs nem00 / nem04 / nem08 / nem12 at S = 16,
33, 60, 64 and E = 40, 130 (their own knockdown matrices), and seeded matrices
of density 0.4 at S = 2, 15, 17 x E = 1, 15, 16, 17, 63, 64, 65 and at S = 17, E
= 1040 (two parts of the fused kernel's cut of E), with rows that start with 1
and with 0, an all-ones row and (S > 2) an all-zeros row.  Rates: (a) the
model's own scalar pair, (b) per-gene rates log-uniform in [1e-9, 0.45], all
distinct, (c) a different such vector for every evaluation of the batch.
Evaluations: fixed_point_models.inputs; caps: score_grad_ref.factored_caps.  The
weights off the permissible set are NaN: they must not be read.

Per case and cap: ll, grad, dA and dB within rates_ref's tolerances, exact
zeros of grad off the permissible set, the same bits for a batch of one, for the
slots of a batch of 37, for a second run and from the device entry on a side
stream; at (a), ll and grad within twice their tolerances of nemo_score_grad on
the same engine.  Each case prints its worst error over tolerance (pytest -s)."""
import numpy as np
import pytest

import rates_ref as rr
import score_grad_ref as gr
import stream_models as sm
from nemo import _lib
from nemo.engine import Engine

pytestmark = pytest.mark.gpu

LD = np.longdouble


def _engine(name):
    d, (a0, b0) = rr.model_d(name)
    return Engine.from_knockdown(d, a0, b0)


def _poisoned(w01, perms, cap):
    w = w01.copy()
    for k, perm in enumerate(perms):
        w[k][~gr.permissible(perm, cap)] = np.nan
    return w


def _worst(tag, got, refs, perms, cap):
    """-> worst err / tol over (ll, grad, dA, dB); asserts every tolerance and the exact zeros."""
    ll, da, db, g = got
    worst = 0.0
    for k, ref in enumerate(refs):
        ok = gr.permissible(perms[k], cap)
        assert np.isfinite(ll[k]) and np.isfinite(g[k]).all() and np.isfinite(da[k]).all() and np.isfinite(db[k]).all(), \
            (tag, cap, k)
        off = g[k][~ok]
        assert (off == 0.0).all() and not np.signbit(off).any(), (tag, cap, k, "grad off the permissible set")
        r = abs(float(LD(ll[k]) - ref.cs.sum())) / ref.tol_ll
        assert r <= 1.0, (tag, cap, k, "ll", r)
        worst = max(worst, r)
        for what, x, want, tol in (("grad", g[k][ok], ref.g[ok], ref.tol[ok]), ("dA", da[k], ref.da, ref.tol_a),
                                   ("dB", db[k], ref.db, ref.tol_b)):
            err = np.abs(x.astype(LD) - want).astype(np.float64)
            pos = tol > 0.0
            r = float((err[pos] / tol[pos]).max()) if pos.any() else 0.0
            assert (err <= tol).all(), (tag, cap, k, what, r)
            worst = max(worst, r)
    return worst


def _dev(eng, pos, w, a, b, cap):
    """nemo_score_rates_dev on a side torch stream, outputs preset to NaN."""
    import torch
    n = pos.shape[0]
    eng.reserve(n)
    side = torch.cuda.Stream()
    dpos, dw = torch.from_numpy(pos).cuda(), torch.from_numpy(w).cuda()
    dr = torch.from_numpy(np.ascontiguousarray(np.stack([a, b], axis=1))).cuda()
    dll = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    ddr = torch.full((n, 2, eng.S), float("nan"), dtype=torch.float64, device="cuda")
    dg = torch.full((n, eng.S, eng.S), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        eng.score_rates_dev(n, dpos.data_ptr(), dw.data_ptr(), dr.data_ptr(), dll.data_ptr(), ddr.data_ptr(),
                            dg.data_ptr(), cap=cap, stream=side.cuda_stream)
    side.synchronize()
    ddr = ddr.cpu().numpy()
    return dll.cpu().numpy(), ddr[:, 0], ddr[:, 1], dg.cpu().numpy()


def _same(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


def _bits(eng, tag, pos, w01, a, b, cap, got):
    """A batch of one, the slots of a batch of 37, a second run, the device entry, and no gradient asked."""
    n = pos.shape[0]
    for one in (0, n - 1):
        sl = slice(one, one + 1)
        g1 = eng.score_rates(pos[sl], w01[sl], a[sl], b[sl], cap=cap)
        assert _same(g1, [x[sl] for x in got]), (tag, cap, "batch of one", one)
    idx = (sm.tile_batch(n, 37) + 5) % n
    args = [np.ascontiguousarray(x[idx]) for x in (pos, w01, a, b)]
    g37 = eng.score_rates(*args, cap=cap)
    assert _same(g37, [x[idx] for x in got]), (tag, cap, "batch of 37")
    assert _same(eng.score_rates(*args, cap=cap), g37), (tag, cap, "second run")
    assert _same(_dev(eng, *args, cap), g37), (tag, cap, "device entry on a side stream")
    l0, a0, b0, none = eng.score_rates(*args, cap=cap, want_grad_w=False)
    assert none is None and _same((l0, a0, b0), g37[:3]), (tag, cap, "without grad")


@pytest.mark.parametrize("setting", rr.SETTINGS)
@pytest.mark.parametrize("name", rr.ladder_ids() + rr.small_ids())
def test_score_rates(name, setting):
    d, perms, pos, w01, a, b = rr.case_inputs(name, setting)
    s = d.shape[0]
    eng = _engine(name)
    worst = 0.0
    try:
        for cap in gr.factored_caps(s):
            ecap = 0 if cap >= s - 1 else cap
            refs = rr.case_refs(name, setting, ecap)
            w = _poisoned(w01, perms, cap)
            got = eng.score_rates(pos, w, a, b, cap=cap)
            worst = max(worst, _worst(f"{name} {setting}", got, refs, perms, cap))
            _bits(eng, f"{name} {setting}", pos, w, a, b, cap, got)
            if setting == "scalar":
                ll2, g2 = eng.score_grad(pos, w, cap=cap)
                for k, ref in enumerate(refs):
                    assert abs(got[0][k] - ll2[k]) <= 2.0 * ref.tol_ll, (name, cap, k, "ll against nemo_score_grad")
                    assert (np.abs(got[3][k] - g2[k]) <= 2.0 * ref.tol).all(), (name, cap, k, "grad against nemo_score_grad")
    finally:
        eng.close()
    print(f"RATES {name} {setting} worst err/tol {worst:.3f}")


def test_scalar_and_vector_rates_broadcast_alike():
    name = "small-S15-E17"
    d, perms, pos, w01, a, b = rr.case_inputs(name, "scalar")
    eng = _engine(name)
    try:
        want = eng.score_rates(pos, w01, a, b)
        assert _same(eng.score_rates(pos, w01, float(a[0, 0]), float(b[0, 0])), want)
        assert _same(eng.score_rates(pos, w01, a[0], b[0]), want)
    finally:
        eng.close()


@pytest.mark.parametrize("s", rr.DIAG_S)
def test_diagonal_alone_at_zero_weights(s):
    """With every weight 0 no pair contributes: dA_k = n_k - M_kk and dB_k = R_k - M_kk, the diagonal
    sums alone -- at every order position, those = 15 mod 16 (where the diagonal tile's row carries R)
    included, under orders that put distinct genes there.  The expectation is formed here, directly,
    in long double."""
    e = 130
    d = rr.small_d(s, e)
    a, b = rr.per_gene_rates(s, 77 + s)
    rng = np.random.default_rng(s)
    perms = [rng.permutation(s) for _ in range(3)]
    at15 = [tuple(p[15::16]) for p in perms]
    assert len(set(at15)) == 3
    pos = np.empty((3, s), dtype=np.int32)
    for k, p in enumerate(perms):
        pos[k, p] = np.arange(s)
    x = np.where(d.astype(bool), -a.astype(LD)[:, None], b.astype(LD)[:, None])
    ow = np.exp(x) / (1 + np.exp(x).sum(axis=0))
    mkk, rk, nk = (ow * d).sum(axis=1), ow.sum(axis=1), d.sum(axis=1).astype(LD)
    eng = Engine.from_knockdown(d, -1.0, -2.0)
    try:
        ll, da, db, g = eng.score_rates(pos, np.zeros((3, s, s)), a, b)
        for k in range(3):
            ref = rr.rates_reference(d, a, b, perms[k], np.zeros((s, s)))
            assert (np.abs(da[k].astype(LD) - (nk - mkk)).astype(np.float64) <= ref.tol_a).all(), (s, k, "dA")
            assert (np.abs(db[k].astype(LD) - (rk - mkk)).astype(np.float64) <= ref.tol_b).all(), (s, k, "dB")
            assert abs(float(LD(ll[k]) - ref.cs.sum())) <= ref.tol_ll
            assert np.isfinite(g[k]).all() and (g[k][~gr.permissible(perms[k])] == 0.0).all()
    finally:
        eng.close()


def _refused(fn, code, match):
    with pytest.raises(_lib.NemoError, match=match) as ei:
        fn()
    assert ei.value.code == code


def test_refusals():
    import torch
    rng = np.random.default_rng(1)
    # S = 65
    d65 = (rng.random((65, 20)) < 0.4).astype(np.uint8)
    eng = Engine.from_knockdown(d65, -1.0, -2.0)
    try:
        _refused(lambda: eng.score_rates(np.arange(65)[None], np.zeros((1, 65, 65)), -1.0, -2.0), _lib.NEMO_ERR_ARG, "S=65")
    finally:
        eng.close()
    # staged from tables, from log ratios, and an f32 context
    m = gr.get_model("small-S15-E17")
    pos, w = np.arange(15, dtype=np.int32)[None], np.zeros((1, 15, 15))
    r = np.where(rng.random((15, 17)) < 0.4, -2.0, 1.0)
    d15 = rr.small_d(15, 17)
    for make, code, match in ((lambda: Engine(m.U, m.T), _lib.NEMO_ERR_STATE, "knockdown"),
                              (lambda: Engine.from_log_ratios(r), _lib.NEMO_ERR_STATE, "knockdown"),
                              (lambda: Engine.from_knockdown(d15, -1.0, -2.0, dtype="f32"), _lib.NEMO_ERR_ARG, "f32")):
        eng = make()
        try:
            _refused(lambda: eng.score_rates(pos, w, -1.0, -2.0), code, match)
        finally:
            eng.close()
    # the host entry validates the rates; the device entry its batch and pointers
    eng = Engine.from_knockdown(d15, -1.0, -2.0)
    lib = _lib.load()
    try:
        for bad in (800.0, -800.0, float("nan"), float("inf")):
            av = np.full(15, -1.0)
            av[7] = bad
            _refused(lambda: eng.score_rates(pos, w, av, -2.0), _lib.NEMO_ERR_ARG, "rates")
            _refused(lambda: eng.score_rates(pos, w, -1.0, av), _lib.NEMO_ERR_ARG, "rates")
        _refused(lambda: eng.score_rates(np.zeros((1, 15), dtype=np.int32), w, -1.0, -2.0), _lib.NEMO_ERR_ARG, "permutation")
        eng.reserve(2)
        dpos = torch.from_numpy(np.tile(pos, (4, 1))).cuda()
        dw = torch.zeros((4, 15, 15), dtype=torch.float64, device="cuda")
        dr = torch.full((4, 2, 15), -1.5, dtype=torch.float64, device="cuda")
        dll = torch.zeros(4, dtype=torch.float64, device="cuda")
        ddr, dg = torch.zeros_like(dr), torch.zeros_like(dw)
        torch.cuda.synchronize()
        args = (dpos.data_ptr(), dw.data_ptr(), dr.data_ptr(), 0, dll.data_ptr(), ddr.data_ptr(), dg.data_ptr(), None)
        assert lib.nemo_score_rates_dev(eng.handle, 4, *args) == _lib.NEMO_ERR_STATE
        assert b"reserved" in lib.nemo_last_error()
        for k in (0, 1, 2, 4, 5):
            bad = list(args)
            bad[k] = None
            assert lib.nemo_score_rates_dev(eng.handle, 2, *bad) == _lib.NEMO_ERR_ARG, k
        assert lib.nemo_score_rates_dev(eng.handle, 2, *args[:3], -1, *args[4:]) == _lib.NEMO_ERR_ARG
        assert lib.nemo_score_rates_dev(eng.handle, 0, *args) == _lib.NEMO_OK
        assert lib.nemo_score_rates(eng.handle, 0, None, None, None, 0, None, None, None) == _lib.NEMO_OK
        assert lib.nemo_score_rates(eng.handle, 1, None, None, None, 0, None, None, None) == _lib.NEMO_ERR_ARG
        torch.cuda.synchronize()
        assert float(dg.abs().sum()) == 0.0 and float(dll.abs().sum()) == 0.0 and float(ddr.abs().sum()) == 0.0
    finally:
        eng.close()
