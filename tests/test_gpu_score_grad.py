"""nemo_score_grad / nemo_score_grad_dev (csrc/nemo_grad.hip) against the
long-double reference of tests/score_grad_ref.py (GPU).

Inputs: the error-rate ladder's rungs nem00 / nem04 / nem08 / nem12 at S = 16,
33, 60, 64 and E = 40, 130 (two bit words, a tile edge), three table-built
models, and seeded two-valued tables at S = 2, 15, 17 x E = 1, 15, 16, 17, 63,
64, 65 (row-block, tile and word boundaries) and at E = 1040 (two parts of
the fused kernel's cut of E) under the fused kernel and, with
option grad_path 1, the two-pass path; nem04 at S = 128 on the two-pass path
by itself; stream_models' real-valued tables (S = 2 to 65, E up to 4100, one
wide table) on the generic two-pass path.  Evaluations:
fixed_point_models.inputs (random orders, identity, reverse; soft, saturated,
all-0, all-1 and coin-flip weights), stream_models.evals for the generic
cases.

Per case and cap: |grad - ref| <= tol_ij everywhere (score_grad_ref's
tolerance, derived there; tests/test_score_grad_cpu.py holds numpy fp64 to a
quarter of it), ll within stream_models.tol_ll, exact zeros off the
permissible set, the same bits with NaN at every entry of w01 that is not
permissible, the same bits for a batch of one, for slots of a batch of 37 and
for a second run, fused and two-pass within 2 tol_ij of one another, and the
device entry on a side stream giving the host entry's bits.  Each case prints
its worst error over tolerance (pytest -s)."""
import numpy as np
import pytest

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


def _poisoned(w01, perms, cap):
    """w01 with NaN at every entry that is not a permissible pair."""
    w = w01.copy()
    for k, perm in enumerate(perms):
        w[k][~gr.permissible(perm, cap)] = np.nan
    return w


def _dev(eng, pos, w, cap):
    """nemo_score_grad_dev on a side torch stream, outputs preset to NaN."""
    import torch
    b = pos.shape[0]
    eng.reserve(b)
    side = torch.cuda.Stream()
    dpos, dw = torch.from_numpy(pos).cuda(), torch.from_numpy(w).cuda()
    dll = torch.full((b,), float("nan"), dtype=torch.float64, device="cuda")
    dg = torch.full((b, eng.S, eng.S), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        eng.score_grad_dev(b, dpos.data_ptr(), dw.data_ptr(), dll.data_ptr(), dg.data_ptr(), cap=cap,
                           stream=side.cuda_stream)
    side.synchronize()
    return dll.cpu().numpy(), dg.cpu().numpy()


def _against_ref(tag, ll, g, refs, perms, cap, factor=1.0):
    """-> worst err / tol; asserts the tolerance, finiteness and the exact zeros."""
    worst = 0.0
    for k, ref in enumerate(refs):
        ok = gr.permissible(perms[k], cap)
        assert np.isfinite(g[k]).all() and np.isfinite(ll[k]), (tag, cap, k)
        off = g[k][~ok]
        assert (off == 0.0).all() and not np.signbit(off).any(), (tag, cap, k, "entries off the permissible set")
        err = np.abs(g[k].astype(LD) - ref.g).astype(np.float64)
        if ok.any():
            ratio = err[ok] / ref.tol[ok]
            worst = max(worst, float(ratio.max()))
            assert (err[ok] <= factor * ref.tol[ok]).all(), (tag, cap, k, float(ratio.max()))
        assert abs(float(LD(ll[k]) - ref.cs.sum())) <= ref.tol_ll, (tag, cap, k, "ll")
    return worst


def _bits(eng, path, tag, pos, w01, perms, cap, ll, g):
    """NaN off the permissible set, batch of one, slots of a batch of 37, a second run, the device entry."""
    n = len(perms)
    l2, g2 = eng.score_grad(pos, _poisoned(w01, perms, cap), cap=cap)
    assert np.array_equal(l2, ll) and np.array_equal(g2, g), (tag, cap, "NaN off the permissible set")
    for one in (0, n - 1):
        l1, g1 = eng.score_grad(pos[one:one + 1], w01[one:one + 1], cap=cap)
        assert l1[0] == ll[one] and np.array_equal(g1[0], g[one]), (tag, cap, "batch of one", one)
    idx = (sm.tile_batch(n, 37) + 5) % n
    p37, w37 = np.ascontiguousarray(pos[idx]), np.ascontiguousarray(w01[idx])
    l37, g37 = eng.score_grad(p37, w37, cap=cap)
    assert np.array_equal(l37, ll[idx]) and np.array_equal(g37, g[idx]), (tag, cap, "batch of 37")
    l3, g3 = eng.score_grad(p37, w37, cap=cap)
    assert np.array_equal(l3, l37) and np.array_equal(g3, g37), (tag, cap, "second run")
    ld, gd = _dev(eng, p37, w37, cap)
    assert np.array_equal(ld, l37) and np.array_equal(gd, g37), (tag, cap, "device entry on a side stream")
    assert eng.get_option("grad_path_used") == path, (tag, cap)


@pytest.mark.parametrize("name", gr.factored_ids())
def test_factored_fused_and_two_pass(name):
    m, perms, pos, w01 = gr.factored_inputs(name)
    eng = _factored_engine(m)
    worst = {1: 0.0, 2: 0.0}
    try:
        for cap in gr.factored_caps(m.S):
            refs = gr.factored_refs(name, cap)
            got = {}
            for path, option in ((2, 0), (1, 1)):
                eng.set_option("grad_path", option)
                ll, g = eng.score_grad(pos, w01, cap=cap)
                assert eng.get_option("grad_path_used") == path, (name, cap)
                worst[path] = max(worst[path], _against_ref(f"{name} path {path}", ll, g, refs, perms, cap))
                _bits(eng, path, f"{name} path {path}", pos, w01, perms, cap, ll, g)
                got[path] = g
            for k, ref in enumerate(refs):
                assert (np.abs(got[2][k] - got[1][k]) <= 2.0 * ref.tol).all(), (name, cap, k, "fused against two-pass")
    finally:
        eng.close()
    print(f"GRAD {name} worst err/tol: fused {worst[2]:.3f} two-pass {worst[1]:.3f}")


def test_factored_past_64_takes_the_two_pass_path():
    name = gr.WIDE_MODEL
    m, perms, pos, w01 = gr.factored_inputs(name)
    eng = _factored_engine(m)
    worst = 0.0
    try:
        for cap in gr.factored_caps(m.S):
            ll, g = eng.score_grad(pos, w01, cap=cap)
            assert eng.get_option("grad_path_used") == 1
            worst = max(worst, _against_ref(name, ll, g, gr.factored_refs(name, cap), perms, cap))
            _bits(eng, 1, name, pos, w01, perms, cap, ll, g)
    finally:
        eng.close()
    print(f"GRAD {name} worst err/tol: two-pass {worst:.3f}")


@pytest.mark.parametrize("name", gr.GENERIC)
def test_generic_tables(name):
    c, _, _, perms, pos, w01 = gr.generic_inputs(name)
    eng = _generic_engine(c)
    worst = 0.0
    try:
        for cap in gr.generic_caps(c.s):
            ll, g = eng.score_grad(pos, w01, cap=cap)
            assert eng.get_option("grad_path_used") == 1
            worst = max(worst, _against_ref(name, ll, g, gr.generic_refs(name, cap), perms, cap))
            _bits(eng, 1, name, pos, w01, perms, cap, ll, g)
    finally:
        eng.close()
    print(f"GRAD {name} worst err/tol: two-pass {worst:.3f}")


@pytest.mark.parametrize("s", [16, 33, 64])
def test_fragment_layout_on_integer_data(s):
    """The second contraction on exact integers.  At weights 0 the cells are U; with U = 0 at one
    child a(e) per effect and -2000 elsewhere the order weights are 1 at (a(e), e) and exactly 0
    elsewhere, so M[i][j] = #{e: a(e) = i, D1[j][e]} is an integer matrix with no symmetry, and
    with lo_j = 0 (f'_lo = 0) the gradient is (e^hi_j - 1) M[i][j]: a transposed or mis-laned
    fragment moves it by whole counts.  Every accumulator tile of S = 64 is met."""
    e = 130
    rng = np.random.default_rng(60 + s)
    bits = rng.random((s, e)) < 0.5
    bits[:, 0] = False
    hi = rng.uniform(0.5, 2.0, s)
    t = np.empty((s, s, e))
    t[:] = np.where(bits, hi[:, None], 0.0)[None]
    a = rng.integers(s, size=e)
    u = np.full((s + 1, e), -2000.0)
    u[a, np.arange(e)] = 0.0
    counts = np.zeros((s, s))
    for k in range(e):
        counts[a[k]] += bits[:, k]
    assert not np.array_equal(counts, counts.T)
    perms = [rng.permutation(s), np.arange(s)[::-1].copy(), rng.permutation(s)]
    pos = np.empty((3, s), dtype=np.int32)
    for k, p in enumerate(perms):
        pos[k, p] = np.arange(s)
    eng = Engine(u, t)
    try:
        assert eng.factored
        for path, option in ((2, 0), (1, 1)):
            eng.set_option("grad_path", option)
            ll, g = eng.score_grad(pos, np.zeros((3, s, s)))
            assert eng.get_option("grad_path_used") == path
            assert np.abs(ll).max() <= 1e-12
            for k, perm in enumerate(perms):
                want = np.where(gr.permissible(perm), np.expm1(hi)[None, :] * counts, 0.0)
                assert (np.abs(g[k] - want) <= 1e-12 * np.maximum(1.0, want)).all(), (s, path, k)
    finally:
        eng.close()


def test_entry_checks():
    import torch
    m, _, pos, w01 = gr.factored_inputs("small-S15-E17")
    lib = _lib.load()
    f32 = Engine(m.U, m.T, dtype="f32")
    try:
        with pytest.raises(RuntimeError, match="f32") as ei:
            f32.score_grad(pos, w01)
        assert ei.value.code == _lib.NEMO_ERR_ARG
    finally:
        f32.close()
    eng = _factored_engine(m)
    try:
        b = pos.shape[0]
        eng.reserve(b)
        dpos, dw = torch.from_numpy(np.tile(pos, (2, 1))).cuda(), torch.from_numpy(np.tile(w01, (2, 1, 1))).cuda()
        dll = torch.zeros(2 * b, dtype=torch.float64, device="cuda")
        dg = torch.zeros((2 * b, m.S, m.S), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        args = (dpos.data_ptr(), dw.data_ptr(), 0, dll.data_ptr(), dg.data_ptr(), None)
        assert lib.nemo_score_grad_dev(eng.handle, 2 * b, *args) == _lib.NEMO_ERR_STATE
        assert b"reserved" in lib.nemo_last_error()
        for k in (0, 1, 3, 4):
            a = list(args)
            a[k] = None
            assert lib.nemo_score_grad_dev(eng.handle, b, *a) == _lib.NEMO_ERR_ARG, k
        assert lib.nemo_score_grad_dev(eng.handle, 0, *args) == _lib.NEMO_OK
        assert lib.nemo_score_grad(eng.handle, 0, None, None, 0, None, None) == _lib.NEMO_OK
        assert lib.nemo_score_grad(eng.handle, 1, None, None, 0, None, None) == _lib.NEMO_ERR_ARG
        with pytest.raises(_lib.NemoError):
            eng.set_option("grad_path", 2)
        torch.cuda.synchronize()
        assert float(dg.abs().sum()) == 0.0 and float(dll.abs().sum()) == 0.0   # no refused call wrote anything
    finally:
        eng.close()
